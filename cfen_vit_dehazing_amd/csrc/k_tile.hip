// Overlapping-tile inference for images of any size (tiled.py): the generator's image size is baked in (learned positional tables and
// F.fold(..., img_dim), v3:1125-1127, 1186, 1321), so an H x W image is cut into T x T tiles, T = cfg.image_size, that run through the
// unchanged forward in batches and are blended back.
//
// Tile plan, per axis of extent L (tiled.tile_grid is the host twin):
//   n   = 1 if L <= T else 1 + ceil((L - T) / (T - o))          (the host picks n; the kernels take it as an argument)
//   p_j = (j * (L - T)) // (n - 1)  (n > 1), p_0 = 0            (origins spread evenly, the last tile flush with the edge)
//   tile pixel (u, v) of tile (i, j) reads source (mirror(p_i + u, H), mirror(q_j + v, W)), numpy 'reflect' (only when L < T)
//   blend weight w(u) = min(1, (min(u, e - 1 - u) + 1) / (o + 1)), e = min(T, L); a tile's weight is w_y * w_x
//   output = the tile value where one tile covers the pixel, else sum(w v) / sum(w) in fp32 over the covering tiles in increasing t = i nx + j
//
//   k_tile_gather : one batch [t0, t0 + B) of tiles -> the network's input slab ((B,T,T,3) uint8 or (B,3,T,T) fp32); tiles past the last
//                   repeat it, so the last batch is full and the batch-B launch plan is reused.  A pure copy.
//   k_tile_blend  : pull form, PX output pixels per thread; reads the covering tiles straight from the forwards' own output slabs placed one
//                   after another (the "arena": slab s = tiles [s B, s B + B), each [xr (B,3,T,T) | xs (B,1,T,T) | xd (B,3,T,T)]).  No atomics,
//                   fixed summation order: run-to-run bitwise.  lane0 > 0: the image shares its slabs with other images (tiled.pack_plan) and
//                   its tile t sits at global slot lane0 + t, slab (lane0 + t) / B, lane (lane0 + t) % B.
#include "cfen_common.hpp"

namespace {

CFEN_DEV int tile_origin(int j, int n, int L, int T) { return n > 1 ? (int)(((long long)j * (L - T)) / (n - 1)) : 0; }

// numpy 'reflect' (the edge pixel is not repeated), periodic with period 2 (L - 1); k >= 0
CFEN_DEV int mirror(int k, int L) {
  if (L == 1) return 0;
  const int period = 2 * (L - 1);
  k %= period;
  return k < L ? k : period - k;
}

// tiles [lo, hi] of an axis that cover coordinate y: p_i <= y < p_i + T.  p_i = floor(i D / (n - 1)), D = L - T > 0 when n > 1
CFEN_DEV void tile_cover(int y, int n, int L, int T, int& lo, int& hi) {
  if (n == 1) {
    lo = hi = 0;
    return;
  }
  const long long D = L - T, m = n - 1;
  // largest i with i D <= (y + 1) m - 1
  long long h = ((long long)(y + 1) * m - 1) / D;
  hi = (int)(h < m ? h : m);
  // smallest i with floor(i D / m) >= y - T + 1
  const long long k = (long long)y - T + 1;
  lo = k <= 0 ? 0 : (int)((k * m + D - 1) / D);
}

CFEN_DEV float tile_weight(int u, int e, int o) {
  const int d = min(u, e - 1 - u);
  return fminf(1.f, (float)(d + 1) / (float)(o + 1));
}

struct TileGeom {
  int H, W, T, ny, nx;
};

// uint8 (H,W,3) -> (B,T,T,3): 16 tile pixels = 48 bytes per thread, three 16-byte stores (T % 16 == 0, dst 16-byte aligned)
__global__ __launch_bounds__(256) void k_tile_gather_u8(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, TileGeom g,
                                                        int t0, int B) {
  const int T = g.T, ntiles = g.ny * g.nx;
  const long long ngroups = (long long)B * T * (T / 16);
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (long long)gridDim.x * 256) {
    const int v0 = (int)(q % (T / 16)) * 16;
    const long long r = q / (T / 16);
    const int u = (int)(r % T), b = (int)(r / T);
    const int t = min(t0 + b, ntiles - 1);
    const int i = t / g.nx, j = t - i * g.nx;
    const int y = mirror(tile_origin(i, g.ny, g.H, T) + u, g.H);
    const int qx = tile_origin(j, g.nx, g.W, T);
    const unsigned char* row = src + (long long)y * g.W * 3;
    union { unsigned char c[48]; uint4 v[3]; } buf;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int x = mirror(qx + v0 + e, g.W);
      buf.c[3 * e] = row[3 * x];
      buf.c[3 * e + 1] = row[3 * x + 1];
      buf.c[3 * e + 2] = row[3 * x + 2];
    }
    uint4* o = reinterpret_cast<uint4*>(dst + (((long long)b * T + u) * T + v0) * 3);
    o[0] = buf.v[0];
    o[1] = buf.v[1];
    o[2] = buf.v[2];
  }
}

// fp32 (3,H,W) -> (B,3,T,T): 4 tile pixels of one channel row per thread, one 16-byte store
__global__ __launch_bounds__(256) void k_tile_gather_f32(const float* __restrict__ src, float* __restrict__ dst, TileGeom g, int t0, int B) {
  const int T = g.T, ntiles = g.ny * g.nx;
  const long long ngroups = (long long)B * 3 * T * (T / 4);
  const long long plane = (long long)g.H * g.W;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (long long)gridDim.x * 256) {
    const int v0 = (int)(q % (T / 4)) * 4;
    long long r = q / (T / 4);
    const int u = (int)(r % T);
    r /= T;
    const int c = (int)(r % 3), b = (int)(r / 3);
    const int t = min(t0 + b, ntiles - 1);
    const int i = t / g.nx, j = t - i * g.nx;
    const int y = mirror(tile_origin(i, g.ny, g.H, T) + u, g.H);
    const int qx = tile_origin(j, g.nx, g.W, T);
    const float* row = src + c * plane + (long long)y * g.W;
    float4 o;
    o.x = row[mirror(qx + v0, g.W)];
    o.y = row[mirror(qx + v0 + 1, g.W)];
    o.z = row[mirror(qx + v0 + 2, g.W)];
    o.w = row[mirror(qx + v0 + 3, g.W)];
    *reinterpret_cast<float4*>(dst + (((long long)b * 3 + c) * T + u) * T + v0) = o;
  }
}

CFEN_DEV float ld(const float* p) { return *p; }
CFEN_DEV float ld(const half_t* p) { return (float)*p; }

CFEN_DEV unsigned char to_u8(float v) { return (unsigned char)(int)((v + 1.f) / 2.0f * 255.0f); }   // k_tensor2im_u8 (k_tokens.hip)

// the 7 blended planes [xr0 xr1 xr2 xs xd0 xd1 xd2] of output pixel (y, x); the image's tile t sits at global slot lane0 + t of the arena
template <typename TA>
CFEN_DEV void blend_pixel(const TA* __restrict__ arena, int B, int lane0, const TileGeom& g, int o, int y, int x, float (&val)[7]) {
  const int T = g.T;
  const long long TT = (long long)T * T, slab = 7 * (long long)B * TT;
  int ilo, ihi, jlo, jhi;
  tile_cover(y, g.ny, g.H, T, ilo, ihi);
  tile_cover(x, g.nx, g.W, T, jlo, jhi);
  if (ilo == ihi && jlo == jhi) {          // one tile: its value unchanged (bitwise the plain forward where the image is T x T)
    const int t = lane0 + ilo * g.nx + jlo, s = t % B;
    const TA* base = arena + (long long)(t / B) * slab + (long long)(y - tile_origin(ilo, g.ny, g.H, T)) * T + (x - tile_origin(jlo, g.nx, g.W, T));
#pragma unroll
    for (int c = 0; c < 3; ++c) val[c] = ld(base + ((long long)s * 3 + c) * TT);
    val[3] = ld(base + (3 * (long long)B + s) * TT);
#pragma unroll
    for (int c = 0; c < 3; ++c) val[4 + c] = ld(base + (4 * (long long)B + (long long)s * 3 + c) * TT);
    return;
  }
  const int ey = min(T, g.H), ex = min(T, g.W);
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, wsum = 0.f;
  for (int i = ilo; i <= ihi; ++i) {
    const int u = y - tile_origin(i, g.ny, g.H, T);
    const float wy = tile_weight(u, ey, o);
    for (int j = jlo; j <= jhi; ++j) {
      const int v = x - tile_origin(j, g.nx, g.W, T);
      const float w = wy * tile_weight(v, ex, o);
      const int t = lane0 + i * g.nx + j, s = t % B;
      const TA* base = arena + (long long)(t / B) * slab + (long long)u * T + v;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += w * ld(base + ((long long)s * 3 + c) * TT);
      acc[3] += w * ld(base + (3 * (long long)B + s) * TT);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[4 + c] += w * ld(base + (4 * (long long)B + (long long)s * 3 + c) * TT);
      wsum += w;
    }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) val[c] = acc[c] / wsum;
}

// fp32 planar outputs xr (3,H,W), xs (1,H,W), xd (3,H,W): 4 consecutive pixels of the flattened plane per thread, one 16-byte store per
// plane (outputs 16-byte aligned; element by element at the ragged end of the plane, and everywhere when H W % 4 != 0 leaves the second and
// third planes of xr / xd unaligned)
template <typename TA>
__global__ __launch_bounds__(256) void k_tile_blend_f32(const TA* __restrict__ arena, int B, int lane0, TileGeom g, int o, float* __restrict__ xr,
                                                        float* __restrict__ xs, float* __restrict__ xd) {
  const long long npix = (long long)g.H * g.W, ngroups = (npix + 3) / 4;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (long long)gridDim.x * 256) {
    const long long p0 = q * 4;
    float val[4][7] = {};
    int y = (int)(p0 / g.W), x = (int)(p0 - (long long)y * g.W);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (p0 + e < npix) blend_pixel(arena, B, lane0, g, o, y, x, val[e]);
      if (++x == g.W) { x = 0; ++y; }
    }
    float* planes[7] = {xr, xr + npix, xr + 2 * npix, xs, xd, xd + npix, xd + 2 * npix};
    if (p0 + 4 <= npix && npix % 4 == 0) {
#pragma unroll
      for (int c = 0; c < 7; ++c) *reinterpret_cast<float4*>(planes[c] + p0) = make_float4(val[0][c], val[1][c], val[2][c], val[3][c]);
    } else {
      for (int e = 0; e < 4 && p0 + e < npix; ++e)
#pragma unroll
        for (int c = 0; c < 7; ++c) planes[c][p0 + e] = val[e][c];
    }
  }
}

// three (H,W,3) uint8 images with util.tensor2im's arithmetic (xs tiled to 3 channels): 16 pixels per thread = 48 bytes per image, three
// 16-byte stores each (outputs 16-byte aligned; the ragged end byte by byte)
template <typename TA>
__global__ __launch_bounds__(256) void k_tile_blend_u8(const TA* __restrict__ arena, int B, int lane0, TileGeom g, int o, unsigned char* __restrict__ xr,
                                                       unsigned char* __restrict__ xs, unsigned char* __restrict__ xd) {
  const long long npix = (long long)g.H * g.W, ngroups = (npix + 15) / 16;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ngroups; q += (long long)gridDim.x * 256) {
    const long long p0 = q * 16;
    union { unsigned char c[48]; uint4 v[3]; } br, bs, bd;
    int y = (int)(p0 / g.W), x = (int)(p0 - (long long)y * g.W);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      float val[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (p0 + e < npix) blend_pixel(arena, B, lane0, g, o, y, x, val);
      if (++x == g.W) { x = 0; ++y; }
      const unsigned char s = to_u8(val[3]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        br.c[3 * e + c] = to_u8(val[c]);
        bs.c[3 * e + c] = s;
        bd.c[3 * e + c] = to_u8(val[4 + c]);
      }
    }
    if (p0 + 16 <= npix) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        reinterpret_cast<uint4*>(xr + p0 * 3)[k] = br.v[k];
        reinterpret_cast<uint4*>(xs + p0 * 3)[k] = bs.v[k];
        reinterpret_cast<uint4*>(xd + p0 * 3)[k] = bd.v[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 48; ++k) {            // (constant indices: the staging stays in registers)
        if (p0 * 3 + k < npix * 3) {
          xr[p0 * 3 + k] = br.c[k];
          xs[p0 * 3 + k] = bs.c[k];
          xd[p0 * 3 + k] = bd.c[k];
        }
      }
    }
  }
}

inline unsigned tile_grid_for(long long n) {
  long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

long long tile_count(int L, int T, int o) { return L <= T ? 1 : 1 + ((long long)L - T + (T - o) - 1) / (T - o); }

// the origins (tile_origin) must stay >= 0 and every pixel of the axis must lie in some tile
bool axis_ok(int L, int T, int n) { return L <= T ? n == 1 : (n >= 2 && (long long)n * T >= L); }

}  // namespace

// dimensions are capped so that every index product above fits its type and an image of the cap is far past any arena a device holds
#define CFEN_TILE_MAX_EDGE 65536

int cfen_tile_gather_impl(int u8, const void* src, void* dst, int H, int W, int T, int ny, int nx, int t0, int B, hipStream_t s) {
  CFEN_CHECK_ARG(src && dst, "tile_gather: null pointer");
  CFEN_CHECK_ARG(u8 == 0 || u8 == 1, "tile_gather: u8 must be 0 or 1");
  CFEN_CHECK_ARG(T >= 16 && T % 16 == 0 && T <= 8192, "tile_gather: tile edge T = %d must be a multiple of 16 in 16 .. 8192", T);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= CFEN_TILE_MAX_EDGE && W <= CFEN_TILE_MAX_EDGE, "tile_gather: image size %d x %d outside 1 .. %d", H, W,
                 CFEN_TILE_MAX_EDGE);
  CFEN_CHECK_ARG(axis_ok(H, T, ny) && axis_ok(W, T, nx), "tile_gather: a %d x %d grid of %d x %d tiles does not tile a %d x %d image", ny, nx, T, T,
                 H, W);
  CFEN_CHECK_ARG((long long)ny * nx <= (1 << 24), "tile_gather: %d x %d tiles is too many", ny, nx);
  CFEN_CHECK_ARG(B >= 1 && B <= 65536 && t0 >= 0 && t0 < ny * nx, "tile_gather: batch [%d, %d + %d) outside the %d tiles", t0, t0, B, ny * nx);
  CFEN_CHECK_ARG(cfen_aligned16(dst), "tile_gather: dst must be 16-byte aligned");
  const TileGeom g = {H, W, T, ny, nx};
  if (u8) {
    CFEN_LAUNCH(k_tile_gather_u8, dim3(tile_grid_for((long long)B * T * (T / 16))), dim3(256), 0, s, (const unsigned char*)src, (unsigned char*)dst,
                g, t0, B);
  } else {
    CFEN_LAUNCH(k_tile_gather_f32, dim3(tile_grid_for((long long)B * 3 * T * (T / 4))), dim3(256), 0, s, (const float*)src, (float*)dst, g, t0, B);
  }
  CFEN_CHECK_LAUNCH("tile_gather");
  return CFEN_OK;
}

int cfen_tile_blend_impl(int dtype, const void* arena, int B, int T, int H, int W, int ny, int nx, int overlap, int out_u8, void* xr, void* xs,
                         void* xd, hipStream_t s) {
  CFEN_CHECK_ARG(arena && xr && xs && xd, "tile_blend: null pointer");
  // dtype packs two fields (cfen_hip.h): bits 0..7 the arena element type, bits 8..23 lane0, the lane of the image's tile 0 in its slab
  CFEN_CHECK_ARG(dtype >= 0 && (dtype >> 24) == 0, "tile_blend: bits 24 and up of dtype = 0x%x must be zero", (unsigned)dtype);
  const int lane0 = (dtype >> 8) & 0xffff;
  dtype &= 0xff;
  CFEN_CHECK_ARG(dtype == 0 || dtype == 1, "tile_blend: unknown arena dtype %d", dtype);
  CFEN_CHECK_ARG(out_u8 == 0 || out_u8 == 1, "tile_blend: out_u8 must be 0 or 1");
  CFEN_CHECK_ARG(T >= 2 && T <= 8192 && B >= 1 && B <= 65536, "tile_blend: bad tile edge T = %d or batch B = %d", T, B);
  CFEN_CHECK_ARG(lane0 < B, "tile_blend: lane0 = %d outside the slab's lanes 0 .. %d", lane0, B - 1);
  CFEN_CHECK_ARG(overlap >= 0 && 2 * overlap <= T, "tile_blend: overlap %d outside 0 .. T/2 = %d", overlap, T / 2);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= CFEN_TILE_MAX_EDGE && W <= CFEN_TILE_MAX_EDGE, "tile_blend: image size %d x %d outside 1 .. %d", H, W,
                 CFEN_TILE_MAX_EDGE);
  CFEN_CHECK_ARG(ny == tile_count(H, T, overlap) && nx == tile_count(W, T, overlap),
                 "tile_blend: a %d x %d grid is not the plan of a %d x %d image with %d x %d tiles and overlap %d (%lld x %lld)", ny, nx, H, W, T, T,
                 overlap, tile_count(H, T, overlap), tile_count(W, T, overlap));
  CFEN_CHECK_ARG(cfen_aligned16(xr) && cfen_aligned16(xs) && cfen_aligned16(xd), "tile_blend: outputs must be 16-byte aligned");
  const TileGeom g = {H, W, T, ny, nx};
  const long long npix = (long long)H * W;
  if (out_u8) {
    const dim3 grid(tile_grid_for((npix + 15) / 16));
    if (dtype == 1)
      CFEN_LAUNCH(k_tile_blend_u8<half_t>, grid, dim3(256), 0, s, (const half_t*)arena, B, lane0, g, overlap, (unsigned char*)xr, (unsigned char*)xs,
                  (unsigned char*)xd);
    else
      CFEN_LAUNCH(k_tile_blend_u8<float>, grid, dim3(256), 0, s, (const float*)arena, B, lane0, g, overlap, (unsigned char*)xr, (unsigned char*)xs,
                  (unsigned char*)xd);
  } else {
    const dim3 grid(tile_grid_for((npix + 3) / 4));
    if (dtype == 1)
      CFEN_LAUNCH(k_tile_blend_f32<half_t>, grid, dim3(256), 0, s, (const half_t*)arena, B, lane0, g, overlap, (float*)xr, (float*)xs, (float*)xd);
    else
      CFEN_LAUNCH(k_tile_blend_f32<float>, grid, dim3(256), 0, s, (const float*)arena, B, lane0, g, overlap, (float*)xr, (float*)xs, (float*)xd);
  }
  CFEN_CHECK_LAUNCH("tile_blend");
  return CFEN_OK;
}
