// No-reference statistics of a hazy image and its dehazed output (include/cfen_noref.h states the definition and the contract; tests/noref_ref.py
// restates it in numpy).  Scored under test.py --eval_noref (metrics.noref, ops.image_noref); ops.dark_channel_u8 uses the map alone.
//
//   k_noref        : a workgroup (256 threads, 4 waves) owns ONE tile of NR_TW x NR_TH pixels of one image pair.  Per side (hazy, then out) it
//                    fills the haloed min(R, G, B) plane in LDS with 255 (the identity of min: the window is clipped to the image), fetches the
//                    tile plus a halo of r pixels (lower / right halo max(r, 1): the gradient needs one neighbour) row by row in groups of four
//                    linear pixel indices p = image address (mod 4) -- such a group starts on a 4-byte boundary whatever the image's alignment,
//                    so three dword loads fetch it when it lies inside the image, single bytes otherwise -- and writes min(R, G, B) and the luma
//                    as bytes.  Row minimum over 2r + 1 columns into a second plane, column minimum over 2r + 1 rows from it; the map is stored
//                    as bytes.  Both lumas stay in LDS; afterwards every thread walks its 16 pixels: two histogram atomics (LDS, integer), the
//                    saturation tests and the two gradient terms in fp64.  Integer sums go through LDS atomics (order-free), the gradient sums
//                    through a shuffle butterfly and then the four waves in wave order.  One record per workgroup.
//   k_noref_finish : grid (B, 2, 17).  z < 16: 16 bins x 16 record lanes, a lane adds records lane, lane + 16, ... of its bin in uint64, the 16
//                    lanes are added through LDS.  z == 16: dark_sum and the saturation count the same way over 256 lanes, and the gradient
//                    partials in the fixed order of img_reduce_partials (cfen_image.hpp), interleaved with the integer sums.
// Two launches; no global atomics, no counters; LDS 26.4 KB per workgroup.
#include <math.h>

#include "../../include/cfen_noref.h"
#include "cfen_image.hpp"

namespace {

constexpr int NR_TW = CFEN_NOREF_TILE_W, NR_TH = CFEN_NOREF_TILE_H;
constexpr int NR_MAXR = CFEN_NOREF_MAX_RADIUS;
constexpr int NR_LW = NR_TW + 2 * NR_MAXR, NR_LH = NR_TH + 2 * NR_MAXR;      // the haloed plane: 96 x 96 bytes
constexpr int NR_YS = 68;                                                    // row stride of the (NR_TH + 1) x (NR_TW + 1) luma planes
constexpr int NR_GROUPS = (NR_LW + 3 + 3) / 4;                               // four-pixel groups that can touch one haloed row: 25
constexpr int NR_PIX = NR_TW * NR_TH / 256;                                  // tile pixels per thread: 16
constexpr int NR_COLS = 258;                                                 // integer columns of one side: 256 bins, dark_sum, sat
constexpr int NR_MAX_EDGE = 65536;
constexpr int NR_MAX_BATCH = 65535;                                          // grid.y

static_assert(CFEN_NOREF_RECORD_BYTES == 2 * NR_COLS * 4 + 2 * 8, "record layout");
static_assert((2 * NR_COLS * 4) % 8 == 0, "the doubles of a record are 8-byte aligned");
static_assert(NR_TW == 64 && NR_TW * NR_TH % 256 == 0 && NR_LW % 4 == 0, "tile shape");

struct NrRecord {
  unsigned cnt[2][NR_COLS];
  double grad[2];
};
static_assert(sizeof(NrRecord) == CFEN_NOREF_RECORD_BYTES, "record size");

union NrBytes {
  unsigned u[3];
  unsigned char c[12];
};

CFEN_DEV unsigned nr_min3(unsigned a, unsigned b, unsigned c) { return min(a, min(b, c)); }

__global__ __launch_bounds__(256) void k_noref(const unsigned char* __restrict__ hazy, const unsigned char* __restrict__ out, int H, int W, int r,
                                               int tiles_x, unsigned char* __restrict__ dark0, unsigned char* __restrict__ dark1,
                                               NrRecord* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) unsigned char mn[NR_LH][NR_LW];      // min(R, G, B) of the haloed tile; 255 outside the image
  __shared__ __attribute__((aligned(16))) unsigned char rm[NR_LH][NR_TW];      // its row minimum
  __shared__ unsigned char ly_[2][NR_TH + 1][NR_YS];                          // luma of the tile plus one column / row, both sides
  __shared__ unsigned hist[2][256];
  __shared__ unsigned isum[4];                                                 // dark_sum 0, dark_sum 1, sat_in, sat_new
  __shared__ double red[2][4];
  const int tid = threadIdx.x, img = blockIdx.y;
  const int tile = blockIdx.x, x0 = (tile % tiles_x) * NR_TW, y0 = (tile / tiles_x) * NR_TH;
  const long long npix = (long long)H * W;
  const int hi = r > 0 ? r : 1;                                                // lower / right halo
  hist[0][tid] = 0u;
  hist[1][tid] = 0u;
  if (tid < 4) isum[tid] = 0u;
  // the columns this tile fetches: [xs, xe), clipped to the image
  const int xs = max(x0 - r, 0), xe = min(x0 + NR_TW + hi, W);

  for (int side = 0; side < 2; ++side) {
    const unsigned char* __restrict__ src = (side == 0 ? hazy : out) + (size_t)img * (size_t)npix * 3;
    unsigned char* __restrict__ dmap = side == 0 ? dark0 : dark1;
    const int a = (int)(reinterpret_cast<uintptr_t>(src) & 3);                 // block-uniform: pixel groups p = a (mod 4) are dword aligned
    for (int i = tid; i < NR_LH * NR_LW / 4; i += 256) reinterpret_cast<unsigned*>(&mn[0][0])[i] = 0xffffffffu;
    __syncthreads();
    // fetch: item = (row of the haloed tile, group of four linear pixel indices)
    for (int item = tid; item < NR_LH * NR_GROUPS; item += 256) {
      const int ly = item / NR_GROUPS, g = item % NR_GROUPS;
      const int gy = y0 - r + ly;
      if (ly >= NR_TH + r + hi || gy < 0 || gy >= H) continue;
      const long long L0 = (long long)gy * W + xs, L1 = (long long)gy * W + xe;      // linear indices of the row's span
      const long long gp = L0 - ((L0 - a) & 3) + 4 * g;                       // first index of the group: gp = a (mod 4), gp <= L0 for g = 0
      if (gp >= L1) continue;
      NrBytes v;
      v.u[0] = v.u[1] = v.u[2] = 0u;
      if (gp >= 0 && gp + 4 <= npix) {                                         // wholly inside the image's memory (it may leave the span)
        const unsigned* p = reinterpret_cast<const unsigned*>(src + gp * 3);   // 3 gp + address = 4 a = 0 (mod 4)
        v.u[0] = p[0];
        v.u[1] = p[1];
        v.u[2] = p[2];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (gp + j >= L0 && gp + j < L1) {
            v.c[3 * j] = src[(gp + j) * 3];
            v.c[3 * j + 1] = src[(gp + j) * 3 + 1];
            v.c[3 * j + 2] = src[(gp + j) * 3 + 2];
          }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long p = gp + j;
        if (p < L0 || p >= L1) continue;
        const int lx = (int)(p - L0) + xs - (x0 - r);                          // column of the haloed tile: < NR_TW + r + hi <= NR_LW
        const unsigned R = v.c[3 * j], G = v.c[3 * j + 1], Bc = v.c[3 * j + 2];
        mn[ly][lx] = (unsigned char)nr_min3(R, G, Bc);
        const int ty = ly - r, tx = lx - r;
        if (ty >= 0 && tx >= 0 && ty <= NR_TH && tx <= NR_TW) ly_[side][ty][tx] = (unsigned char)((77u * R + 150u * G + 29u * Bc + 128u) >> 8);
      }
    }
    __syncthreads();
    // row minimum: rm[ly][tx] = min of mn[ly][tx .. tx + 2r]
    for (int i = tid; i < (NR_TH + 2 * r) * NR_TW; i += 256) {
      const int ly = i / NR_TW, tx = i % NR_TW;
      unsigned m = 255u;
      for (int k = 0; k <= 2 * r; ++k) m = min(m, (unsigned)mn[ly][tx + k]);
      rm[ly][tx] = (unsigned char)m;
    }
    __syncthreads();
    // column minimum, the map and dark_sum
    unsigned dsum = 0u;
#pragma unroll 4
    for (int k = 0; k < NR_PIX; ++k) {
      const int i = tid + 256 * k, ty = i / NR_TW, tx = i % NR_TW;
      const int gy = y0 + ty, gx = x0 + tx;
      if (gy >= H || gx >= W) continue;
      unsigned m = 255u;
      for (int q = 0; q <= 2 * r; ++q) m = min(m, (unsigned)rm[ty + q][tx]);
      dsum += m;
      if (dmap != nullptr) dmap[(size_t)img * (size_t)npix + (size_t)gy * W + gx] = (unsigned char)m;
    }
    atomicAdd(&isum[side], dsum);
    // (the next side's fill of mn follows reads of rm only; its fetch and row minimum come after barriers that all of these reads precede)
  }

  // histograms, saturation and gradients from the two luma planes (complete since the barrier after the second fetch)
  double g0 = 0.0, g1 = 0.0;
  unsigned sat_in = 0u, sat_new = 0u;
#pragma unroll 4
  for (int k = 0; k < NR_PIX; ++k) {
    const int i = tid + 256 * k, ty = i / NR_TW, tx = i % NR_TW;
    const int gy = y0 + ty, gx = x0 + tx;
    if (gy >= H || gx >= W) continue;
    const int yh = ly_[0][ty][tx], yo = ly_[1][ty][tx];
    atomicAdd(&hist[0][yh], 1u);
    atomicAdd(&hist[1][yo], 1u);
    const bool sh = yh == 0 || yh == 255, so = yo == 0 || yo == 255;
    sat_in += sh ? 1u : 0u;
    sat_new += (so && !sh) ? 1u : 0u;
    if (gy + 1 < H && gx + 1 < W) {
      const int dx0 = (int)ly_[0][ty][tx + 1] - yh, dy0 = (int)ly_[0][ty + 1][tx] - yh;
      const int dx1 = (int)ly_[1][ty][tx + 1] - yo, dy1 = (int)ly_[1][ty + 1][tx] - yo;
      g0 += sqrt(0.5 * (double)(dx0 * dx0 + dy0 * dy0));
      g1 += sqrt(0.5 * (double)(dx1 * dx1 + dy1 * dy1));
    }
  }
  atomicAdd(&isum[2], sat_in);
  atomicAdd(&isum[3], sat_new);
  g0 = wave_sum(g0);
  g1 = wave_sum(g1);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = g0;
    red[1][tid >> 6] = g1;
  }
  __syncthreads();
  NrRecord* o = rec + ((size_t)img * gridDim.x + blockIdx.x);
  o->cnt[0][tid] = hist[0][tid];
  o->cnt[1][tid] = hist[1][tid];
  if (tid < 2) {
    o->cnt[tid][256] = isum[tid];
    o->cnt[tid][257] = isum[2 + tid];
    o->grad[tid] = block4_sum(red[tid], 1);
  }
}

__global__ __launch_bounds__(256) void k_noref_finish(const NrRecord* __restrict__ rec, int nrec, unsigned long long* __restrict__ counts,
                                                      double* __restrict__ grad) {
  __shared__ unsigned long long isum[2][256];
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.x, side = blockIdx.y, z = blockIdx.z;
  const NrRecord* p = rec + (size_t)b * nrec;
  unsigned long long* c = counts + ((size_t)b * 2 + side) * 259;
  if (z < 16) {                                                                // block-uniform
    const int bin = 16 * z + (tid & 15), lane = tid >> 4;
    unsigned long long s = 0ull;
    for (int i = lane; i < nrec; i += 16) s += p[i].cnt[side][bin];
    isum[0][tid] = s;
    __syncthreads();
    if (tid < 16) {
      unsigned long long t = 0ull;
      for (int l = 0; l < 16; ++l) t += isum[0][16 * l + tid];
      c[16 * z + tid] = t;
    }
    return;
  }
  unsigned long long s0 = 0ull, s1 = 0ull;
  double s = 0.0;
  for (int i = tid; i < nrec; i += 256) {
    s0 += p[i].cnt[side][256];
    s1 += p[i].cnt[side][257];
    s += p[i].grad[side];
  }
  isum[0][tid] = s0;
  isum[1][tid] = s1;
  red[tid] = s;
  __syncthreads();
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) {
      isum[0][tid] += isum[0][tid + n];
      isum[1][tid] += isum[1][tid + n];
      red[tid] += red[tid + n];
    }
    __syncthreads();
  }
  if (tid == 0) {
    c[256] = isum[0][0];
    c[257] = isum[1][0];
    c[258] = 0ull;
    grad[(size_t)b * 2 + side] = red[0];
  }
}

bool nr_dims_ok(int B, int H, int W, int r) {
  return B >= 1 && B <= NR_MAX_BATCH && H >= 1 && W >= 1 && H <= NR_MAX_EDGE && W <= NR_MAX_EDGE && r >= 0 && r <= NR_MAXR;
}

int nr_tiles_x(int W) { return (W + NR_TW - 1) / NR_TW; }
int nr_tiles_y(int H) { return (H + NR_TH - 1) / NR_TH; }      // tiles per image <= 2^20

}  // namespace

extern "C" size_t cfen_noref_bytes(int B, int H, int W, int radius) {
  if (!nr_dims_ok(B, H, W, radius)) return 0;
  return (size_t)B * (size_t)nr_tiles_x(W) * (size_t)nr_tiles_y(H) * sizeof(NrRecord);
}

extern "C" int cfen_noref_u8(const unsigned char* hazy, const unsigned char* out, int B, int H, int W, int radius, void* scratch,
                             unsigned long long* counts, double* grad, unsigned char* dark_hazy, unsigned char* dark_out, void* stream) {
  CFEN_CHECK_ARG(hazy && out && scratch && counts && grad, "noref_u8: null pointer (hazy, out, scratch, counts and grad are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= NR_MAX_BATCH, "noref_u8: B = %d outside 1 .. %d", B, NR_MAX_BATCH);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= NR_MAX_EDGE && W <= NR_MAX_EDGE, "noref_u8: sizes H = %d, W = %d outside 1 .. %d", H, W, NR_MAX_EDGE);
  CFEN_CHECK_ARG(radius >= 0 && radius <= NR_MAXR, "noref_u8: radius = %d outside 0 .. %d", radius, NR_MAXR);
  CFEN_CHECK_ARG(cfen_aligned(scratch, 8) && cfen_aligned(counts, 8) && cfen_aligned(grad, 8),
                 "noref_u8: scratch, counts and grad must be 8-byte aligned (64-bit words)");
  const int tiles_x = nr_tiles_x(W), ntiles = tiles_x * nr_tiles_y(H);
  hipStream_t s = (hipStream_t)stream;
  CFEN_LAUNCH(k_noref, dim3((unsigned)ntiles, (unsigned)B), dim3(256), 0, s, hazy, out, H, W, radius, tiles_x, dark_hazy, dark_out,
              (NrRecord*)scratch);
  CFEN_CHECK_LAUNCH("noref_u8");
  CFEN_LAUNCH(k_noref_finish, dim3((unsigned)B, 2u, 17u), dim3(256), 0, s, (const NrRecord*)scratch, ntiles, counts, grad);
  CFEN_CHECK_LAUNCH("noref_u8 (finish)");
  return CFEN_OK;
}
