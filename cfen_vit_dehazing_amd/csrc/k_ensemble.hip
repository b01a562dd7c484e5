// Geometric self-ensemble (x8) on the device (ensemble.py): the network's output is the mean over the eight flips / transposes of its input
// (the reference's Model.forward_x8, models/vit_model.py:102-147, inherited from IPT; its dehazing model never calls it).
//
// Variant i = b0 + 2 b1 + 4 b2 of a T x T plane x, with v = flip W, h = flip H, t = swap H and W (v first):
//   x_i = t^b2(h^b1(v^b0(x)))          x_i[r][c] = x[fr(r)][fc(c)]  (b2 = 0),   x[fr(c)][fc(r)]  (b2 = 1)
//   fr(k) = b1 ? T - 1 - k : k,  fc(k) = b0 ? T - 1 - k : k
// and every output plane y_i of the forward of x_i is mapped back as v^b0(h^b1(t^b2(y_i))):
//   out[r][c] = 0.125f * (((((((z_0 + z_1) + z_2) + z_3) + z_4) + z_5) + z_6) + z_7),   z_i[r][c] = y_i[fr(r)][fc(c)]  (b2 = 0),  y_i[fc(c)][fr(r)]  (b2 = 1)
// fp32 adds in increasing i and one exact scaling: nothing else happens to the values, so the result is bitwise reproducible and bitwise the
// same sum written with any other fp32 adds in that order.
//
//   k_x8_expand : image m of the input -> the network's batch-8 input slab in variant order.  A pure copy.
//   k_x8_merge  : M forward output slabs back to back (slab m = [xr (8,3,T,T) | xs (8,1,T,T) | xd (8,3,T,T)], fp32 or fp16) -> the merged outputs.
//
// Memory access: every global read and write is a whole 16-byte vector along the contiguous axis of its tensor.  The flips are index arithmetic (a
// flipped vector is read whole and its elements reversed in registers); the four transposed variants pass through an LDS tile of dwords with rows
// padded to 33 / 65: with ds_read_b32 / ds_write_b32 (bank = dword address mod 32, conflicts per 32-lane half) a row walk has lanes at
// (row, 4 q + k) -> bank row + 4 q + k, a column walk lanes at (4 q + k, col) -> bank 4 q + k + col (33 = 1 mod 32): both cover 32 distinct banks
// for 4 rows x 8 quads.  Where a lane carries 8 (fp16 arena) or 16 (uint8 pixels) elements the column walk is 2-way (8 q or 16 q mod 32); these
// kernels are bound by their global traffic, not by LDS.  No atomics, no counters.
#include "cfen_common.hpp"

namespace {

constexpr int XT = 32;        // tile rows; the tile is XT x (8 E) elements, E = elements per 16-byte vector of the transposed side

// ---- expand --------------------------------------------------------------------------------------------------------------------------------------
// fp32 (3,T,T) plane c -> planes (i, c) of (8,3,T,T).  One 32 x 32 source tile per block, one float4 per thread and variant.
__global__ __launch_bounds__(256) void k_x8_expand_f32(const float* __restrict__ src, float* __restrict__ dst, int T) {
  __shared__ float buf[XT][XT + 1];
  const int t = threadIdx.x, row = t >> 3, q = t & 7;
  const int R = blockIdx.y * XT + row, C = blockIdx.x * XT + 4 * q, c = blockIdx.z;
  const long long TT = (long long)T * T;
  const bool ok = R < T && C < T;                       // T % 16 == 0: a quad is inside or outside as a whole
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) v = *reinterpret_cast<const float4*>(src + c * TT + (long long)R * T + C);
  buf[row][4 * q] = v.x;
  buf[row][4 * q + 1] = v.y;
  buf[row][4 * q + 2] = v.z;
  buf[row][4 * q + 3] = v.w;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {                         // plain and flipped: from registers
    if (!ok) break;
    const int b0 = i & 1, b1 = i >> 1;
    const int r = b1 ? T - 1 - R : R, c0 = b0 ? T - 4 - C : C;
    *reinterpret_cast<float4*>(dst + (i * 3 + c) * TT + (long long)r * T + c0) = b0 ? make_float4(v.w, v.z, v.y, v.x) : v;
  }
  // transposed: destination (r', c') = (fc(source column), fr(source row)); this thread writes destination row `row` of the tile, quad q
  const int sC = blockIdx.x * XT + row, sR = blockIdx.y * XT + 4 * q;      // source column of the destination row, first source row of the quad
  if (sC < T && sR < T) {
#pragma unroll
    for (int i = 4; i < 8; ++i) {
      const int b0 = i & 1, b1 = (i >> 1) & 1;
      const float e0 = buf[4 * q][row], e1 = buf[4 * q + 1][row], e2 = buf[4 * q + 2][row], e3 = buf[4 * q + 3][row];
      const int r = b0 ? T - 1 - sC : sC, c0 = b1 ? T - 4 - sR : sR;
      *reinterpret_cast<float4*>(dst + (i * 3 + c) * TT + (long long)r * T + c0) = b1 ? make_float4(e3, e2, e1, e0) : make_float4(e0, e1, e2, e3);
    }
  }
}

// 16 pixels of 3 bytes <-> three 16-byte vectors; a pixel travels as one dword (r | g << 8 | b << 16)
struct Px16 {
  unsigned p[16];
};

CFEN_DEV void px_unpack(const uint4* g, Px16& o) {
  const uint4 a = g[0], b = g[1], c = g[2];
  const unsigned d[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    o.p[4 * k] = d[3 * k] & 0xffffffu;
    o.p[4 * k + 1] = (d[3 * k] >> 24) | ((d[3 * k + 1] & 0xffffu) << 8);
    o.p[4 * k + 2] = (d[3 * k + 1] >> 16) | ((d[3 * k + 2] & 0xffu) << 16);
    o.p[4 * k + 3] = d[3 * k + 2] >> 8;
  }
}

// rev: pixel order reversed
CFEN_DEV void px_pack(const Px16& s, bool rev, uint4* g) {
  unsigned p[16], d[12];
#pragma unroll
  for (int e = 0; e < 16; ++e) p[e] = rev ? s.p[15 - e] : s.p[e];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    d[3 * k] = p[4 * k] | (p[4 * k + 1] << 24);
    d[3 * k + 1] = (p[4 * k + 1] >> 8) | (p[4 * k + 2] << 16);
    d[3 * k + 2] = (p[4 * k + 2] >> 16) | (p[4 * k + 3] << 8);
  }
  g[0] = make_uint4(d[0], d[1], d[2], d[3]);
  g[1] = make_uint4(d[4], d[5], d[6], d[7]);
  g[2] = make_uint4(d[8], d[9], d[10], d[11]);
}

// uint8 (T,T,3) -> (8,T,T,3).  One 64 x 64 pixel source tile per block, 16 pixels = 48 bytes = three 16-byte vectors per thread and variant.
__global__ __launch_bounds__(256) void k_x8_expand_u8(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int T) {
  __shared__ unsigned buf[64][65];
  const int t = threadIdx.x, row = t >> 2, q = t & 3;
  const int R = blockIdx.y * 64 + row, C = blockIdx.x * 64 + 16 * q;
  const long long img = (long long)T * T * 3;
  const bool ok = R < T && C < T;
  Px16 v = {};
  if (ok) px_unpack(reinterpret_cast<const uint4*>(src + ((long long)R * T + C) * 3), v);
#pragma unroll
  for (int e = 0; e < 16; ++e) buf[row][16 * q + e] = v.p[e];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!ok) break;
    const int b0 = i & 1, b1 = i >> 1;
    const int r = b1 ? T - 1 - R : R, c0 = b0 ? T - 16 - C : C;
    px_pack(v, b0, reinterpret_cast<uint4*>(dst + i * img + ((long long)r * T + c0) * 3));
  }
  const int sC = blockIdx.x * 64 + row, sR = blockIdx.y * 64 + 16 * q;
  if (sC < T && sR < T) {
    Px16 w;
#pragma unroll
    for (int e = 0; e < 16; ++e) w.p[e] = buf[16 * q + e][row];
#pragma unroll
    for (int i = 4; i < 8; ++i) {
      const int b0 = i & 1, b1 = (i >> 1) & 1;
      const int r = b0 ? T - 1 - sC : sC, c0 = b1 ? T - 16 - sR : sR;
      px_pack(w, b1, reinterpret_cast<uint4*>(dst + i * img + ((long long)r * T + c0) * 3));
    }
  }
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------------------------
CFEN_DEV unsigned char to_u8(float v) { return (unsigned char)(int)((v + 1.f) / 2.0f * 255.0f); }   // k_tile_blend_u8 (k_tile.hip), k_tensor2im_u8

// plane p (0..6 = xr0 xr1 xr2 xs xd0 xd1 xd2) of variant i inside one slab [xr (8,3) | xs (8,1) | xd (8,3)], in planes of T T elements
CFEN_DEV int slab_plane(int i, int p) { return p < 3 ? i * 3 + p : (p == 3 ? 24 + i : 32 + i * 3 + (p - 4)); }

// One XT x (8 E) output tile per block, E = 16 / sizeof(TA) consecutive output pixels of a row per thread: the plain / flipped variants are one
// 16-byte read each, the transposed ones are staged (one 16-byte read per thread and variant) in LDS as fp32 and read back along columns.
//   U8 = false: blockIdx.z = m * 7 + p, one fp32 plane, E / 4 float4 stores per thread.
//   U8 = true : blockIdx.z = m * 3 + g, image g (xr, xs, xd) as (T,T,3) bytes from its 3 / 1 / 3 planes; the thread's E pixels (3 E bytes) go
//               through an LDS row image so that the stores are whole 16-byte vectors too.
template <typename TA, bool U8>
__global__ __launch_bounds__(256) void k_x8_merge(const TA* __restrict__ arena, int T, void* __restrict__ o_xr, void* __restrict__ o_xs,
                                                  void* __restrict__ o_xd) {
  constexpr int E = 16 / (int)sizeof(TA), TC = 8 * E, CPR = XT / E;      // CPR: 16-byte chunks per staged row (XT elements)
  __shared__ float buf[4][TC][XT + 1];
  __shared__ unsigned stage[U8 ? XT * (TC * 3 / 4) : 1];
  const int t = threadIdx.x;
  const long long TT = (long long)T * T;
  const int ngroups = U8 ? 3 : 7;
  const int m = blockIdx.z / ngroups, g = blockIdx.z % ngroups;
  const TA* slab = arena + (long long)m * 56 * TT;
  const int R0 = blockIdx.y * XT, C0 = blockIdx.x * TC;
  // output role: row orow of the tile, columns oc0 .. oc0 + E - 1
  const int orow = t >> 3, oc0 = (t & 7) * E;
  const int R = R0 + orow, C = C0 + oc0;
  const bool ok = R < T && C < T;
  // staging role: source row srow of the transposed tile (= output column, up to the flip), chunk ch of its XT columns (= output rows)
  const int srow = t / CPR, ch = t % CPR;
  const int p_lo = U8 ? (g == 0 ? 0 : (g == 1 ? 3 : 4)) : g, np = U8 ? (g == 1 ? 1 : 3) : 1;
  float res[3][E];
#pragma unroll
  for (int pi = 0; pi < 3; ++pi) {
    if (pi >= np) break;
    const int p = p_lo + pi;
    if (pi) __syncthreads();                 // the previous plane's column reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b0 = j & 1, b1 = j >> 1;
      const int oc = b0 ? TC - 1 - srow : srow;              // output column (tile-local) this source row maps to
      const int orl = b1 ? XT - E - ch * E : ch * E;         // lowest output row (tile-local) of the chunk
      float f[E];
#pragma unroll
      for (int k = 0; k < E; ++k) f[k] = 0.f;
      if (C0 + oc < T && R0 + orl < T) {
        const int sr = b0 ? T - 1 - (C0 + oc) : C0 + oc;                   // fc(output column)
        const int sc = b1 ? T - E - (R0 + orl) : R0 + orl;                 // fr of the chunk's highest output row = its lowest source column
        Vec16<TA>::load(slab + slab_plane(4 + j, p) * TT + (long long)sr * T + sc, f);
      }
#pragma unroll
      for (int k = 0; k < E; ++k) buf[j][srow][ch * E + k] = f[k];
    }
    __syncthreads();
    float acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = 0.f;
    if (ok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b0 = i & 1, b1 = i >> 1;
        const int r = b1 ? T - 1 - R : R, c0 = b0 ? T - E - C : C;
        float f[E];
        Vec16<TA>::load(slab + slab_plane(i, p) * TT + (long long)r * T + c0, f);
#pragma unroll
        for (int k = 0; k < E; ++k) {
          const float z = b0 ? f[E - 1 - k] : f[k];
          acc[k] = i == 0 ? z : acc[k] + z;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b0 = j & 1, b1 = j >> 1;
        const int lc = b1 ? XT - 1 - orow : orow;
#pragma unroll
        for (int k = 0; k < E; ++k) acc[k] += buf[j][b0 ? TC - 1 - (oc0 + k) : oc0 + k][lc];
      }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) res[pi][k] = acc[k] * 0.125f;
  }
  if constexpr (!U8) {
    if (ok) {
      float* out = (g < 3 ? (float*)o_xr + (m * 3 + g) * TT : (g == 3 ? (float*)o_xs + m * TT : (float*)o_xd + (m * 3 + g - 4) * TT)) + (long long)R * T + C;
#pragma unroll
      for (int k = 0; k < E; k += 4) *reinterpret_cast<float4*>(out + k) = make_float4(res[0][k], res[0][k + 1], res[0][k + 2], res[0][k + 3]);
    }
  } else {
    // E pixels x 3 bytes = 3 E / 4 dwords per thread into the row image [XT][TC * 3 / 4] dwords, then 16 bytes per thread out
    constexpr int RD = TC * 3 / 4;           // dwords per tile row
    unsigned px[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const unsigned a = to_u8(res[0][k]);
      px[k] = np == 1 ? a * 0x010101u : (a | ((unsigned)to_u8(res[1][k]) << 8) | ((unsigned)to_u8(res[2][k]) << 16));
    }
#pragma unroll
    for (int k = 0; k < E / 4; ++k) {
      unsigned* d = stage + orow * RD + (oc0 / 4 + k) * 3;
      d[0] = px[4 * k] | (px[4 * k + 1] << 24);
      d[1] = (px[4 * k + 1] >> 8) | (px[4 * k + 2] << 16);
      d[2] = (px[4 * k + 2] >> 16) | (px[4 * k + 3] << 8);
    }
    __syncthreads();
    unsigned char* out = (unsigned char*)(g == 0 ? o_xr : (g == 1 ? o_xs : o_xd)) + (long long)m * TT * 3;
    constexpr int VR = RD / 4;               // 16-byte vectors per tile row
    for (int q = t; q < XT * VR; q += 256) {
      const int r = q / VR, v = q % VR;
      if (R0 + r < T && C0 + v * 16 / 3 < T) {           // vector v starts at pixel 16 v / 3 of the row; T % 16 == 0 keeps a row's valid part whole vectors
        const unsigned* s = stage + r * RD + 4 * v;
        *reinterpret_cast<uint4*>(out + ((long long)(R0 + r) * T + C0) * 3 + 16 * v) = make_uint4(s[0], s[1], s[2], s[3]);
      }
    }
  }
}

}  // namespace

#define CFEN_X8_MAX_IMAGES 4096

int cfen_x8_expand_impl(int u8, const void* src, void* dst, int M, int m, int T, hipStream_t s) {
  CFEN_CHECK_ARG(src && dst, "x8_expand: null pointer");
  CFEN_CHECK_ARG(u8 == 0 || u8 == 1, "x8_expand: u8 must be 0 or 1");
  CFEN_CHECK_ARG(T >= 16 && T % 16 == 0 && T <= 8192, "x8_expand: image edge T = %d must be a multiple of 16 in 16 .. 8192", T);
  CFEN_CHECK_ARG(M >= 1 && M <= CFEN_X8_MAX_IMAGES && m >= 0 && m < M, "x8_expand: image %d outside the %d images of the input (1 .. %d)", m, M,
                 CFEN_X8_MAX_IMAGES);
  CFEN_CHECK_ARG(cfen_aligned16(src) && cfen_aligned16(dst), "x8_expand: src and dst must be 16-byte aligned");
  const long long TT = (long long)T * T;
  if (u8) {
    CFEN_LAUNCH(k_x8_expand_u8, dim3((T + 63) / 64, (T + 63) / 64), dim3(256), 0, s, (const unsigned char*)src + m * 3 * TT, (unsigned char*)dst, T);
  } else {
    CFEN_LAUNCH(k_x8_expand_f32, dim3((T + XT - 1) / XT, (T + XT - 1) / XT, 3), dim3(256), 0, s, (const float*)src + m * 3 * TT, (float*)dst, T);
  }
  CFEN_CHECK_LAUNCH("x8_expand");
  return CFEN_OK;
}

int cfen_x8_merge_impl(int dtype, const void* arena, int M, int T, int out_u8, void* xr, void* xs, void* xd, hipStream_t s) {
  CFEN_CHECK_ARG(arena && xr && xs && xd, "x8_merge: null pointer");
  CFEN_CHECK_ARG(dtype == 0 || dtype == 1, "x8_merge: unknown arena dtype %d", dtype);
  CFEN_CHECK_ARG(out_u8 == 0 || out_u8 == 1, "x8_merge: out_u8 must be 0 or 1");
  CFEN_CHECK_ARG(T >= 16 && T % 16 == 0 && T <= 8192, "x8_merge: image edge T = %d must be a multiple of 16 in 16 .. 8192", T);
  CFEN_CHECK_ARG(M >= 1 && M <= CFEN_X8_MAX_IMAGES, "x8_merge: %d images outside 1 .. %d", M, CFEN_X8_MAX_IMAGES);
  CFEN_CHECK_ARG(cfen_aligned16(arena) && cfen_aligned16(xr) && cfen_aligned16(xs) && cfen_aligned16(xd),
                 "x8_merge: the arena and the outputs must be 16-byte aligned");
  const int tc = dtype == 1 ? 64 : 32;
  const dim3 grid((T + tc - 1) / tc, (T + XT - 1) / XT, M * (out_u8 ? 3 : 7));
  if (out_u8) {
    if (dtype == 1)
      CFEN_LAUNCH((k_x8_merge<half_t, true>), grid, dim3(256), 0, s, (const half_t*)arena, T, xr, xs, xd);
    else
      CFEN_LAUNCH((k_x8_merge<float, true>), grid, dim3(256), 0, s, (const float*)arena, T, xr, xs, xd);
  } else {
    if (dtype == 1)
      CFEN_LAUNCH((k_x8_merge<half_t, false>), grid, dim3(256), 0, s, (const half_t*)arena, T, xr, xs, xd);
    else
      CFEN_LAUNCH((k_x8_merge<float, false>), grid, dim3(256), 0, s, (const float*)arena, T, xr, xs, xd);
  }
  CFEN_CHECK_LAUNCH("x8_merge");
  return CFEN_OK;
}
