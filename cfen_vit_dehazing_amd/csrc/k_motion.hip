// Motion compensation for the temporal stabilisation (include/cfen_motion.h states the definition and the contract; tests/motion_ref.py restates it).
//
//   k_motion_search : a workgroup of 256 threads takes one block of one frame.  The block (invalid pixels of an edge block as 0) and its
//                     (Bk + 2R)^2 window of the previous frame -- window entry i is the pixel at clamp(origin - R + i), so the definition's
//                     clamp is the staging's -- go to LDS as RGB0 dwords: one v_sad_u8 does one pixel with its accumulate, the fourth byte
//                     adds |0 - 0|.  The block's rows are cut into NS slices of RS rows; a thread owns one slice, holds its RS x Bk pixels in
//                     registers and walks the candidates lane, lane + L, ... with one dword LDS read per pixel and candidate.  The window's row
//                     stride is 2R + 33 dwords = (2R + 1) mod 32, so the 32 lanes of a read, candidates c .. c + 31 in (dy, dx) order, hit 32
//                     different banks.  An edge block (block-uniform) walks its valid pixels in a plain loop with both operands from LDS.
//                     The slices' partial sums (at most 2 x 32 x 765, a uint16) meet in LDS; then a thread per candidate forms
//                     cost and packs (cost, |dy| + |dx|, dy + 16, dx + 16) into one 64-bit key whose order is the definition's lexicographic one,
//                     and the minimum goes lane butterfly -> four waves in wave order.  All integer: the result is the same bits on every run.
//   k_motion_warp   : a thread takes two consecutive pixels: per pixel the block's vector, the clamped source pixel, three bytes and the six
//                     floats as one 16-byte and one 8-byte load (which comes first depends on the source pixel's parity); the pair's twelve
//                     floats leave as three 16-byte stores.
// One launch each; no atomics, no counters, no scratch.
#include "../../include/cfen_motion.h"
#include "cfen_image.hpp"

namespace {

constexpr int MS_RMAX = 16;
constexpr int MS_MAX_EDGE = 16384;

CFEN_DEV int ms_clamp(int v, int n) { return min(max(v, 0), n - 1); }

CFEN_DEV unsigned ms_rgb0(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

// the sum over a slice of |cur - window| where the whole Bk x Bk block lies inside the frame: the slice's pixels are in registers
template <int BK, int RS>
CFEN_DEV unsigned ms_slice_sad(const unsigned (&cur)[RS][BK], const unsigned* win, int wsp) {
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < RS; ++j) {
#pragma unroll
    for (int px = 0; px < BK; ++px) s = __builtin_amdgcn_sad_u8(cur[j][px], win[j * wsp + px], s);
  }
  return s;
}

// the same over the nrows x nbx valid pixels of a slice of an edge block, both operands from LDS
CFEN_DEV unsigned ms_slice_sad_edge(const unsigned* cur, int bk, const unsigned* win, int wsp, int nrows, int nbx) {
  unsigned s = 0;
  for (int j = 0; j < nrows; ++j)
    for (int px = 0; px < nbx; ++px) s = __builtin_amdgcn_sad_u8(cur[j * bk + px], win[j * wsp + px], s);
  return s;
}

constexpr int ms_slices(int bk) { return bk == 32 ? 16 : 8; }

// bytes of dynamic LDS: the four waves' minima, the block, the window, the partial sums
size_t ms_lds_bytes(int bk, int R) {
  const int n = 2 * R + 1;
  return 32 + (size_t)bk * bk * 4 + (size_t)(bk + 2 * R) * (2 * R + 33) * 4 + (size_t)ms_slices(bk) * n * n * 2;
}

template <int BK>
__global__ __launch_bounds__(256) void k_motion_search(const unsigned char* __restrict__ guide, const unsigned char* __restrict__ prev_guide,
                                                       short* __restrict__ vec, int* __restrict__ sad, int h, int w, int R, int bias, int bh, int bw) {
  constexpr int NS = ms_slices(BK), RS = BK / NS, L = 256 / NS;
  extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
  const int n = 2 * R + 1, NC = n * n, WSP = 2 * R + 33;
  unsigned long long* sRed = reinterpret_cast<unsigned long long*>(ms_lds);
  unsigned* sCur = reinterpret_cast<unsigned*>(ms_lds + 32);
  unsigned* sWin = sCur + BK * BK;
  unsigned short* sPart = reinterpret_cast<unsigned short*>(sWin + (BK + 2 * R) * WSP);
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % bw, by = (blockIdx.x / bw) % bh, k = blockIdx.x / (bw * bh);
  const int y0 = by * BK, x0 = bx * BK;
  const int nby = min(BK, h - y0), nbx = min(BK, w - x0);
  const long long frame = (long long)h * w * 3;
  const unsigned char* cur = guide + k * frame;
  const unsigned char* prv = k ? cur - frame : prev_guide;
  const int wc = nbx + 2 * R;                                                                // window columns and rows that a valid pixel can reach
  for (int i = tid; i < (nby + 2 * R) * wc; i += 256) {
    const int wy = i / wc, wx = i - wy * wc;
    sWin[wy * WSP + wx] = ms_rgb0(prv + ((long long)ms_clamp(y0 - R + wy, h) * w + ms_clamp(x0 - R + wx, w)) * 3);
  }
  for (int i = tid; i < BK * BK; i += 256) {
    const int py = i / BK, px = i % BK;
    sCur[i] = py < nby && px < nbx ? ms_rgb0(cur + ((long long)(y0 + py) * w + x0 + px) * 3) : 0u;
  }
  __syncthreads();
  const int s = tid / L, lane = tid % L, r0 = s * RS;
  const int nrows = min(max(nby - r0, 0), RS);
  unsigned c4[RS][BK];
#pragma unroll
  for (int j = 0; j < RS; ++j) {
#pragma unroll
    for (int q = 0; q < BK / 4; ++q) {
      const uint4 v = *reinterpret_cast<const uint4*>(sCur + (r0 + j) * BK + q * 4);
      c4[j][q * 4] = v.x, c4[j][q * 4 + 1] = v.y, c4[j][q * 4 + 2] = v.z, c4[j][q * 4 + 3] = v.w;
    }
  }
  const bool full = nby == BK && nbx == BK;
  for (int c = lane; c < NC; c += L) {
    const int cy = c / n, cx = c - cy * n;                                                   // dy + R, dx + R
    const unsigned* win = sWin + (r0 + cy) * WSP + cx;
    const unsigned p = full ? ms_slice_sad<BK, RS>(c4, win, WSP) : ms_slice_sad_edge(sCur + r0 * BK, BK, win, WSP, nrows, nbx);
    sPart[s * NC + c] = (unsigned short)p;
  }
  __syncthreads();
  const int nb3 = 3 * nby * nbx;
  unsigned long long best = ~0ull;
  for (int c = tid; c < NC; c += 256) {
    unsigned S = 0;
#pragma unroll
    for (int j = 0; j < NS; ++j) S += sPart[j * NC + c];
    const int cy = c / n, cx = c - cy * n;
    const unsigned l1 = (unsigned)(abs(cy - R) + abs(cx - R));
    const unsigned cost = 16u * S + (unsigned)bias * l1 * (unsigned)nb3;
    const unsigned long long key = ((unsigned long long)cost << 18) | (l1 << 12) | ((unsigned)(cy - R + 16) << 6) | (unsigned)(cx - R + 16);
    best = key < best ? key : best;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(best, m, 64);
    best = o < best ? o : best;
  }
  if ((tid & 63) == 0) sRed[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int j = 1; j < 4; ++j) best = sRed[j] < best ? sRed[j] : best;
    const int dx = (int)(best & 63) - 16, dy = (int)((best >> 6) & 63) - 16;
    const unsigned l1 = (unsigned)(best >> 12) & 63, cost = (unsigned)(best >> 18);
    const long long o = blockIdx.x;
    vec[o * 2] = (short)dy;
    vec[o * 2 + 1] = (short)dx;
    sad[o] = (int)((cost - (unsigned)bias * l1 * (unsigned)nb3) >> 4);
  }
}

__global__ __launch_bounds__(256) void k_motion_warp(const short* __restrict__ vec, const unsigned char* __restrict__ prev_guide,
                                                     const float* __restrict__ state, unsigned char* __restrict__ prev_out,
                                                     float* __restrict__ state_out, int h, int w, int shift, int bw) {
  const int npx = h * w;                                                                     // at most 2^28
  const int i = (blockIdx.x * 256 + threadIdx.x) * 2;
  if (i >= npx) return;
  const int np = min(2, npx - i);
  float f[2][6];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j >= np) break;
    const int p = i + j, y = p / w, x = p - y * w;
    const int b = (y >> shift) * bw + (x >> shift);
    const int q = ms_clamp(y + vec[2 * b], h) * w + ms_clamp(x + vec[2 * b + 1], w);
    const unsigned char* src = prev_guide + (long long)q * 3;
    unsigned char* dst = prev_out + (long long)p * 3;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
    const float* sp = state + (long long)q * 6;                                              // 24 q bytes in: 16-byte aligned where q is even
    if (q & 1) {
      const float2 a = *reinterpret_cast<const float2*>(sp);
      const float4 c = *reinterpret_cast<const float4*>(sp + 2);
      f[j][0] = a.x, f[j][1] = a.y, f[j][2] = c.x, f[j][3] = c.y, f[j][4] = c.z, f[j][5] = c.w;
    } else {
      const float4 a = *reinterpret_cast<const float4*>(sp);
      const float2 c = *reinterpret_cast<const float2*>(sp + 4);
      f[j][0] = a.x, f[j][1] = a.y, f[j][2] = a.z, f[j][3] = a.w, f[j][4] = c.x, f[j][5] = c.y;
    }
  }
  float* o = state_out + (long long)i * 6;                                                   // i is even: 16-byte aligned
  *reinterpret_cast<float4*>(o) = make_float4(f[0][0], f[0][1], f[0][2], f[0][3]);
  if (np == 2) {
    *reinterpret_cast<float4*>(o + 4) = make_float4(f[0][4], f[0][5], f[1][0], f[1][1]);
    *reinterpret_cast<float4*>(o + 8) = make_float4(f[1][2], f[1][3], f[1][4], f[1][5]);
  } else {
    *reinterpret_cast<float2*>(o + 4) = make_float2(f[0][4], f[0][5]);
  }
}

bool ms_block_ok(int block) { return block == 8 || block == 16 || block == 32; }

}  // namespace

extern "C" int cfen_motion_search_u8(const unsigned char* guide, const unsigned char* prev_guide, int B, int h, int w, int block, int range, int bias,
                                     short* vec, int* sad, void* stream) {
  CFEN_CHECK_ARG(guide && prev_guide && vec && sad, "motion_search_u8: null pointer (guide, prev_guide, vec and sad are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "motion_search_u8: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= MS_MAX_EDGE && w <= MS_MAX_EDGE, "motion_search_u8: sizes h = %d, w = %d outside 1 .. %d", h, w, MS_MAX_EDGE);
  CFEN_CHECK_ARG(ms_block_ok(block), "motion_search_u8: block = %d is none of 8, 16, 32", block);
  CFEN_CHECK_ARG(range >= 1 && range <= MS_RMAX, "motion_search_u8: range = %d outside 1 .. %d", range, MS_RMAX);
  CFEN_CHECK_ARG(bias >= 0 && bias <= 255, "motion_search_u8: bias = %d outside 0 .. 255", bias);
  CFEN_CHECK_ARG(cfen_aligned(vec, 4) && cfen_aligned(sad, 4), "motion_search_u8: vec and sad must be 4-byte aligned");
  const int bh = (h + block - 1) / block, bw = (w + block - 1) / block;
  const long long px = (long long)h * w, blocks = (long long)B * bh * bw;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "motion_search_u8: B = %d frames of %d x %d are too large for one launch", B, h, w);
  const void* const ptrs[4] = {guide, prev_guide, vec, sad};
  const long long bytes[4] = {B * px * 3, px * 3, blocks * 4, blocks * 4};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 4), "motion_search_u8: guide, prev_guide, vec and sad must not overlap");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = ms_lds_bytes(block, range);                                             // at most 55616 bytes
  if (block == 8)
    CFEN_LAUNCH(k_motion_search<8>, dim3((unsigned)blocks), dim3(256), lds, s, guide, prev_guide, vec, sad, h, w, range, bias, bh, bw);
  else if (block == 16)
    CFEN_LAUNCH(k_motion_search<16>, dim3((unsigned)blocks), dim3(256), lds, s, guide, prev_guide, vec, sad, h, w, range, bias, bh, bw);
  else
    CFEN_LAUNCH(k_motion_search<32>, dim3((unsigned)blocks), dim3(256), lds, s, guide, prev_guide, vec, sad, h, w, range, bias, bh, bw);
  CFEN_CHECK_LAUNCH("motion_search_u8");
  return CFEN_OK;
}

extern "C" int cfen_motion_warp(const short* vec, const unsigned char* prev_guide, const float* state, int h, int w, int block,
                                unsigned char* prev_out, float* state_out, void* stream) {
  CFEN_CHECK_ARG(vec && prev_guide && state && prev_out && state_out,
                 "motion_warp: null pointer (vec, prev_guide, state, prev_out and state_out are all required)");
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= MS_MAX_EDGE && w <= MS_MAX_EDGE, "motion_warp: sizes h = %d, w = %d outside 1 .. %d", h, w, MS_MAX_EDGE);
  CFEN_CHECK_ARG(ms_block_ok(block), "motion_warp: block = %d is none of 8, 16, 32", block);
  CFEN_CHECK_ARG(cfen_aligned(vec, 4), "motion_warp: vec must be 4-byte aligned");
  CFEN_CHECK_ARG(cfen_aligned16(state) && cfen_aligned16(state_out), "motion_warp: state and state_out must be 16-byte aligned");
  const int bh = (h + block - 1) / block, bw = (w + block - 1) / block;
  const long long px = (long long)h * w;
  const void* const ptrs[5] = {vec, prev_guide, state, prev_out, state_out};
  const long long bytes[5] = {(long long)bh * bw * 4, px * 3, px * 24, px * 3, px * 24};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 5), "motion_warp: vec, prev_guide, state, prev_out and state_out must not overlap");
  const int shift = block == 8 ? 3 : block == 16 ? 4 : 5;
  CFEN_LAUNCH(k_motion_warp, dim3((unsigned)((px + 511) / 512)), dim3(256), 0, (hipStream_t)stream, vec, prev_guide, state, prev_out, state_out, h, w,
              shift, bw);
  CFEN_CHECK_LAUNCH("motion_warp");
  return CFEN_OK;
}
