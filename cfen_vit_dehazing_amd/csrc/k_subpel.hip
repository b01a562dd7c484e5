// Sub-pixel motion compensation (include/cfen_subpel.h states the definition and the contract; tests/subpel_ref.py restates it).
//
//   k_subpel_refine : a workgroup of 256 threads takes one block of one frame.  The block (invalid pixels of an edge block as 0) and the (Bk + 2)^2
//                     window of the previous frame around origin + v0 - 1 -- window entry i is the pixel at clamp(origin + v0 - 1 + i), so both
//                     tap clamps of the definition are the staging's -- go to LDS as RGB0 dwords, as in k_motion_search.  Every tap of every
//                     candidate of a pixel lies in the pixel's 3 x 3 neighbourhood of the window, so a thread OWNS PIXELS (tid, tid + 256, ...)
//                     and walks all (2Q - 1)^2 candidates over nine dwords it reads from LDS once: nine LDS reads per pixel against some 700
//                     VALU operations at Q = 4, where a thread per candidate (k_motion_search's split) would read four taps per pixel and candidate.
//                     The bilinear sample runs on two channels at once: R and B sit in the 16-bit halves of p & 0x00ff00ff, G in (p >> 8) & 255;
//                     a weighted sum of four taps is at most 16 * 255 + 8, so the halves never carry into each other.  It is separable and
//                     exact in integers: the horizontal sums (4 - fx) p_0 + fx p_1 of the three rows are formed once per ex and shared by
//                     the 2Q - 1 values of ey; the vertical sum, + 8, >> 4 and one v_sad_u8 against the block's pixel finish a candidate.
//                     The loops over candidates are unrolled, so the (2Q - 1)^2 sums of a thread stay in registers.  The window's row stride
//                     is chosen so that the 32 lanes of one half of a ds_read_b32 hit 32 banks: 34 at Bk = 32 (one row per half), 48 at
//                     Bk = 16 (two rows, 16 banks apart), 24 at Bk = 8 (four rows, 24 = -8 mod 32 apart).  The threads' sums (at most
//                     4 x 765, a uint16) meet in LDS as [candidate][thread]; four threads per candidate add 64 of them each from eight
//                     16-byte reads and meet by two lane exchanges; then cost4 and the packed 64-bit key (cost4, |v4|_1 - |4 v0|_1 + 6, ey, ex),
//                     whose order is the definition's lexicographic one, and the minimum goes lane butterfly -> four waves in wave order.
//                     All integer: the result is the same bits on every run.
//   k_subpel_warp   : shaped like k_motion_warp: a thread takes two consecutive pixels; per pixel the block's vec4, the four clamped taps, three
//                     integer-bilinear bytes and the six floats of each tap as one 16-byte and one 8-byte load, lerped in the header's order;
//                     the pair's twelve floats leave as three 16-byte stores.
// One launch each; no atomics, no counters, no scratch.
#include "../../include/cfen_subpel.h"
#include "cfen_image.hpp"

namespace {

constexpr int SP_MAX_EDGE = 16384;
constexpr int SP_VMAX = 2048;

CFEN_DEV int sp_clamp(int v, int n) { return min(max(v, 0), n - 1); }

CFEN_DEV unsigned sp_rgb0(const unsigned char* p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16); }

constexpr int sp_win_stride(int bk) { return bk == 32 ? 34 : bk == 16 ? 48 : 24; }

template <int BK, int Q>
__global__ __launch_bounds__(256) void k_subpel_refine(const unsigned char* __restrict__ guide, const unsigned char* __restrict__ prev_guide,
                                                       const short* __restrict__ vec, short* __restrict__ vec4, int* __restrict__ sad4, int h, int w,
                                                       int bias, int bh, int bw) {
  constexpr int N = 2 * Q - 1, NC = N * N, STEP = 4 / Q, WS = sp_win_stride(BK), PPT = BK * BK > 256 ? BK * BK / 256 : 1;
  __shared__ unsigned long long sRed[4];
  __shared__ unsigned sCur[BK * BK];
  __shared__ unsigned sWin[(BK + 2) * WS];
  __shared__ __attribute__((aligned(16))) unsigned short sPart[NC * 256];
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % bw, by = (blockIdx.x / bw) % bh, k = blockIdx.x / (bw * bh);
  const int y0 = by * BK, x0 = bx * BK;
  const int nby = min(BK, h - y0), nbx = min(BK, w - x0);
  const long long frame = (long long)h * w * 3;
  const unsigned char* cur = guide + k * frame;
  const unsigned char* prv = k ? cur - frame : prev_guide;
  const long long o = blockIdx.x;
  const int dy0 = min(max((int)vec[o * 2], -SP_VMAX), SP_VMAX), dx0 = min(max((int)vec[o * 2 + 1], -SP_VMAX), SP_VMAX);
  const int wc = nbx + 2;                                                                    // window columns and rows that a valid pixel can reach
  for (int i = tid; i < (nby + 2) * wc; i += 256) {
    const int wy = i / wc, wx = i - wy * wc;
    sWin[wy * WS + wx] = sp_rgb0(prv + ((long long)sp_clamp(y0 + dy0 - 1 + wy, h) * w + sp_clamp(x0 + dx0 - 1 + wx, w)) * 3);
  }
  for (int i = tid; i < BK * BK; i += 256) {
    const int py = i / BK, px = i % BK;
    sCur[i] = py < nby && px < nbx ? sp_rgb0(cur + ((long long)(y0 + py) * w + x0 + px) * 3) : 0u;
  }
  __syncthreads();
  unsigned acc[N][N];
#pragma unroll
  for (int a = 0; a < N; ++a) {
#pragma unroll
    for (int b = 0; b < N; ++b) acc[a][b] = 0u;
  }
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = tid + j * 256;
    const int py = i / BK, px = i % BK;
    if (i < BK * BK && py < nby && px < nbx) {
      const unsigned c = sCur[i];
      unsigned rb[3][3], g[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const unsigned p = sWin[(py + a) * WS + px + b];
          rb[a][b] = p & 0x00ff00ffu;
          g[a][b] = (p >> 8) & 0xffu;
        }
      }
#pragma unroll
      for (int xi = 0; xi < N; ++xi) {
        const int ex = (xi - (Q - 1)) * STEP;                                                // compile-time after unrolling
        const int b0 = ex < 0 ? 0 : 1;
        const unsigned fx = (unsigned)(ex & 3);
        unsigned hrb[3], hg[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          hrb[a] = (4u - fx) * rb[a][b0] + fx * rb[a][b0 + 1];                               // at most 4 * 255 per half
          hg[a] = (4u - fx) * g[a][b0] + fx * g[a][b0 + 1];
        }
#pragma unroll
        for (int yi = 0; yi < N; ++yi) {
          const int ey = (yi - (Q - 1)) * STEP;
          const int a0 = ey < 0 ? 0 : 1;
          const unsigned fy = (unsigned)(ey & 3);
          const unsigned vrb = (((4u - fy) * hrb[a0] + fy * hrb[a0 + 1] + 0x00080008u) >> 4) & 0x00ff00ffu;
          const unsigned vg = ((4u - fy) * hg[a0] + fy * hg[a0 + 1] + 8u) >> 4;
          acc[yi][xi] = __builtin_amdgcn_sad_u8(c, vrb | (vg << 8), acc[yi][xi]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < N; ++a) {
#pragma unroll
    for (int b = 0; b < N; ++b) sPart[(a * N + b) * 256 + tid] = (unsigned short)acc[a][b];
  }
  __syncthreads();
  const int nb3 = 3 * nby * nbx;
  unsigned long long best = ~0ull;
  unsigned S = 0;
  const int c = tid >> 2, q = tid & 3;
  if (c < NC) {
    const uint4* part = reinterpret_cast<const uint4*>(sPart + c * 256 + q * 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint4 v = part[j];
      S += (v.x & 0xffffu) + (v.x >> 16) + (v.y & 0xffffu) + (v.y >> 16) + (v.z & 0xffffu) + (v.z >> 16) + (v.w & 0xffffu) + (v.w >> 16);
    }
  }
  S += __shfl_xor(S, 1, 64);
  S += __shfl_xor(S, 2, 64);
  const int base4y = 4 * dy0, base4x = 4 * dx0;
  const int l1base = abs(base4y) + abs(base4x);
  if (c < NC) {
    const int yi = c / N, xi = c - yi * N;
    const int ey = (yi - (Q - 1)) * STEP, ex = (xi - (Q - 1)) * STEP;
    const int l1 = abs(base4y + ey) + abs(base4x + ex);
    const unsigned long long cost = 64ull * S + (unsigned long long)bias * (unsigned)l1 * (unsigned)nb3;      // below 2^34 for any int16 vector
    best = (cost << 10) | ((unsigned)(l1 - l1base + 6) << 6) | ((unsigned)(ey + 3) << 3) | (unsigned)(ex + 3);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long v = __shfl_xor(best, m, 64);
    best = v < best ? v : best;
  }
  if ((tid & 63) == 0) sRed[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int j = 1; j < 4; ++j) best = sRed[j] < best ? sRed[j] : best;
    const int ex = (int)(best & 7) - 3, ey = (int)((best >> 3) & 7) - 3;
    const int l1 = (int)((best >> 6) & 15) - 6 + l1base;
    const unsigned long long cost = best >> 10;
    vec4[o * 2] = (short)(base4y + ey);
    vec4[o * 2 + 1] = (short)(base4x + ex);
    sad4[o] = (int)((cost - (unsigned long long)bias * (unsigned)l1 * (unsigned)nb3) >> 6);
  }
}

// the six floats of pixel q of a (h, w, 6) fp32 field: 24 q bytes in, 16-byte aligned where q is even
CFEN_DEV void sp_load6(const float* __restrict__ state, int q, float (&f)[6]) {
  const float* sp = state + (long long)q * 6;
  if (q & 1) {
    const float2 a = *reinterpret_cast<const float2*>(sp);
    const float4 c = *reinterpret_cast<const float4*>(sp + 2);
    f[0] = a.x, f[1] = a.y, f[2] = c.x, f[3] = c.y, f[4] = c.z, f[5] = c.w;
  } else {
    const float4 a = *reinterpret_cast<const float4*>(sp);
    const float2 c = *reinterpret_cast<const float2*>(sp + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = c.x, f[5] = c.y;
  }
}

__global__ __launch_bounds__(256) void k_subpel_warp(const short* __restrict__ vec4, const unsigned char* __restrict__ prev_guide,
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
    const int y4 = 4 * y + vec4[2 * b], x4 = 4 * x + vec4[2 * b + 1];
    const int ya = sp_clamp(y4 >> 2, h), yb = sp_clamp((y4 >> 2) + 1, h), xa = sp_clamp(x4 >> 2, w), xb = sp_clamp((x4 >> 2) + 1, w);
    const int fy = y4 & 3, fx = x4 & 3;
    const int q00 = ya * w + xa, q01 = ya * w + xb, q10 = yb * w + xa, q11 = yb * w + xb;
    const unsigned char* s00 = prev_guide + (long long)q00 * 3;
    const unsigned char* s01 = prev_guide + (long long)q01 * 3;
    const unsigned char* s10 = prev_guide + (long long)q10 * 3;
    const unsigned char* s11 = prev_guide + (long long)q11 * 3;
    unsigned char* dst = prev_out + (long long)p * 3;
    const int w00 = (4 - fy) * (4 - fx), w01 = (4 - fy) * fx, w10 = fy * (4 - fx), w11 = fy * fx;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dst[ch] = (unsigned char)((w00 * s00[ch] + w01 * s01[ch] + w10 * s10[ch] + w11 * s11[ch] + 8) >> 4);
    float a00[6], a01[6], a10[6], a11[6];
    sp_load6(state, q00, a00);
    sp_load6(state, q01, a01);
    sp_load6(state, q10, a10);
    sp_load6(state, q11, a11);
    const float gx = (float)fx * 0.25f, gy = (float)fy * 0.25f;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const float t0 = a00[e] + gx * (a01[e] - a00[e]);
      const float t1 = a10[e] + gx * (a11[e] - a10[e]);
      f[j][e] = t0 + gy * (t1 - t0);
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

bool sp_block_ok(int block) { return block == 8 || block == 16 || block == 32; }

template <int BK>
void sp_launch_refine(int subpel, unsigned blocks, hipStream_t s, const unsigned char* guide, const unsigned char* prev_guide, const short* vec,
                      short* vec4, int* sad4, int h, int w, int bias, int bh, int bw) {
  if (subpel == 2)
    CFEN_LAUNCH((k_subpel_refine<BK, 2>), dim3(blocks), dim3(256), 0, s, guide, prev_guide, vec, vec4, sad4, h, w, bias, bh, bw);
  else
    CFEN_LAUNCH((k_subpel_refine<BK, 4>), dim3(blocks), dim3(256), 0, s, guide, prev_guide, vec, vec4, sad4, h, w, bias, bh, bw);
}

}  // namespace

extern "C" int cfen_motion_refine_u8(const unsigned char* guide, const unsigned char* prev_guide, const short* vec, int B, int h, int w, int block,
                                     int subpel, int bias, short* vec4, int* sad4, void* stream) {
  CFEN_CHECK_ARG(guide && prev_guide && vec && vec4 && sad4,
                 "motion_refine_u8: null pointer (guide, prev_guide, vec, vec4 and sad4 are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "motion_refine_u8: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= SP_MAX_EDGE && w <= SP_MAX_EDGE, "motion_refine_u8: sizes h = %d, w = %d outside 1 .. %d", h, w, SP_MAX_EDGE);
  CFEN_CHECK_ARG(sp_block_ok(block), "motion_refine_u8: block = %d is none of 8, 16, 32", block);
  CFEN_CHECK_ARG(subpel == 2 || subpel == 4, "motion_refine_u8: subpel = %d is neither 2 nor 4", subpel);
  CFEN_CHECK_ARG(bias >= 0 && bias <= 255, "motion_refine_u8: bias = %d outside 0 .. 255", bias);
  CFEN_CHECK_ARG(cfen_aligned(vec, 4) && cfen_aligned(vec4, 4) && cfen_aligned(sad4, 4), "motion_refine_u8: vec, vec4 and sad4 must be 4-byte aligned");
  const int bh = (h + block - 1) / block, bw = (w + block - 1) / block;
  const long long px = (long long)h * w, blocks = (long long)B * bh * bw;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "motion_refine_u8: B = %d frames of %d x %d are too large for one launch", B, h, w);
  const void* const ptrs[5] = {guide, prev_guide, vec, vec4, sad4};
  const long long bytes[5] = {B * px * 3, px * 3, blocks * 4, blocks * 4, blocks * 4};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 5), "motion_refine_u8: guide, prev_guide, vec, vec4 and sad4 must not overlap");
  hipStream_t s = (hipStream_t)stream;
  if (block == 8)
    sp_launch_refine<8>(subpel, (unsigned)blocks, s, guide, prev_guide, vec, vec4, sad4, h, w, bias, bh, bw);
  else if (block == 16)
    sp_launch_refine<16>(subpel, (unsigned)blocks, s, guide, prev_guide, vec, vec4, sad4, h, w, bias, bh, bw);
  else
    sp_launch_refine<32>(subpel, (unsigned)blocks, s, guide, prev_guide, vec, vec4, sad4, h, w, bias, bh, bw);
  CFEN_CHECK_LAUNCH("motion_refine_u8");
  return CFEN_OK;
}

extern "C" int cfen_motion_warp_subpel(const short* vec4, const unsigned char* prev_guide, const float* state, int h, int w, int block,
                                       unsigned char* prev_out, float* state_out, void* stream) {
  CFEN_CHECK_ARG(vec4 && prev_guide && state && prev_out && state_out,
                 "motion_warp_subpel: null pointer (vec4, prev_guide, state, prev_out and state_out are all required)");
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= SP_MAX_EDGE && w <= SP_MAX_EDGE, "motion_warp_subpel: sizes h = %d, w = %d outside 1 .. %d", h, w, SP_MAX_EDGE);
  CFEN_CHECK_ARG(sp_block_ok(block), "motion_warp_subpel: block = %d is none of 8, 16, 32", block);
  CFEN_CHECK_ARG(cfen_aligned(vec4, 4), "motion_warp_subpel: vec4 must be 4-byte aligned");
  CFEN_CHECK_ARG(cfen_aligned16(state) && cfen_aligned16(state_out), "motion_warp_subpel: state and state_out must be 16-byte aligned");
  const int bh = (h + block - 1) / block, bw = (w + block - 1) / block;
  const long long px = (long long)h * w;
  const void* const ptrs[5] = {vec4, prev_guide, state, prev_out, state_out};
  const long long bytes[5] = {(long long)bh * bw * 4, px * 3, px * 24, px * 3, px * 24};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 5), "motion_warp_subpel: vec4, prev_guide, state, prev_out and state_out must not overlap");
  const int shift = block == 8 ? 3 : block == 16 ? 4 : 5;
  CFEN_LAUNCH(k_subpel_warp, dim3((unsigned)((px + 511) / 512)), dim3(256), 0, (hipStream_t)stream, vec4, prev_guide, state, prev_out, state_out, h, w,
              shift, bw);
  CFEN_CHECK_LAUNCH("motion_warp_subpel");
  return CFEN_OK;
}
