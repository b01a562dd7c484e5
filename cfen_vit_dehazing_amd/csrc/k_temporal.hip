// Temporal stabilisation of a dehazed stream (include/cfen_temporal.h states the definition and the contract; tests/temporal_ref.py restates it).
//
// The coefficient fields (a, b) of the local linear model of include/cfen_guided.h are smoothed over time by a recursion that a motion test
// switches off where the scene changed, and the CHANGE of the coefficients is applied to the full-resolution output.
//
//   k_temporal_blend : a workgroup takes TB_T x TB_T = 16 x 16 pixels and walks the B frames of the call in order, the recursion's S in six
//                      registers per thread.  Per frame the per-pixel sum over the channels of |I_k - I_{k-1}| of the tile with its halo of r
//                      (zeros outside the image) goes to LDS as 16-bit integers (at most 765); the window sum D is formed separably in int32
//                      (row sums of the (16 + 2r) x 16 strip into LDS, then one column sum per thread), as k_guided_coef forms its sums.  The
//                      previous frame's bytes are only read: neighbouring tiles read them as halo.  state is read and written by the thread that
//                      owns the pixel, once each.
//   k_temporal_apply : the kernel that sees the full-resolution frame: img_affine_apply (cfen_image.hpp) on the delta field with the dehazed
//                      frame as second byte row, dst = (y + DA g) + DB.  At the working resolution of frames up to 1024 pixels the ratio is
//                      near 1:1, so its runs usually take the unstaged path.
// One launch each; no atomics, no counters, no scratch.
#include <math.h>

#include "../../include/cfen_temporal.h"
#include "cfen_image.hpp"

namespace {

constexpr int TB_T = 16;                       // tile edge of the blend kernel (256 threads, one pixel each)
constexpr int TB_RMAX = 16;
constexpr int TB_R = TB_T + 2 * TB_RMAX;       // 48: tile + halo at the largest radius
constexpr int TB_MAX_EDGE = 16384;             // (2y+1) h - H fits int32

__global__ __launch_bounds__(256) void k_temporal_blend(const unsigned char* __restrict__ guide, const unsigned char* __restrict__ prev_guide,
                                                        const float* __restrict__ coef, float* __restrict__ state, float* __restrict__ delta,
                                                        int B, int h, int w, int r, float motion, float strength, int have_state, int ntx) {
  __shared__ unsigned short sD[TB_R][TB_R];
  __shared__ int rs[TB_R][TB_T];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int y0 = (blockIdx.x / ntx) * TB_T, x0 = (blockIdx.x % ntx) * TB_T;
  const int R = TB_T + 2 * r;
  const int y = y0 + ty, x = x0 + tx;
  const bool own = y < h && x < w;
  const int N = img_window_count(y, r, h) * img_window_count(x, r, w);                                     // (meaningless, and unused, where the thread has no pixel)
  const long long frame = (long long)h * w;
  const long long px = own ? (long long)y * w + x : 0;
  float S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (own && have_state) {
#pragma unroll
    for (int j = 0; j < 6; ++j) S[j] = state[px * 6 + j];
  }
  for (int k = 0; k < B; ++k) {
    float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (own) {
#pragma unroll
      for (int j = 0; j < 6; ++j) c[j] = coef[(k * frame + px) * 6 + j];
    }
    float dl[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k == 0 && !have_state) {                                                            // block-uniform: the first frame of a stream
#pragma unroll
      for (int j = 0; j < 6; ++j) S[j] = c[j];
    } else {
      const unsigned char* cur = guide + k * frame * 3;
      const unsigned char* prv = k ? cur - frame * 3 : prev_guide;
      for (int i = tid; i < R * R; i += 256) {
        const int ry = i / R, rx = i - ry * R;
        const int gy = y0 - r + ry, gx = x0 - r + rx;
        int d = 0;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
          const long long o = ((long long)gy * w + gx) * 3;
          d = abs((int)cur[o] - (int)prv[o]) + abs((int)cur[o + 1] - (int)prv[o + 1]) + abs((int)cur[o + 2] - (int)prv[o + 2]);
        }
        sD[ry][rx] = (unsigned short)d;
      }
      __syncthreads();
      for (int i = tid; i < R * TB_T; i += 256) {                                           // row sums: strip row ry, tile column cx
        const int ry = i >> 4, cx = i & 15;
        int s = 0;
        for (int d = 0; d <= 2 * r; ++d) s += sD[ry][cx + d];
        rs[ry][cx] = s;
      }
      __syncthreads();
      int D = 0;
      for (int d = 0; d <= 2 * r; ++d) D += rs[ty + d][tx];
      // (no third barrier: the next frame's sD is written while others still read rs, and its rs only after that frame's first barrier)
      const float dm = (float)D / (float)(3 * N);
      const float keep = fminf(fmaxf(1.f - dm / motion, 0.f), 1.f);
      const float kk = strength * keep;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        S[j] = c[j] + kk * (S[j] - c[j]);
        dl[j] = S[j] - c[j];
      }
    }
    if (own) {
      float* o = delta + (k * frame + px) * 6;
#pragma unroll
      for (int j = 0; j < 6; ++j) o[j] = dl[j];
    }
  }
  if (own) {
#pragma unroll
    for (int j = 0; j < 6; ++j) state[px * 6 + j] = S[j];
  }
}

template <int V>
__global__ __launch_bounds__(256) void k_temporal_apply(const float* __restrict__ delta, const unsigned char* __restrict__ guide,
                                                        const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, int H,
                                                        int W, int nseg) {
  img_affine_apply<V, true>(delta, guide, src, dst, h, w, H, W, nseg);
}

}  // namespace

extern "C" int cfen_temporal_blend(const unsigned char* guide, const unsigned char* prev_guide, const float* coef, int B, int h, int w, int radius,
                                   float motion, float strength, int have_state, float* state, float* delta, void* stream) {
  CFEN_CHECK_ARG(guide && coef && state && delta, "temporal_blend: null pointer (guide, coef, state and delta are all required)");
  CFEN_CHECK_ARG(have_state == 0 || have_state == 1, "temporal_blend: have_state = %d is neither 0 nor 1", have_state);
  CFEN_CHECK_ARG(!have_state || prev_guide, "temporal_blend: null pointer (have_state = 1 needs prev_guide)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "temporal_blend: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= TB_MAX_EDGE && w <= TB_MAX_EDGE, "temporal_blend: sizes h = %d, w = %d outside 1 .. %d", h, w, TB_MAX_EDGE);
  CFEN_CHECK_ARG(radius >= 1 && radius <= TB_RMAX, "temporal_blend: radius = %d outside 1 .. %d", radius, TB_RMAX);
  CFEN_CHECK_ARG(isfinite(motion) && motion > 0.f, "temporal_blend: motion = %g must be finite and > 0", (double)motion);
  CFEN_CHECK_ARG(strength >= 0.f && strength < 1.f, "temporal_blend: strength = %g outside [0, 1)", (double)strength);
  CFEN_CHECK_ARG(cfen_aligned16(coef) && cfen_aligned16(state) && cfen_aligned16(delta), "temporal_blend: coef, state and delta must be 16-byte aligned");
  const long long px = (long long)h * w;
  const void* const ptrs[5] = {guide, have_state ? prev_guide : nullptr, coef, state, delta};
  const long long bytes[5] = {B * px * 3, px * 3, B * px * 24, px * 24, B * px * 24};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 5), "temporal_blend: guide, prev_guide, coef, state and delta must not overlap");
  const int ntx = (w + TB_T - 1) / TB_T, nty = (h + TB_T - 1) / TB_T;
  hipStream_t s = (hipStream_t)stream;
  CFEN_LAUNCH(k_temporal_blend, dim3((unsigned)(ntx * nty)), dim3(256), 0, s, guide, prev_guide, coef, state, delta, B, h, w, radius, motion, strength,
              have_state, ntx);
  CFEN_CHECK_LAUNCH("temporal_blend");
  return CFEN_OK;
}

extern "C" int cfen_temporal_apply_u8(const float* delta, int B, int h, int w, const unsigned char* guide_hi, const unsigned char* src_hi, int H, int W,
                                      unsigned char* dst, void* stream) {
  CFEN_CHECK_ARG(delta && guide_hi && src_hi && dst, "temporal_apply_u8: null pointer (delta, guide_hi, src_hi and dst are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "temporal_apply_u8: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1 && h <= TB_MAX_EDGE && w <= TB_MAX_EDGE && H <= TB_MAX_EDGE && W <= TB_MAX_EDGE,
                 "temporal_apply_u8: sizes h = %d, w = %d, H = %d, W = %d outside 1 .. %d", h, w, H, W, TB_MAX_EDGE);
  CFEN_CHECK_ARG(cfen_aligned16(delta), "temporal_apply_u8: delta must be 16-byte aligned");
  const long long lo = (long long)B * h * w * 24, hi = (long long)B * H * W * 3;
  const void* const ptrs[4] = {delta, guide_hi, src_hi, dst};
  const long long bytes[4] = {lo, hi, hi, hi};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 4), "temporal_apply_u8: delta, guide_hi, src_hi and dst must not overlap");
  IMG_LAUNCH_APPLY(k_temporal_apply, "temporal_apply_u8", (hipStream_t)stream, B, h, w, H, W,
                   reinterpret_cast<uintptr_t>(guide_hi) | reinterpret_cast<uintptr_t>(src_hi) | reinterpret_cast<uintptr_t>(dst), delta, guide_hi, src_hi,
                   dst);
  return CFEN_OK;
}
