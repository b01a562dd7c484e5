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
//   k_temporal_apply : the kernel that sees the full-resolution frame; k_guided_apply's scheme.  A workgroup of 4 waves takes 4 KiB of one output
//                      row (a lane 16 consecutive bytes), so y0, y1 and fy are block-uniform.  (1) the delta columns the run covers are
//                      interpolated vertically into LDS (TA_COLS columns at most; a run that covers more -- a downward or near-1:1 horizontal
//                      ratio, which the working resolution of frames up to 1024 pixels is -- reads both rows from global memory per pixel
//                      instead: a block-uniform choice, the same arithmetic); (2) one thread per pixel does the horizontal lerp and leaves DA
//                      and DB per output BYTE in LDS; (3) a lane reads its 16 hazy and 16 dehazed bytes (the loads are issued before (1)),
//                      16 + 16 deltas as four + four 16-byte LDS reads, and stores 16 bytes -- or single bytes when 3 W or a pointer is not a
//                      multiple of 16; the last lane of a row may then own fewer than 16 bytes.
// One launch each; no atomics, no counters, no scratch.
#include <math.h>

#include "../../include/cfen_temporal.h"
#include "cfen_common.hpp"

namespace {

constexpr int TB_T = 16;                       // tile edge of the blend kernel (256 threads, one pixel each)
constexpr int TB_RMAX = 16;
constexpr int TB_R = TB_T + 2 * TB_RMAX;       // 48: tile + halo at the largest radius
constexpr int TB_MAX_EDGE = 16384;             // (2y+1) h - H fits int32
constexpr int TA_RUN = 4096;                   // bytes of one output row per workgroup
constexpr int TA_COLS = 1024;                  // delta columns staged at most (24 KB)

// pixels of the window around `p` (radius r) that lie inside [0, n)
CFEN_DEV int tb_count(int p, int r, int n) { return min(p + r, n - 1) - max(p - r, 0) + 1; }

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
  const int N = tb_count(y, r, h) * tb_count(x, r, w);                                     // (meaningless, and unused, where the thread has no pixel)
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

// source coordinate of output index i on an axis in -> out: ((2i+1) in - out) / (2 out), clamped below at 0, in integers
CFEN_DEV void ta_coord(int i, int in, int out, int& i0, int& i1, float& f) {
  const int num = (2 * i + 1) * in - out, den = 2 * out;
  if (num <= 0) {
    i0 = 0;
    f = 0.f;
  } else {
    i0 = num / den;
    f = (float)(num - i0 * den) / (float)den;
  }
  i1 = min(i0 + 1, in - 1);
}

// (the clamp is on the float and the four bytes of a dword are put together with shifts and ors: a shift-then-clamp of int32 pairs may become
// gfx950's v_ashr_pk_u8_i32, which gave wrong bytes on the device: DESIGN sections 13 and 17)
CFEN_DEV unsigned ta_byte(float yv, float A, float g, float B) {
  float v = floorf((yv + A * g) + B + 0.5f);
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (unsigned)(int)v;
}

template <int V>
__global__ __launch_bounds__(256) void k_temporal_apply(const float* __restrict__ delta, const unsigned char* __restrict__ guide,
                                                        const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h, int w, int H,
                                                        int W, int nseg) {
  __shared__ __attribute__((aligned(16))) float sA[TA_RUN];
  __shared__ __attribute__((aligned(16))) float sB[TA_RUN];
  __shared__ float cv[TA_COLS * 6];
  const int tid = threadIdx.x;
  const int row = blockIdx.x / nseg, sg = blockIdx.x - row * nseg;                          // row = b * H + y
  const int b = row / H, y = row - b * H;
  const int pitch = W * 3;
  const int byte0 = sg * TA_RUN, off = byte0 + tid * 16;
  const unsigned char* grow = guide + (long long)row * pitch;
  const unsigned char* srow = src + (long long)row * pitch;
  union { uint4 q; unsigned u[4]; unsigned char c[16]; } gv, yv;
  if (V == 16) {
    if (off < pitch) {                                                                      // pitch % 16 == 0: a lane's 16 bytes are whole or absent
      gv.q = *reinterpret_cast<const uint4*>(grow + off);
      yv.q = *reinterpret_cast<const uint4*>(srow + off);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      gv.c[j] = off + j < pitch ? grow[off + j] : (unsigned char)0;
      yv.c[j] = off + j < pitch ? srow[off + j] : (unsigned char)0;
    }
  }
  int y0, y1;
  float fy;
  ta_coord(y, h, H, y0, y1, fy);
  const int pfirst = byte0 / 3, plast = min((byte0 + TA_RUN - 1) / 3, W - 1);
  int cfirst, clast, unused;
  float unusedf;
  ta_coord(pfirst, w, W, cfirst, unused, unusedf);
  ta_coord(plast, w, W, unused, clast, unusedf);
  const int ncols = clast - cfirst + 1;
  const bool staged = ncols <= TA_COLS;                                                    // block-uniform
  const float* c0 = delta + ((long long)b * h + y0) * w * 6;
  const float* c1 = delta + ((long long)b * h + y1) * w * 6;
  if (staged) {
    for (int i = tid; i < ncols * 6; i += 256) {
      const float lo = c0[cfirst * 6 + i], hi = c1[cfirst * 6 + i];
      cv[i] = lo + fy * (hi - lo);
    }
  }
  __syncthreads();
  for (int p = pfirst + tid; p <= plast; p += 256) {
    int xa, xb;
    float fx;
    ta_coord(p, w, W, xa, xb, fx);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      float l, r;
      if (staged) {
        l = cv[(xa - cfirst) * 6 + k];
        r = cv[(xb - cfirst) * 6 + k];
      } else {
        const float l0 = c0[xa * 6 + k], l1 = c1[xa * 6 + k], r0 = c0[xb * 6 + k], r1 = c1[xb * 6 + k];
        l = l0 + fy * (l1 - l0);
        r = r0 + fy * (r1 - r0);
      }
      const int idx = p * 3 + (k < 3 ? k : k - 3) - byte0;                                   // the run may begin or end inside a pixel
      if (idx >= 0 && idx < TA_RUN) (k < 3 ? sA : sB)[idx] = l + fx * (r - l);
    }
  }
  __syncthreads();
  if (off >= pitch) return;
  unsigned char* drow = dst + (long long)row * pitch;
  if (V == 16) {
    union { uint4 q; unsigned u[4]; } o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const floatx4 A = *reinterpret_cast<const floatx4*>(&sA[tid * 16 + d * 4]), Bv = *reinterpret_cast<const floatx4*>(&sB[tid * 16 + d * 4]);
      const unsigned g = gv.u[d], s = yv.u[d];
      o.u[d] = ta_byte((float)(s & 255u), A[0], (float)(g & 255u), Bv[0]) | (ta_byte((float)((s >> 8) & 255u), A[1], (float)((g >> 8) & 255u), Bv[1]) << 8) |
               (ta_byte((float)((s >> 16) & 255u), A[2], (float)((g >> 16) & 255u), Bv[2]) << 16) |
               (ta_byte((float)(s >> 24), A[3], (float)(g >> 24), Bv[3]) << 24);
    }
    *reinterpret_cast<uint4*>(drow + off) = o.q;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (off + j < pitch) drow[off + j] = (unsigned char)ta_byte((float)yv.c[j], sA[tid * 16 + j], (float)gv.c[j], sB[tid * 16 + j]);
  }
}

bool tp_overlap(const void* p, long long np, const void* q, long long nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

// no two of the n ranges overlap (a null pointer is a range that is not there)
bool tp_disjoint(const void* const* p, const long long* bytes, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (p[i] && p[j] && tp_overlap(p[i], bytes[i], p[j], bytes[j])) return false;
  return true;
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
  CFEN_CHECK_ARG(tp_disjoint(ptrs, bytes, 5), "temporal_blend: guide, prev_guide, coef, state and delta must not overlap");
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
  CFEN_CHECK_ARG(tp_disjoint(ptrs, bytes, 4), "temporal_apply_u8: delta, guide_hi, src_hi and dst must not overlap");
  const int pitch = W * 3, nseg = (pitch + TA_RUN - 1) / TA_RUN;
  const long long blocks = (long long)B * H * nseg;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "temporal_apply_u8: B = %d images of %d x %d are too large for one launch", B, H, W);
  hipStream_t s = (hipStream_t)stream;
  const uintptr_t all = reinterpret_cast<uintptr_t>(guide_hi) | reinterpret_cast<uintptr_t>(src_hi) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)pitch;
  if (all % 16 == 0)
    CFEN_LAUNCH(k_temporal_apply<16>, dim3((unsigned)blocks), dim3(256), 0, s, delta, guide_hi, src_hi, dst, h, w, H, W, nseg);
  else
    CFEN_LAUNCH(k_temporal_apply<1>, dim3((unsigned)blocks), dim3(256), 0, s, delta, guide_hi, src_hi, dst, h, w, H, W, nseg);
  CFEN_CHECK_LAUNCH("temporal_apply_u8");
  return CFEN_OK;
}
