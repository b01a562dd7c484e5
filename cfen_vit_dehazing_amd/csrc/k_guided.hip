// Guided upsampling of 8-bit RGB images (include/cfen_guided.h states the definition and the contract; tests/guided_ref.py restates it).
//
// At low resolution a local linear model P ~ a I + b between the hazy input I and the network's output P is fitted per pixel and channel over a
// (2r+1)^2 window, the coefficients are box-smoothed, upsampled bilinearly and applied to the FULL-resolution hazy image.
//
//   k_guided_coef  : a workgroup takes GD_T x GD_T = 16 x 16 pixels: the tile of I and P with its halo of r (zeros outside the image) goes to
//                    LDS as bytes; per channel the four window sums S_I, S_P, S_II, S_IP are formed separably in int32 (row sums of the
//                    (16 + 2r) x 16 strip into LDS, then one column sum per thread), C and V in int64, a and b by two fp32 divisions.
//                    Channel by channel: the row sums of one channel are 12 KB at r = 16, all three with the 13.5 KB of bytes would not leave
//                    room for a second workgroup's worth of LDS.
//   k_guided_mean  : the same separable box on the six fp32 planes of tmp, one plane at a time, divided by N.
//   k_guided_apply : the kernel that sees the full-resolution image.  A workgroup of 4 waves takes 4 KiB of one output row (a wave 1 KiB, a lane
//                    16 consecutive bytes), so y0, y1 and fy are block-uniform.  (1) the coefficient columns the run covers, [x0 of its first
//                    pixel, x1 of its last], are interpolated vertically into LDS (GA_COLS columns at most; a run that covers more -- a
//                    downward or near-1:1 horizontal ratio -- reads both rows from global memory per pixel instead: a block-uniform choice,
//                    the same arithmetic); (2) one thread per pixel does the horizontal lerp and leaves Abar and Bbar per output BYTE in LDS;
//                    (3) a lane reads its 16 guide bytes (the load is issued before (1)), 16 + 16 coefficients as four + four 16-byte LDS
//                    reads, and stores 16 bytes -- or single bytes when 3 W or a pointer is not a multiple of 16; the last lane of a row may then
//                    own fewer than 16 bytes.
// Three launches; no atomics, no counters, no scratch.
#include <math.h>

#include "../../include/cfen_guided.h"
#include "cfen_common.hpp"

namespace {

constexpr int GD_T = 16;                       // tile edge of the two low-resolution kernels (256 threads, one pixel each)
constexpr int GD_RMAX = 16;
constexpr int GD_R = GD_T + 2 * GD_RMAX;       // 48: tile + halo at the largest radius
constexpr int GD_MAX_EDGE = 16384;             // (2y+1) h - H fits int32
constexpr int GA_RUN = 4096;                   // bytes of one output row per workgroup
constexpr int GA_COLS = 1024;                  // coefficient columns staged at most (24 KB)

// pixels of the window around `p` (radius r) that lie inside [0, n)
CFEN_DEV int gd_count(int p, int r, int n) { return min(p + r, n - 1) - max(p - r, 0) + 1; }

__global__ __launch_bounds__(256) void k_guided_coef(const unsigned char* __restrict__ guide, const unsigned char* __restrict__ src, float* __restrict__ tmp,
                                                     int h, int w, int r, float eps255, int ntx, int nty) {
  __shared__ unsigned char sI[GD_R][GD_R * 3];
  __shared__ unsigned char sP[GD_R][GD_R * 3];
  __shared__ int rs[4][GD_R][GD_T];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int b = blockIdx.x / (ntx * nty), t = blockIdx.x - b * (ntx * nty);
  const int y0 = (t / ntx) * GD_T, x0 = (t % ntx) * GD_T;
  const int R = GD_T + 2 * r, rowbytes = R * 3;
  const unsigned char* gI = guide + (long long)b * h * w * 3;
  const unsigned char* gP = src + (long long)b * h * w * 3;
  for (int i = tid; i < R * rowbytes; i += 256) {
    const int ry = i / rowbytes, rb = i - ry * rowbytes;
    const int gy = y0 - r + ry, gb = (x0 - r) * 3 + rb;                                    // row, and byte of that row, in the image
    const bool in = gy >= 0 && gy < h && gb >= 0 && gb < w * 3;
    const long long o = (long long)gy * w * 3 + gb;
    sI[ry][rb] = in ? gI[o] : (unsigned char)0;
    sP[ry][rb] = in ? gP[o] : (unsigned char)0;
  }
  __syncthreads();
  const int y = y0 + ty, x = x0 + tx;
  const int N = gd_count(y, r, h) * gd_count(x, r, w);                                     // (meaningless, and unused, where the thread has no pixel)
  float a[3], bb[3];
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < R * GD_T; i += 256) {                                            // row sums: strip row ry, tile column cx
      const int ry = i >> 4, cx = i & 15;
      int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
      for (int d = 0; d <= 2 * r; ++d) {
        const int vi = sI[ry][(cx + d) * 3 + c], vp = sP[ry][(cx + d) * 3 + c];
        s0 += vi;
        s1 += vp;
        s2 += vi * vi;
        s3 += vi * vp;
      }
      rs[0][ry][cx] = s0;
      rs[1][ry][cx] = s1;
      rs[2][ry][cx] = s2;
      rs[3][ry][cx] = s3;
    }
    __syncthreads();
    int SI = 0, SP = 0, SII = 0, SIP = 0;
    for (int d = 0; d <= 2 * r; ++d) {
      SI += rs[0][ty + d][tx];
      SP += rs[1][ty + d][tx];
      SII += rs[2][ty + d][tx];
      SIP += rs[3][ty + d][tx];
    }
    __syncthreads();                                                                       // the next channel overwrites rs
    const long long C = (long long)N * SIP - (long long)SI * SP;
    const long long V = (long long)N * SII - (long long)SI * SI;
    a[c] = (float)C / ((float)V + eps255 * (float)(N * N));
    bb[c] = ((float)SP - a[c] * (float)SI) / (float)N;
  }
  if (y < h && x < w) {
    float* o = tmp + (((long long)b * h + y) * w + x) * 6;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
    o[3] = bb[0]; o[4] = bb[1]; o[5] = bb[2];
  }
}

__global__ __launch_bounds__(256) void k_guided_mean(const float* __restrict__ tmp, float* __restrict__ coef, int h, int w, int r, int ntx, int nty) {
  __shared__ float sT[GD_R][GD_R];
  __shared__ float rs[GD_R][GD_T];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int b = blockIdx.x / (ntx * nty), t = blockIdx.x - b * (ntx * nty);
  const int y0 = (t / ntx) * GD_T, x0 = (t % ntx) * GD_T;
  const int R = GD_T + 2 * r;
  const float* g = tmp + (long long)b * h * w * 6;
  const int y = y0 + ty, x = x0 + tx;
  const float N = (float)(gd_count(y, r, h) * gd_count(x, r, w));
  float m[6];
  for (int k = 0; k < 6; ++k) {
    for (int i = tid; i < R * R; i += 256) {
      const int ry = i / R, rx = i - ry * R;
      const int gy = y0 - r + ry, gx = x0 - r + rx;
      sT[ry][rx] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? g[((long long)gy * w + gx) * 6 + k] : 0.f;      // + 0 outside the image: exact
    }
    __syncthreads();
    for (int i = tid; i < R * GD_T; i += 256) {
      const int ry = i >> 4, cx = i & 15;
      float s = 0.f;
      for (int d = 0; d <= 2 * r; ++d) s += sT[ry][cx + d];
      rs[ry][cx] = s;
    }
    __syncthreads();
    float s = 0.f;
    for (int d = 0; d <= 2 * r; ++d) s += rs[ty + d][tx];
    m[k] = s / N;
    __syncthreads();                                                                       // the next plane overwrites sT and rs
  }
  if (y < h && x < w) {
    float* o = coef + (((long long)b * h + y) * w + x) * 6;
    for (int k = 0; k < 6; ++k) o[k] = m[k];
  }
}

// source coordinate of output index i on an axis in -> out: ((2i+1) in - out) / (2 out), clamped below at 0, in integers
CFEN_DEV void ga_coord(int i, int in, int out, int& i0, int& i1, float& f) {
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

// (the compiler may fuse a shift-then-clamp of two int32 into gfx950's v_ashr_pk_u8_i32, which gave wrong bytes on the device in a variant of
// k_resample_v: DESIGN section 13.  Here the clamp is on the float and the four bytes of a dword are put together with shifts and ors)
CFEN_DEV unsigned ga_byte(float A, float g, float B) {
  float v = floorf(A * g + B + 0.5f);
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (unsigned)(int)v;
}

template <int V>
__global__ __launch_bounds__(256) void k_guided_apply(const float* __restrict__ coef, const unsigned char* __restrict__ guide, unsigned char* __restrict__ dst,
                                                      int h, int w, int H, int W, int nseg) {
  __shared__ __attribute__((aligned(16))) float sA[GA_RUN];
  __shared__ __attribute__((aligned(16))) float sB[GA_RUN];
  __shared__ float cv[GA_COLS * 6];
  const int tid = threadIdx.x;
  const int row = blockIdx.x / nseg, sg = blockIdx.x - row * nseg;                          // row = b * H + y
  const int b = row / H, y = row - b * H;
  const int pitch = W * 3;
  const int byte0 = sg * GA_RUN, off = byte0 + tid * 16;
  const unsigned char* grow = guide + (long long)row * pitch;
  union { uint4 q; unsigned u[4]; unsigned char c[16]; } gv;
  if (V == 16) {
    if (off < pitch) gv.q = *reinterpret_cast<const uint4*>(grow + off);                    // pitch % 16 == 0: a lane's 16 bytes are whole or absent
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) gv.c[j] = off + j < pitch ? grow[off + j] : (unsigned char)0;
  }
  int y0, y1;
  float fy;
  ga_coord(y, h, H, y0, y1, fy);
  const int pfirst = byte0 / 3, plast = min((byte0 + GA_RUN - 1) / 3, W - 1);
  int cfirst, clast, unused;
  float unusedf;
  ga_coord(pfirst, w, W, cfirst, unused, unusedf);
  ga_coord(plast, w, W, unused, clast, unusedf);
  const int ncols = clast - cfirst + 1;
  const bool staged = ncols <= GA_COLS;                                                    // block-uniform
  const float* c0 = coef + ((long long)b * h + y0) * w * 6;
  const float* c1 = coef + ((long long)b * h + y1) * w * 6;
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
    ga_coord(p, w, W, xa, xb, fx);
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
      if (idx >= 0 && idx < GA_RUN) (k < 3 ? sA : sB)[idx] = l + fx * (r - l);
    }
  }
  __syncthreads();
  if (off >= pitch) return;
  unsigned char* drow = dst + (long long)row * pitch;
  if (V == 16) {
    union { uint4 q; unsigned u[4]; } o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const floatx4 A = *reinterpret_cast<const floatx4*>(&sA[tid * 16 + d * 4]), B = *reinterpret_cast<const floatx4*>(&sB[tid * 16 + d * 4]);
      const unsigned g = gv.u[d];
      o.u[d] = ga_byte(A[0], (float)(g & 255u), B[0]) | (ga_byte(A[1], (float)((g >> 8) & 255u), B[1]) << 8) |
               (ga_byte(A[2], (float)((g >> 16) & 255u), B[2]) << 16) | (ga_byte(A[3], (float)(g >> 24), B[3]) << 24);
    }
    *reinterpret_cast<uint4*>(drow + off) = o.q;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (off + j < pitch) drow[off + j] = (unsigned char)ga_byte(sA[tid * 16 + j], (float)gv.c[j], sB[tid * 16 + j]);
  }
}

bool gd_overlap(const void* p, long long np, const void* q, long long nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

}  // namespace

extern "C" int cfen_guided_coef_u8(const unsigned char* guide, const unsigned char* src, int B, int h, int w, int radius, float eps255, float* tmp,
                                   float* coef, void* stream) {
  CFEN_CHECK_ARG(guide && src && tmp && coef, "guided_coef_u8: null pointer (guide, src, tmp and coef are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "guided_coef_u8: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && h <= GD_MAX_EDGE && w <= GD_MAX_EDGE, "guided_coef_u8: sizes h = %d, w = %d outside 1 .. %d", h, w, GD_MAX_EDGE);
  CFEN_CHECK_ARG(radius >= 1 && radius <= GD_RMAX, "guided_coef_u8: radius = %d outside 1 .. %d", radius, GD_RMAX);
  CFEN_CHECK_ARG(isfinite(eps255) && eps255 > 0.f, "guided_coef_u8: eps255 = %g must be finite and > 0", (double)eps255);
  CFEN_CHECK_ARG(cfen_aligned16(tmp) && cfen_aligned16(coef), "guided_coef_u8: tmp and coef must be 16-byte aligned");
  const long long px = (long long)B * h * w;
  CFEN_CHECK_ARG(!gd_overlap(tmp, px * 24, coef, px * 24) && !gd_overlap(guide, px * 3, src, px * 3) && !gd_overlap(guide, px * 3, tmp, px * 24) &&
                 !gd_overlap(guide, px * 3, coef, px * 24) && !gd_overlap(src, px * 3, tmp, px * 24) && !gd_overlap(src, px * 3, coef, px * 24),
                 "guided_coef_u8: guide, src, tmp and coef must not overlap");
  const int ntx = (w + GD_T - 1) / GD_T, nty = (h + GD_T - 1) / GD_T;
  const long long blocks = (long long)B * ntx * nty;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "guided_coef_u8: B = %d images of %d x %d are too large for one launch", B, h, w);
  hipStream_t s = (hipStream_t)stream;
  CFEN_LAUNCH(k_guided_coef, dim3((unsigned)blocks), dim3(256), 0, s, guide, src, tmp, h, w, radius, eps255, ntx, nty);
  CFEN_CHECK_LAUNCH("guided_coef_u8 (coefficients)");
  CFEN_LAUNCH(k_guided_mean, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)tmp, coef, h, w, radius, ntx, nty);
  CFEN_CHECK_LAUNCH("guided_coef_u8 (mean)");
  return CFEN_OK;
}

extern "C" int cfen_guided_apply_u8(const float* coef, int B, int h, int w, const unsigned char* guide_hi, int H, int W, unsigned char* dst,
                                    void* stream) {
  CFEN_CHECK_ARG(coef && guide_hi && dst, "guided_apply_u8: null pointer (coef, guide_hi and dst are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "guided_apply_u8: B = %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(h >= 1 && w >= 1 && H >= 1 && W >= 1 && h <= GD_MAX_EDGE && w <= GD_MAX_EDGE && H <= GD_MAX_EDGE && W <= GD_MAX_EDGE,
                 "guided_apply_u8: sizes h = %d, w = %d, H = %d, W = %d outside 1 .. %d", h, w, H, W, GD_MAX_EDGE);
  CFEN_CHECK_ARG(cfen_aligned16(coef), "guided_apply_u8: coef must be 16-byte aligned");
  const long long lo = (long long)B * h * w * 24, hi = (long long)B * H * W * 3;
  CFEN_CHECK_ARG(!gd_overlap(guide_hi, hi, dst, hi) && !gd_overlap(coef, lo, dst, hi) && !gd_overlap(coef, lo, guide_hi, hi),
                 "guided_apply_u8: coef, guide_hi and dst must not overlap");
  const int pitch = W * 3, nseg = (pitch + GA_RUN - 1) / GA_RUN;
  const long long blocks = (long long)B * H * nseg;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "guided_apply_u8: B = %d images of %d x %d are too large for one launch", B, H, W);
  hipStream_t s = (hipStream_t)stream;
  const uintptr_t both = reinterpret_cast<uintptr_t>(guide_hi) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)pitch;
  if (both % 16 == 0)
    CFEN_LAUNCH(k_guided_apply<16>, dim3((unsigned)blocks), dim3(256), 0, s, coef, guide_hi, dst, h, w, H, W, nseg);
  else
    CFEN_LAUNCH(k_guided_apply<1>, dim3((unsigned)blocks), dim3(256), 0, s, coef, guide_hi, dst, h, w, H, W, nseg);
  CFEN_CHECK_LAUNCH("guided_apply_u8");
  return CFEN_OK;
}
