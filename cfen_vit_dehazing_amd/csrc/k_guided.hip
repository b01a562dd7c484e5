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
//   k_guided_apply : the kernel that sees the full-resolution image: img_affine_apply (cfen_image.hpp) on the coefficient field, dst = A g + B.
// Three launches; no atomics, no counters, no scratch.
#include <math.h>

#include "../../include/cfen_guided.h"
#include "cfen_image.hpp"

namespace {

constexpr int GD_T = 16;                       // tile edge of the two low-resolution kernels (256 threads, one pixel each)
constexpr int GD_RMAX = 16;
constexpr int GD_R = GD_T + 2 * GD_RMAX;       // 48: tile + halo at the largest radius
constexpr int GD_MAX_EDGE = 16384;             // (2y+1) h - H fits int32

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
  const int N = img_window_count(y, r, h) * img_window_count(x, r, w);                                     // (meaningless, and unused, where the thread has no pixel)
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
  const float N = (float)(img_window_count(y, r, h) * img_window_count(x, r, w));
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

template <int V>
__global__ __launch_bounds__(256) void k_guided_apply(const float* __restrict__ coef, const unsigned char* __restrict__ guide, unsigned char* __restrict__ dst,
                                                      int h, int w, int H, int W, int nseg) {
  img_affine_apply<V, false>(coef, guide, nullptr, dst, h, w, H, W, nseg);
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
  const void* const ptrs[4] = {guide, src, tmp, coef};
  const long long bytes[4] = {px * 3, px * 3, px * 24, px * 24};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 4), "guided_coef_u8: guide, src, tmp and coef must not overlap");
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
  const void* const ptrs[3] = {coef, guide_hi, dst};
  const long long bytes[3] = {lo, hi, hi};
  CFEN_CHECK_ARG(cfen_ranges_disjoint(ptrs, bytes, 3), "guided_apply_u8: coef, guide_hi and dst must not overlap");
  IMG_LAUNCH_APPLY(k_guided_apply, "guided_apply_u8", (hipStream_t)stream, B, h, w, H, W,
                   reinterpret_cast<uintptr_t>(guide_hi) | reinterpret_cast<uintptr_t>(dst), coef, guide_hi, dst);
  return CFEN_OK;
}
