// Image quality of a dehazed output against its ground truth (metrics.py, test.py --eval): per image pair the sum of squared errors (for PSNR)
// and the mean SSIM, in ONE fused pass -- no mu / sigma maps ever reach HBM.
//
// Definition (include/cfen_hip.h): both images on the [0,1] scale in fp32; SSIM is the reference's pytorch_msssim.ssim(window_size = 11,
// size_average = True, val_range = 1) (pytorch_msssim/__init__.py:19-70): an 11 x 11 Gaussian window (sigma 1.5, normalised), VALID convolution,
// C1 = 0.01^2, C2 = 0.03^2, the mean over all C (H - 10) (W - 10) window positions.
//
//   k_image_metrics : a workgroup (256 threads) owns MT_H x MT_W = 24 x 64 window positions of one image pair.  Per channel it
//                       1. stages the (24 + 10) x (64 + 10) pixels under those windows of both images in LDS as fp32 (zeros past the image), and adds
//                          the squared error of the pixels the tile OWNS: [y0, y0 + 24) x [x0, x0 + 64), the last tile row / column up to the image
//                          edge -- so the 10-pixel border without a window of its own is counted, every pixel exactly once;
//                       2. row pass: the 11-tap filter along x over a, b, a^2, b^2, ab -> five (34 x 64) planes in LDS; a wave reads 64 consecutive
//                          floats per tap (conflict-free);
//                       3. column pass: a thread owns one column and 6 consecutive rows, reads the 16 row-filtered values under them once per plane
//                          and forms 6 SSIM map values.
//                     Per-thread sums are fp64 (the squared error of uint8 input is summed in integers first: exact), reduced over the wave with
//                     shuffles, over the 4 waves through LDS in wave order, and written as this tile's (sse, ssim sum) pair to `part`.
//   k_image_metrics_finish : one workgroup per image adds the tiles' pairs in a fixed order in fp64 (thread t takes tiles t, t + 256, ... in
//                     increasing order, then a fixed LDS tree) and writes out[b] = (sse, ssim sum / count).
// No atomics and no counters: the same inputs give the same bits on every run, on any stream, at any batch size.
#include "cfen_common.hpp"

namespace {

constexpr int MT_H = 24, MT_W = 64, MT_HALO = 10, MT_TAPS = 11;
constexpr int MT_SH = MT_H + MT_HALO, MT_SW = MT_W + MT_HALO;   // staged rows / columns
constexpr int MT_R = MT_H / 4;                                   // rows per thread in the column pass (4 waves, one column per lane)

// exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, evaluated in fp64 and rounded once
__constant__ const float MT_G[MT_TAPS] = {1.028380084e-03f, 7.598758135e-03f, 3.600077213e-02f, 1.093606895e-01f, 2.130055377e-01f, 2.660117249e-01f,
                                          2.130055377e-01f, 1.093606895e-01f, 3.600077213e-02f, 7.598758135e-03f, 1.028380084e-03f};

struct MetricsGeom {
  int C, H, W, nty, ntx;
  float lo, range;      // fp32 input: v -> (v - lo) / range
};

CFEN_DEV double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // butterfly: every lane ends with the bitwise identical total
  return v;
}

// one SSIM map value from the five filtered quantities.  No FMA contraction: with a == b the numerator and the denominator must come out
// bitwise equal (2 m m against m m + m m), so that identical images score exactly 1
CFEN_DEV float ssim_value(float mu1, float mu2, float e11, float e22, float e12) {
#pragma clang fp contract(off)
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
  const float v1 = 2.0f * sigma12 + C2, v2 = sigma1_sq + sigma2_sq + C2;
  return ((2.0f * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2);
}

template <bool U8>
__global__ __launch_bounds__(256) void k_image_metrics(const void* __restrict__ pa, const void* __restrict__ pb, MetricsGeom g,
                                                       double* __restrict__ part) {
  __shared__ float sa[MT_SH][MT_SW], sb[MT_SH][MT_SW];
  __shared__ float hq[5][MT_SH][MT_W];
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int ty = tile / g.ntx, tx = tile - ty * g.ntx;
  const int y0 = ty * MT_H, x0 = tx * MT_W;
  const int H = g.H, W = g.W;
  // pixels this tile owns for the squared error
  const int own_y1 = ty == g.nty - 1 ? H : y0 + MT_H, own_x1 = tx == g.ntx - 1 ? W : x0 + MT_W;
  const long long plane = (long long)H * W;
  unsigned sse_u = 0;
  double sse_d = 0.0, ssim_d = 0.0;

  for (int c = 0; c < g.C; ++c) {
    // 1. stage
    for (int i = tid; i < MT_SH * MT_SW; i += 256) {
      const int r = i / MT_SW, q = i - r * MT_SW;
      const int y = y0 + r, x = x0 + q;
      float va = 0.f, vb = 0.f;
      if (y < H && x < W) {
        const bool own = y < own_y1 && x < own_x1;
        if (U8) {
          const long long o = (((long long)b * H + y) * W + x) * 3 + c;
          const int ia = static_cast<const unsigned char*>(pa)[o], ib = static_cast<const unsigned char*>(pb)[o];
          va = __fdiv_rn((float)ia, 255.0f);
          vb = __fdiv_rn((float)ib, 255.0f);
          if (own) sse_u += (unsigned)((ia - ib) * (ia - ib));
        } else {
          const long long o = ((long long)b * g.C + c) * plane + (long long)y * W + x;
          va = __fdiv_rn(static_cast<const float*>(pa)[o] - g.lo, g.range);
          vb = __fdiv_rn(static_cast<const float*>(pb)[o] - g.lo, g.range);
          if (own) {
            const double d = 255.0 * ((double)va - (double)vb);
            sse_d += d * d;
          }
        }
      }
      sa[r][q] = va;
      sb[r][q] = vb;
    }
    __syncthreads();
    // 2. row pass: column `lane` of rows wave, wave + 4, ...
    for (int r = wave; r < MT_SH; r += 4) {
      float s1 = 0.f, s2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
      for (int j = 0; j < MT_TAPS; ++j) {
        const float w = MT_G[j], a = sa[r][lane + j], v = sb[r][lane + j];
        s1 = fmaf(w, a, s1);
        s2 = fmaf(w, v, s2);
        s11 = fmaf(w, a * a, s11);
        s22 = fmaf(w, v * v, s22);
        s12 = fmaf(w, a * v, s12);
      }
      hq[0][r][lane] = s1;
      hq[1][r][lane] = s2;
      hq[2][r][lane] = s11;
      hq[3][r][lane] = s22;
      hq[4][r][lane] = s12;
    }
    __syncthreads();
    // 3. column pass: column `lane`, rows wave * MT_R .. + MT_R - 1
    float f[5][MT_R];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      float col[MT_R + MT_HALO];
#pragma unroll
      for (int i = 0; i < MT_R + MT_HALO; ++i) col[i] = hq[q][wave * MT_R + i][lane];
#pragma unroll
      for (int k = 0; k < MT_R; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < MT_TAPS; ++j) s = fmaf(MT_G[j], col[k + j], s);
        f[q][k] = s;
      }
    }
    if (x0 + lane + MT_HALO < W) {
#pragma unroll
      for (int k = 0; k < MT_R; ++k)
        if (y0 + wave * MT_R + k + MT_HALO < H) ssim_d += (double)ssim_value(f[0][k], f[1][k], f[2][k], f[3][k], f[4][k]);
    }
    __syncthreads();          // the next channel overwrites sa / sb / hq
  }

  const double sse = wave_sum(U8 ? (double)sse_u : sse_d);     // uint8: a thread's sum stays under 2^32 (<= 30 staged values x 255^2), integers in fp64 are exact
  const double ssim = wave_sum(ssim_d);
  if (lane == 0) {
    red[wave][0] = sse;
    red[wave][1] = ssim;
  }
  __syncthreads();
  if (tid < 2) part[((long long)b * g.nty * g.ntx + tile) * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void k_image_metrics_finish(const double* __restrict__ part, int ntiles, double count, double* __restrict__ out) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const double* p = part + (long long)b * ntiles * 2;
  double s0 = 0.0, s1 = 0.0;
  for (int i = tid; i < ntiles; i += 256) {
    s0 += p[2 * i];
    s1 += p[2 * i + 1];
  }
  red[0][tid] = s0;
  red[1][tid] = s1;
  __syncthreads();
  for (int n = 128; n >= 1; n >>= 1) {
    if (tid < n) {
      red[0][tid] += red[0][tid + n];
      red[1][tid] += red[1][tid + n];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[2 * b] = red[0][0];
    out[2 * b + 1] = red[1][0] / count;
  }
}

inline long long metrics_tiles(int L, int T) { return ((long long)L - MT_HALO + T - 1) / T; }

}  // namespace

#define CFEN_METRICS_MAX_EDGE 65536

static bool metrics_dims_ok(int B, int C, int H, int W) {
  return B >= 1 && B <= 65535 && (C == 1 || C == 3) && H >= MT_TAPS && W >= MT_TAPS && H <= CFEN_METRICS_MAX_EDGE && W <= CFEN_METRICS_MAX_EDGE;
}

size_t cfen_image_metrics_bytes_impl(int B, int C, int H, int W) {
  if (!metrics_dims_ok(B, C, H, W)) return 0;
  return (size_t)B * (size_t)(metrics_tiles(H, MT_H) * metrics_tiles(W, MT_W)) * 2 * sizeof(double);
}

int cfen_image_metrics_impl(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                            hipStream_t s) {
  CFEN_CHECK_ARG(a && b && scratch && out, "image_metrics: null pointer");
  CFEN_CHECK_ARG(u8 == 0 || u8 == 1, "image_metrics: u8 must be 0 ((B,C,H,W) fp32) or 1 ((B,H,W,3) uint8)");
  CFEN_CHECK_ARG(C == 1 || C == 3, "image_metrics: C = %d, must be 1 or 3", C);
  CFEN_CHECK_ARG(!u8 || C == 3, "image_metrics: uint8 images are (B,H,W,3), got C = %d", C);
  CFEN_CHECK_ARG(H >= MT_TAPS && W >= MT_TAPS, "image_metrics: a %d x %d image is smaller than the 11 x 11 SSIM window", H, W);
  CFEN_CHECK_ARG(H <= CFEN_METRICS_MAX_EDGE && W <= CFEN_METRICS_MAX_EDGE, "image_metrics: image size %d x %d over %d", H, W, CFEN_METRICS_MAX_EDGE);
  CFEN_CHECK_ARG(B >= 1 && B <= 65535, "image_metrics: batch %d outside 1 .. 65535", B);
  CFEN_CHECK_ARG(u8 || (hi > lo && hi - lo < 3.0e38f), "image_metrics: the value range (lo, hi) = (%g, %g) is empty or not finite", (double)lo, (double)hi);
  CFEN_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0,
                 "image_metrics: out and scratch must be 8-byte aligned (doubles)");
  CFEN_CHECK_ARG(u8 || ((reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(b) & 3) == 0), "image_metrics: fp32 images must be 4-byte aligned");
  const int nty = (int)metrics_tiles(H, MT_H), ntx = (int)metrics_tiles(W, MT_W);
  const MetricsGeom g = {C, H, W, nty, ntx, u8 ? 0.f : lo, u8 ? 1.f : hi - lo};
  const dim3 grid((unsigned)(nty * ntx), (unsigned)B);
  if (u8)
    CFEN_LAUNCH(k_image_metrics<true>, grid, dim3(256), 0, s, a, b, g, (double*)scratch);
  else
    CFEN_LAUNCH(k_image_metrics<false>, grid, dim3(256), 0, s, a, b, g, (double*)scratch);
  CFEN_CHECK_LAUNCH("image_metrics");
  CFEN_LAUNCH(k_image_metrics_finish, dim3((unsigned)B), dim3(256), 0, s, (const double*)scratch, nty * ntx,
              (double)C * (double)(H - MT_HALO) * (double)(W - MT_HALO), out);
  CFEN_CHECK_LAUNCH("image_metrics_finish");
  return CFEN_OK;
}
