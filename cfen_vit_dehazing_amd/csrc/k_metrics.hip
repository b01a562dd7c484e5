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
//                       2. row pass (ssim_row_pass of cfen_image.hpp, shared with k_planes.hip): the 11-tap filter along x over a, b, a^2, b^2, ab -> five (34 x 64) planes in LDS; a wave reads 64 consecutive
//                          floats per tap (conflict-free);
//                       3. column pass (ssim_col_pass): a thread owns one column and 6 consecutive rows, reads the 16 row-filtered values under them once per plane
//                          and forms 6 SSIM map values.
//                     Per-thread sums are fp64 (the squared error of uint8 input is summed in integers first: exact), reduced over the wave with
//                     shuffles, over the 4 waves through LDS in wave order, and written as this tile's (sse, ssim sum) pair to `part`.
//   k_image_metrics_finish : one workgroup per image adds the tiles' pairs in the fixed order of img_reduce_partials (cfen_image.hpp) and writes
//                     out[b] = (sse, ssim sum / count).
// No atomics and no counters: the same inputs give the same bits on every run, on any stream, at any batch size.
//
// MS-SSIM (cfen_image_msssim) runs the same tile body once per pyramid level, five launches and one finish:
//   k_msssim_level : the tile body with a second fp64 sum, cs = (2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2), beside the SSIM sum.  A tile's origin is
//                     even in both axes, so after staging a channel the workgroup also owns the 2 x 2 blocks under [y0, y0 + 24) x [x0, x0 + 64) (the
//                     last tile row / column up to the pooled image's edge): it writes their means, (a + b + c + d) * 0.25f in fp32, for both images
//                     into the next level's planar fp32 plane of the caller's workspace -- every pooled pixel exactly once, no pooling pass of its
//                     own.  Level 0 reads the caller's images (and sums the squared error as above), levels 1 .. 4 read the workspace.
//   k_msssim_finish : one workgroup per (level, image) adds that level's per-tile (sse, ssim sum, cs sum) in the order of k_image_metrics_finish.
// Level 0 runs the very instructions of k_image_metrics on the same tiles, so its (sse, ssim) come out bit for bit the same.
#include "cfen_image.hpp"

namespace {

struct MetricsGeom {
  int C, H, W, nty, ntx;
  float lo, range;      // fp32 input: v -> (v - lo) / range
};

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

// the same value and, for MS-SSIM, its contrast-structure factor cs = v1 / v2 (1 exactly for a == b: 2 s against s + s)
CFEN_DEV float ssim_cs_value(float mu1, float mu2, float e11, float e22, float e12, float& cs) {
#pragma clang fp contract(off)
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
  const float v1 = 2.0f * sigma12 + C2, v2 = sigma1_sq + sigma2_sq + C2;
  cs = v1 / v2;
  return ((2.0f * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2);
}

// where a level's 2 x 2 means go (MS-SSIM): planar fp32 (B,C,Hn,Wn) for both images; a == nullptr at the last level
struct MetricsPool {
  float *a, *b;
  int Hn, Wn;
};

enum { MT_SRC_U8 = 0, MT_SRC_F32 = 1, MT_SRC_PLANAR01 = 2 };      // (B,H,W,3) bytes; (B,C,H,W) fp32 mapped by (lo, range); (B,C,H,W) fp32 already on [0,1]

// One tile of one image pair.  MS = false: writes (sse, ssim sum) to part -- k_image_metrics.  MS = true: (sse, ssim sum, cs sum), and the pooled block.
template <int SRC, bool MS>
CFEN_DEV void metrics_tile(const void* __restrict__ pa, const void* __restrict__ pb, const MetricsGeom& g, double* __restrict__ part,
                           const MetricsPool& pool) {
  constexpr bool U8 = SRC == MT_SRC_U8;
  constexpr int NP = MS ? 3 : 2;
  __shared__ float sa[MT_SH][MT_SW], sb[MT_SH][MT_SW];
  __shared__ float hq[5][MT_SH][MT_W];
  __shared__ double red[4][NP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, b = blockIdx.y;
  const int ty = tile / g.ntx, tx = tile - ty * g.ntx;
  const int y0 = ty * MT_H, x0 = tx * MT_W;
  const int H = g.H, W = g.W;
  // pixels this tile owns for the squared error
  const int own_y1 = ty == g.nty - 1 ? H : y0 + MT_H, own_x1 = tx == g.ntx - 1 ? W : x0 + MT_W;
  const long long plane = (long long)H * W;
  unsigned sse_u = 0;
  double sse_d = 0.0, ssim_d = 0.0, cs_d = 0.0;

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
        } else if (SRC == MT_SRC_PLANAR01) {
          const long long o = ((long long)b * g.C + c) * plane + (long long)y * W + x;
          va = static_cast<const float*>(pa)[o];
          vb = static_cast<const float*>(pb)[o];
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
    if (MS && pool.a) {
      // the 2 x 2 means this tile owns, rows [y0 / 2, ..) x columns [x0 / 2, ..) of the next level: 12 x 32, the last tile row / column up to the
      // pooled edge (at most 17 x 37: the staged 34 x 74 pixels reach the image's edge there)
      const int py0 = y0 >> 1, px0 = x0 >> 1;
      const int ph = (ty == g.nty - 1 ? pool.Hn : py0 + MT_H / 2) - py0, pw = (tx == g.ntx - 1 ? pool.Wn : px0 + MT_W / 2) - px0;
      const long long base = ((long long)b * g.C + c) * ((long long)pool.Hn * pool.Wn);
      for (int i = tid; i < ph * pw; i += 256) {
        const int r = i / pw, q = i - r * pw;
        const long long o = base + (long long)(py0 + r) * pool.Wn + (px0 + q);
        pool.a[o] = (((sa[2 * r][2 * q] + sa[2 * r][2 * q + 1]) + sa[2 * r + 1][2 * q]) + sa[2 * r + 1][2 * q + 1]) * 0.25f;
        pool.b[o] = (((sb[2 * r][2 * q] + sb[2 * r][2 * q + 1]) + sb[2 * r + 1][2 * q]) + sb[2 * r + 1][2 * q + 1]) * 0.25f;
      }
    }
    // 2. row pass, 3. column pass (cfen_image.hpp)
    ssim_row_pass(sa, sb, hq, wave, lane);
    __syncthreads();
    float f[5][MT_R];
    ssim_col_pass(hq, wave, lane, f);
    if (x0 + lane + MT_HALO < W) {
#pragma unroll
      for (int k = 0; k < MT_R; ++k)
        if (y0 + wave * MT_R + k + MT_HALO < H) {
          if (MS) {
            float cs;
            ssim_d += (double)ssim_cs_value(f[0][k], f[1][k], f[2][k], f[3][k], f[4][k], cs);
            cs_d += (double)cs;
          } else {
            ssim_d += (double)ssim_value(f[0][k], f[1][k], f[2][k], f[3][k], f[4][k]);
          }
        }
    }
    __syncthreads();          // the next channel overwrites sa / sb / hq
  }

  const double sse = wave_sum(U8 ? (double)sse_u : sse_d);     // uint8: a thread's sum stays under 2^32 (<= 30 staged values x 255^2), integers in fp64 are exact
  const double ssim = wave_sum(ssim_d);
  const double cs = MS ? wave_sum(cs_d) : 0.0;
  if (lane == 0) {
    red[wave][0] = sse;
    red[wave][1] = ssim;
    if (MS) red[wave][NP - 1] = cs;
  }
  __syncthreads();
  if (tid < NP) part[((long long)b * g.nty * g.ntx + tile) * NP + tid] = block4_sum(&red[0][tid], NP);
}

template <bool U8>
__global__ __launch_bounds__(256) void k_image_metrics(const void* __restrict__ pa, const void* __restrict__ pb, MetricsGeom g,
                                                       double* __restrict__ part) {
  metrics_tile<U8 ? MT_SRC_U8 : MT_SRC_F32, false>(pa, pb, g, part, MetricsPool{nullptr, nullptr, 0, 0});
}

template <int SRC>
__global__ __launch_bounds__(256) void k_msssim_level(const void* __restrict__ pa, const void* __restrict__ pb, MetricsGeom g,
                                                      double* __restrict__ part, MetricsPool pool) {
  metrics_tile<SRC, true>(pa, pb, g, part, pool);
}

__global__ __launch_bounds__(256) void k_image_metrics_finish(const double* __restrict__ part, int ntiles, double count, double* __restrict__ out) {
  __shared__ double red[2][256];
  const int b = blockIdx.x;
  img_reduce_partials<2>(part + (long long)b * ntiles * 2, ntiles, red);
  if (threadIdx.x == 0) {
    out[2 * b] = red[0][0];
    out[2 * b + 1] = red[1][0] / count;
  }
}

constexpr int MS_LEVELS = 5, MS_MIN_EDGE = MT_TAPS << (MS_LEVELS - 1);      // level 4 must still hold one window: 176

struct MsFinish {
  long long off[MS_LEVELS];      // level l's partials start at part + off[l]: [B][ntiles[l]][3] doubles
  int ntiles[MS_LEVELS];
  double count[MS_LEVELS];       // window positions of level l over all channels
};

// workgroup (l, b): out[b] = (sse, ssim_0, cs_0, ..., ssim_4, cs_4), the sums of level l in the order of k_image_metrics_finish
__global__ __launch_bounds__(256) void k_msssim_finish(const double* __restrict__ part, MsFinish f, double* __restrict__ out) {
  __shared__ double red[3][256];
  const int l = blockIdx.x, b = blockIdx.y;
  const int ntiles = f.ntiles[l];
  img_reduce_partials<3>(part + f.off[l] + (long long)b * ntiles * 3, ntiles, red);
  if (threadIdx.x == 0) {
    double* o = out + (long long)b * (1 + 2 * MS_LEVELS);
    if (l == 0) o[0] = red[0][0];
    o[1 + 2 * l] = red[1][0] / f.count[l];
    o[2 + 2 * l] = red[2][0] / f.count[l];
  }
}

// the pyramid's geometry and the layout of the scratch: every level's partials first (doubles), then levels 1 .. 4 of image a and of image b (floats)
struct MsPlan {
  int H[MS_LEVELS], W[MS_LEVELS], nty[MS_LEVELS], ntx[MS_LEVELS];
  size_t part_off[MS_LEVELS], pyr_off[MS_LEVELS];      // in doubles / in floats from the pyramid's start (pyr_off[0] unused); image b follows image a
  size_t part_doubles, bytes;
};

inline MsPlan msssim_plan(int B, int C, int H, int W) {
  MsPlan p = {};
  size_t doubles = 0, floats = 0;
  for (int l = 0; l < MS_LEVELS; ++l) {
    p.H[l] = l ? p.H[l - 1] / 2 : H;
    p.W[l] = l ? p.W[l - 1] / 2 : W;
    p.nty[l] = (int)metrics_tiles(p.H[l], MT_H);
    p.ntx[l] = (int)metrics_tiles(p.W[l], MT_W);
    p.part_off[l] = doubles;
    doubles += (size_t)B * (size_t)p.nty[l] * (size_t)p.ntx[l] * 3;
    p.pyr_off[l] = floats;
    if (l) floats += 2 * (size_t)B * (size_t)C * (size_t)p.H[l] * (size_t)p.W[l];
  }
  p.part_doubles = doubles;
  p.bytes = (doubles * sizeof(double) + floats * sizeof(float) + 15) / 16 * 16;
  return p;
}

}  // namespace

#define CFEN_METRICS_MAX_EDGE 65536

static bool metrics_dims_ok(int B, int C, int H, int W) {
  return B >= 1 && B <= 65535 && (C == 1 || C == 3) && H >= MT_TAPS && W >= MT_TAPS && H <= CFEN_METRICS_MAX_EDGE && W <= CFEN_METRICS_MAX_EDGE;
}

size_t cfen_image_metrics_bytes_impl(int B, int C, int H, int W) {
  if (!metrics_dims_ok(B, C, H, W)) return 0;
  return (size_t)B * (size_t)(metrics_tiles(H, MT_H) * metrics_tiles(W, MT_W)) * 2 * sizeof(double);
}

// the argument checks of both entry points; `name` is the entry point's and min_edge the smallest image edge it takes
static int metrics_check_args(const char* name, int min_edge, int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi,
                              const void* scratch, const double* out) {
  CFEN_CHECK_ARG(a && b && scratch && out, "%s: null pointer", name);
  CFEN_CHECK_ARG(u8 == 0 || u8 == 1, "%s: u8 must be 0 ((B,C,H,W) fp32) or 1 ((B,H,W,3) uint8)", name);
  CFEN_CHECK_ARG(C == 1 || C == 3, "%s: C = %d, must be 1 or 3", name, C);
  CFEN_CHECK_ARG(!u8 || C == 3, "%s: uint8 images are (B,H,W,3), got C = %d", name, C);
  if (min_edge == MT_TAPS)
    CFEN_CHECK_ARG(H >= min_edge && W >= min_edge, "%s: a %d x %d image is smaller than the 11 x 11 SSIM window", name, H, W);
  else
    CFEN_CHECK_ARG(H >= min_edge && W >= min_edge,
                   "%s: a %d x %d image is under %d pixels on a side: the fifth level would be smaller than the 11 x 11 SSIM window", name, H, W, min_edge);
  CFEN_CHECK_ARG(H <= CFEN_METRICS_MAX_EDGE && W <= CFEN_METRICS_MAX_EDGE, "%s: image size %d x %d over %d", name, H, W, CFEN_METRICS_MAX_EDGE);
  CFEN_CHECK_ARG(B >= 1 && B <= 65535, "%s: batch %d outside 1 .. 65535", name, B);
  CFEN_CHECK_ARG(u8 || (hi > lo && hi - lo < 3.0e38f), "%s: the value range (lo, hi) = (%g, %g) is empty or not finite", name, (double)lo, (double)hi);
  CFEN_CHECK_ARG(cfen_aligned(out, 8) && cfen_aligned(scratch, 8), "%s: out and scratch must be 8-byte aligned (doubles)", name);
  CFEN_CHECK_ARG(u8 || (cfen_aligned(a, 4) && cfen_aligned(b, 4)), "%s: fp32 images must be 4-byte aligned", name);
  return CFEN_OK;
}

int cfen_image_metrics_impl(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                            hipStream_t s) {
  if (const int e = metrics_check_args("image_metrics", MT_TAPS, u8, a, b, B, C, H, W, lo, hi, scratch, out)) return e;
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

static bool msssim_dims_ok(int B, int C, int H, int W) { return metrics_dims_ok(B, C, H, W) && H >= MS_MIN_EDGE && W >= MS_MIN_EDGE; }

size_t cfen_image_msssim_bytes_impl(int B, int C, int H, int W) {
  if (!msssim_dims_ok(B, C, H, W)) return 0;
  return msssim_plan(B, C, H, W).bytes;
}

int cfen_image_msssim_impl(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                           hipStream_t s) {
  if (const int e = metrics_check_args("image_msssim", MS_MIN_EDGE, u8, a, b, B, C, H, W, lo, hi, scratch, out)) return e;
  const MsPlan p = msssim_plan(B, C, H, W);
  double* part = (double*)scratch;
  float* pyr = (float*)(part + p.part_doubles);
  MsFinish f;
  const void *src_a = a, *src_b = b;
  for (int l = 0; l < MS_LEVELS; ++l) {
    const MetricsGeom g = {C, p.H[l], p.W[l], p.nty[l], p.ntx[l], (u8 || l) ? 0.f : lo, (u8 || l) ? 1.f : hi - lo};
    MetricsPool pool = {nullptr, nullptr, 0, 0};
    if (l + 1 < MS_LEVELS) {
      const size_t n = (size_t)B * (size_t)C * (size_t)p.H[l + 1] * (size_t)p.W[l + 1];
      pool = MetricsPool{pyr + p.pyr_off[l + 1], pyr + p.pyr_off[l + 1] + n, p.H[l + 1], p.W[l + 1]};
    }
    const dim3 grid((unsigned)(p.nty[l] * p.ntx[l]), (unsigned)B);
    if (l)
      CFEN_LAUNCH(k_msssim_level<MT_SRC_PLANAR01>, grid, dim3(256), 0, s, src_a, src_b, g, part + p.part_off[l], pool);
    else if (u8)
      CFEN_LAUNCH(k_msssim_level<MT_SRC_U8>, grid, dim3(256), 0, s, src_a, src_b, g, part + p.part_off[l], pool);
    else
      CFEN_LAUNCH(k_msssim_level<MT_SRC_F32>, grid, dim3(256), 0, s, src_a, src_b, g, part + p.part_off[l], pool);
    CFEN_CHECK_LAUNCH("image_msssim");
    src_a = pool.a;
    src_b = pool.b;
    f.off[l] = (long long)p.part_off[l];
    f.ntiles[l] = p.nty[l] * p.ntx[l];
    f.count[l] = (double)C * (double)(p.H[l] - MT_HALO) * (double)(p.W[l] - MT_HALO);
  }
  CFEN_LAUNCH(k_msssim_finish, dim3(MS_LEVELS, (unsigned)B), dim3(256), 0, s, (const double*)part, f, out);
  CFEN_CHECK_LAUNCH("image_msssim_finish");
  return CFEN_OK;
}
