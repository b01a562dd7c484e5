// Full-reference scores of a YCbCr stream against a ground-truth stream, plane by plane on the stored samples (include/cfen_planes.h states the
// definition and the contract; tests/planes_ref.py restates it in numpy).  Scored under dehaze_video.py --eval_gt (gtscore.Scorer,
// ops.plane_metrics) on the payload bytes that leave, after rgb_to_yuv_u8 / rgb_f32_to_yuv16.
//
//   k_plane_metrics        : grid (tiles, plane, B).  A workgroup (256 threads) owns MT_H x MT_W = 24 x 64 window positions of one plane of one
//                            frame pair: the tile of k_image_metrics (cfen_image.hpp) on one channel.  It
//                              1. stages the 34 x 74 samples under those windows of both frames in LDS as (float)v / (float)top - 0.5 (zeros past the
//                                 plane), and adds, for the samples the tile OWNS ([y0, y0 + 24) x [x0, x0 + 64), the last tile row / column up to the
//                                 plane's edge), (a - b)^2 and |(a - a_prev) - (b - b_prev)| in 64-bit integers: every sample exactly once;
//                              2. 3. runs the row and the column pass of cfen_image.hpp and sums its SSIM map values (pl_ssim_value) in fp64.
//                            The sums go lane butterfly -> four waves in wave order -> one (ssim sum, SSE, DT) per tile in scratch.  A workgroup
//                            past its plane's last tile (the chroma planes have fewer tiles than the luma plane) leaves at once.
//   k_plane_metrics_finish : grid (3, B).  One workgroup per plane adds the tiles' SSIM sums in the order of img_reduce_partials, the integers in
//                            uint64, and writes the plane's four words; a plane the format does not have gets (0, 0, NaN, 0).
// Two launches; no global atomics, no counters.  Samples are read one by one: consecutive lanes read consecutive samples of a staged row.
#include "../../include/cfen_planes.h"
#include "cfen_image.hpp"

namespace {

struct PlGeom {
  int h[3], w[3];               // the planes' sizes; 0 x 0 for a plane the format does not have
  int nty[3], ntx[3];           // tiles per plane edge
  long long off[3];             // byte offset of the plane inside a frame
  int tile0[3];                 // the plane's first tile among the frame's
  int frame_tiles, nplanes, top;
};

typedef unsigned long long pl_u64;

template <bool DEEP>
CFEN_DEV int pl_load(const unsigned char* p, long long i, int top) {
  if (DEEP) return min((int)reinterpret_cast<const unsigned short*>(p)[i], top);
  return (int)p[i];
}

// Samples are staged CENTRED, x - 0.5: variances and the covariance do not change under a shift, and e - mu^2 then cancels at |mu| <= 0.5 where
// the typical mu is near 0; the luminance term takes mu + 0.5 back.  On a plane of ONE window, where nothing averages the map's rounding out, this
// brings the distance from float64 from 6e-6 down to under 2e-6 (tests/test_hip_plane_metrics.py).  No FMA contraction, as in ssim_value of
// k_metrics.hip: with a == b the numerator and the denominator come out bitwise equal, so identical planes score exactly 1.
constexpr float PL_CENTRE = 0.5f;

CFEN_DEV float pl_ssim_value(float m1, float m2, float e11, float e22, float e12) {
#pragma clang fp contract(off)
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float sigma1_sq = e11 - m1 * m1, sigma2_sq = e22 - m2 * m2, sigma12 = e12 - m1 * m2;
  const float mu1 = m1 + PL_CENTRE, mu2 = m2 + PL_CENTRE;
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float v1 = 2.0f * sigma12 + C2, v2 = sigma1_sq + sigma2_sq + C2;
  return ((2.0f * mu1_mu2 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2);
}

// where the partials of plane `plane` of frame k start, in 8-byte words: n doubles (ssim sums), then n pairs (SSE, DT)
CFEN_DEV long long pl_segment(const PlGeom& g, int k, int plane) { return ((long long)k * g.frame_tiles + g.tile0[plane]) * 3; }

template <bool DEEP>
__global__ __launch_bounds__(256) void k_plane_metrics(const unsigned char* a, size_t stride_a, const unsigned char* b, size_t stride_b,
                                                       const unsigned char* a_prev, const unsigned char* b_prev, PlGeom g,
                                                       pl_u64* __restrict__ part) {
  __shared__ float sa[MT_SH][MT_SW], sb[MT_SH][MT_SW];
  __shared__ float hq[5][MT_SH][MT_W];
  __shared__ double red_d[4];
  __shared__ pl_u64 red_u[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, plane = blockIdx.y, k = blockIdx.z;
  const int H = g.h[plane], W = g.w[plane], nty = g.nty[plane], ntx = g.ntx[plane];
  if (tile >= nty * ntx) return;                                              // block-uniform
  const int ty = tile / ntx, tx = tile - ty * ntx;
  const int y0 = ty * MT_H, x0 = tx * MT_W;
  const int own_y1 = ty == nty - 1 ? H : y0 + MT_H, own_x1 = tx == ntx - 1 ? W : x0 + MT_W;
  const unsigned char* pa = a + (size_t)k * stride_a + g.off[plane];
  const unsigned char* pb = b + (size_t)k * stride_b + g.off[plane];
  const unsigned char* qa = k ? pa - stride_a : (a_prev ? a_prev + g.off[plane] : nullptr);
  const unsigned char* qb = k ? pb - stride_b : (b_prev ? b_prev + g.off[plane] : nullptr);
  const float ftop = (float)g.top;
  pl_u64 sse = 0, dt = 0;
  double ssim_d = 0.0;

  // 1. stage
  for (int i = tid; i < MT_SH * MT_SW; i += 256) {
    const int r = i / MT_SW, q = i - r * MT_SW;
    const int y = y0 + r, x = x0 + q;
    float va = 0.f, vb = 0.f;
    if (y < H && x < W) {
      const long long o = (long long)y * W + x;
      const int ia = pl_load<DEEP>(pa, o, g.top), ib = pl_load<DEEP>(pb, o, g.top);
      va = __fdiv_rn((float)ia, ftop) - PL_CENTRE;
      vb = __fdiv_rn((float)ib, ftop) - PL_CENTRE;
      if (y < own_y1 && x < own_x1) {
        const unsigned d = (unsigned)abs(ia - ib);                             // <= 65535: d * d < 2^32
        sse += (pl_u64)(d * d);
        if (qa != nullptr) dt += (pl_u64)abs((ia - pl_load<DEEP>(qa, o, g.top)) - (ib - pl_load<DEEP>(qb, o, g.top)));
      }
    }
    sa[r][q] = va;
    sb[r][q] = vb;
  }
  __syncthreads();
  // 2. row pass, 3. column pass (cfen_image.hpp)
  ssim_row_pass(sa, sb, hq, wave, lane);
  __syncthreads();
  float f[5][MT_R];
  ssim_col_pass(hq, wave, lane, f);
  if (x0 + lane + MT_HALO < W) {
#pragma unroll
    for (int j = 0; j < MT_R; ++j)
      if (y0 + wave * MT_R + j + MT_HALO < H) ssim_d += (double)pl_ssim_value(f[0][j], f[1][j], f[2][j], f[3][j], f[4][j]);
  }

  sse = wave_sum(sse);
  dt = wave_sum(dt);
  ssim_d = wave_sum(ssim_d);
  if (lane == 0) {
    red_d[wave] = ssim_d;
    red_u[wave][0] = sse;
    red_u[wave][1] = dt;
  }
  __syncthreads();
  if (tid == 0) {
    pl_u64* seg = part + pl_segment(g, k, plane);
    const int n = nty * ntx;
    seg[tile] = (pl_u64)__double_as_longlong(block4_sum(red_d, 1));
    seg[n + 2 * tile] = ((red_u[0][0] + red_u[1][0]) + red_u[2][0]) + red_u[3][0];
    seg[n + 2 * tile + 1] = ((red_u[0][1] + red_u[1][1]) + red_u[2][1]) + red_u[3][1];
  }
}

__global__ __launch_bounds__(256) void k_plane_metrics_finish(const pl_u64* __restrict__ part, PlGeom g, pl_u64* __restrict__ out) {
  __shared__ double red[1][256];
  __shared__ pl_u64 red_u[4][2];
  const int tid = threadIdx.x, plane = blockIdx.x, k = blockIdx.y;
  pl_u64* o = out + ((long long)k * 3 + plane) * 4;
  const pl_u64 nan_bits = 0x7ff8000000000000ull;
  if (plane >= g.nplanes) {                                                    // block-uniform
    if (tid < 4) o[tid] = tid == 2 ? nan_bits : 0ull;
    return;
  }
  const int H = g.h[plane], W = g.w[plane], n = g.nty[plane] * g.ntx[plane];
  const pl_u64* seg = part + pl_segment(g, k, plane);
  img_reduce_partials<1>(reinterpret_cast<const double*>(seg), n, red);
  pl_u64 sse = 0, dt = 0;
  for (int i = tid; i < n; i += 256) {
    sse += seg[n + 2 * i];
    dt += seg[n + 2 * i + 1];
  }
  sse = wave_sum(sse);
  dt = wave_sum(dt);
  if ((tid & 63) == 0) {
    red_u[tid >> 6][0] = sse;
    red_u[tid >> 6][1] = dt;
  }
  __syncthreads();
  if (tid == 0) {
    o[0] = ((red_u[0][0] + red_u[1][0]) + red_u[2][0]) + red_u[3][0];
    o[1] = ((red_u[0][1] + red_u[1][1]) + red_u[2][1]) + red_u[3][1];
    o[2] = (H >= MT_TAPS && W >= MT_TAPS) ? (pl_u64)__double_as_longlong(red[0][0] / ((double)(H - MT_HALO) * (double)(W - MT_HALO))) : nan_bits;
    o[3] = (pl_u64)H * (pl_u64)W;
  }
}

bool pl_dims_ok(int B, int H, int W, int chroma) {
  return B >= 1 && B <= CFEN_YUV_MAX_BATCH && H >= 1 && W >= 1 && H <= CFEN_YUV_MAX_EDGE && W <= CFEN_YUV_MAX_EDGE &&
         (long long)H * W <= (1ll << 31) && chroma >= CFEN_YUV_420JPEG && chroma <= CFEN_YUV_MONO;
}

int pl_tiles(int L, int T) { return (int)(L > MT_HALO ? metrics_tiles(L, T) : 1); }      // a plane too small for a window still has one tile

// the planes of H x W frames of `chroma` (pl_dims_ok holds), `esz` bytes per sample
PlGeom pl_geom(int H, int W, int chroma, int depth) {
  PlGeom g = {};
  const int esz = depth > 8 ? 2 : 1;
  const int Wc = chroma == CFEN_YUV_444 ? W : (W + 1) >> 1, Hc = chroma <= CFEN_YUV_420MPEG2 ? (H + 1) >> 1 : H;
  g.nplanes = chroma == CFEN_YUV_MONO ? 1 : 3;
  g.top = (1 << depth) - 1;
  for (int p = 0; p < g.nplanes; ++p) {
    g.h[p] = p ? Hc : H;
    g.w[p] = p ? Wc : W;
    g.nty[p] = pl_tiles(g.h[p], MT_H);
    g.ntx[p] = pl_tiles(g.w[p], MT_W);
    g.off[p] = p ? ((long long)H * W + (long long)(p - 1) * Hc * Wc) * esz : 0;
    g.tile0[p] = g.frame_tiles;
    g.frame_tiles += g.nty[p] * g.ntx[p];                                      // <= 3 * 2^31 / (24 * 64) + edges: far inside an int
  }
  return g;
}

long long pl_frame_bytes(const PlGeom& g, int depth) {
  long long n = 0;
  for (int p = 0; p < g.nplanes; ++p) n += (long long)g.h[p] * g.w[p];
  return n * (depth > 8 ? 2 : 1);
}

}  // namespace

extern "C" size_t cfen_plane_metrics_bytes(int B, int H, int W, int chroma) {
  if (!pl_dims_ok(B, H, W, chroma)) return 0;
  return (size_t)B * (size_t)pl_geom(H, W, chroma, 8).frame_tiles * 3 * sizeof(pl_u64);
}

extern "C" int cfen_plane_metrics(const void* a, size_t stride_a, const void* b, size_t stride_b, const void* a_prev, const void* b_prev, int B,
                                  int H, int W, int chroma, int depth, void* scratch, void* out, void* stream) {
  CFEN_CHECK_ARG(a && b && scratch && out, "plane_metrics: null pointer (a, b, scratch and out are all required)");
  CFEN_CHECK_ARG((a_prev == nullptr) == (b_prev == nullptr), "plane_metrics: a_prev and b_prev must both be NULL or both be set");
  CFEN_CHECK_ARG(B >= 1 && B <= CFEN_YUV_MAX_BATCH, "plane_metrics: B = %d outside 1 .. %d", B, CFEN_YUV_MAX_BATCH);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= CFEN_YUV_MAX_EDGE && W <= CFEN_YUV_MAX_EDGE, "plane_metrics: sizes H = %d, W = %d outside 1 .. %d", H, W,
                 CFEN_YUV_MAX_EDGE);
  CFEN_CHECK_ARG((long long)H * W <= (1ll << 31), "plane_metrics: H W = %lld samples over 2^31 (the 64-bit SSE could overflow at 16 bits)",
                 (long long)H * W);
  CFEN_CHECK_ARG(chroma >= CFEN_YUV_420JPEG && chroma <= CFEN_YUV_MONO, "plane_metrics: unknown chroma format %d", chroma);
  CFEN_CHECK_ARG(depth >= CFEN_PLANES_MIN_DEPTH && depth <= CFEN_PLANES_MAX_DEPTH, "plane_metrics: depth = %d outside %d .. %d", depth,
                 CFEN_PLANES_MIN_DEPTH, CFEN_PLANES_MAX_DEPTH);
  const PlGeom g = pl_geom(H, W, chroma, depth);
  const long long nb = pl_frame_bytes(g, depth);
  CFEN_CHECK_ARG(stride_a >= (size_t)nb && stride_b >= (size_t)nb, "plane_metrics: stride_a = %zu or stride_b = %zu is below the frame size %lld",
                 stride_a, stride_b, nb);
  if (depth > 8)
    CFEN_CHECK_ARG(cfen_aligned(a, 2) && cfen_aligned(b, 2) && cfen_aligned(a_prev, 2) && cfen_aligned(b_prev, 2) && stride_a % 2 == 0 &&
                       stride_b % 2 == 0,
                   "plane_metrics: at depth %d the samples are 16-bit words: an odd pointer or stride", depth);
  CFEN_CHECK_ARG(cfen_aligned(out, 8) && cfen_aligned(scratch, 8), "plane_metrics: out and scratch must be 8-byte aligned (64-bit words)");
  int ntiles = 0;
  for (int p = 0; p < g.nplanes; ++p) ntiles = g.nty[p] * g.ntx[p] > ntiles ? g.nty[p] * g.ntx[p] : ntiles;
  hipStream_t s = (hipStream_t)stream;
  const unsigned char *pa = (const unsigned char*)a, *pb = (const unsigned char*)b, *qa = (const unsigned char*)a_prev,
                      *qb = (const unsigned char*)b_prev;
  const dim3 grid((unsigned)ntiles, (unsigned)g.nplanes, (unsigned)B);
  if (depth > 8)
    CFEN_LAUNCH(k_plane_metrics<true>, grid, dim3(256), 0, s, pa, stride_a, pb, stride_b, qa, qb, g, (pl_u64*)scratch);
  else
    CFEN_LAUNCH(k_plane_metrics<false>, grid, dim3(256), 0, s, pa, stride_a, pb, stride_b, qa, qb, g, (pl_u64*)scratch);
  CFEN_CHECK_LAUNCH("plane_metrics");
  CFEN_LAUNCH(k_plane_metrics_finish, dim3(3, (unsigned)B), dim3(256), 0, s, (const pl_u64*)scratch, g, (pl_u64*)out);
  CFEN_CHECK_LAUNCH("plane_metrics (finish)");
  return CFEN_OK;
}
