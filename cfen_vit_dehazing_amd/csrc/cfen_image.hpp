// What the image-side kernels share (k_guided, k_temporal, k_metrics, k_planes, k_colordiff, k_noref, k_png): window and source coordinates,
// the rounding to a byte, the full-resolution apply kernel of k_guided / k_temporal with its launch, the fixed-order fp64 reductions the
// scores are built from, and the SSIM tile (window, row and column pass) of k_metrics / k_planes.  Each argument below is made here once; the .hip files state only what is their own.
#pragma once
#include <math.h>

#include "cfen_common.hpp"

// ---- coordinates and rounding -----------------------------------------------------------------------------------------------------------
// pixels of the window around `p` (radius r) that lie inside [0, n)
CFEN_DEV int img_window_count(int p, int r, int n) { return min(p + r, n - 1) - max(p - r, 0) + 1; }

// source coordinate of output index i on an axis in -> out: ((2i+1) in - out) / (2 out), clamped below at 0, in integers
CFEN_DEV void img_src_coord(int i, int in, int out, int& i0, int& i1, float& f) {
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

// round half up to a byte.  The clamp is on the FLOAT, and callers put the four bytes of a dword together with shifts and ors: a
// shift-then-clamp of int32 pairs may become gfx950's v_ashr_pk_u8_i32, which gave wrong bytes on the device (a variant of k_resample_v, and
// k_yuv's yv_dot: DESIGN sections 13 and 17; build.check_no_ashr_pk_u8 counts the instruction).  The caller forms `v` itself, so that the
// association of its sum is written where the sum is.
CFEN_DEV unsigned img_round_byte(float v) {
  v = floorf(v + 0.5f);
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (unsigned)(int)v;
}

// ---- the apply kernel: dst = round(A g + B), or round((y + A g) + B) with ADD_SRC, A and B upsampled bilinearly from `field` ----------------
// The kernel that sees the full-resolution image.  field: (B, h, w, 6) fp32, A in 0..2 and B in 3..5; guide, src and dst: (B, H, W, 3) bytes.
// A workgroup of 4 waves takes IMG_RUN bytes of one output row (a wave 1 KiB, a lane 16 consecutive bytes), so y0, y1 and fy are block-uniform.
//   (1) the field columns the run covers, [x0 of its first pixel, x1 of its last], are interpolated vertically into LDS (IMG_COLS columns at
//       most; a run that covers more -- a downward or near-1:1 horizontal ratio -- reads both rows from global memory per pixel instead: a
//       block-uniform choice, the same arithmetic);
//   (2) one thread per pixel does the horizontal lerp and leaves A and B per output BYTE in LDS;
//   (3) a lane reads its 16 guide (and src) bytes (the loads are issued before (1)), 16 + 16 coefficients as four + four 16-byte LDS reads, and
//       stores 16 bytes (V = 16) -- or single bytes when 3 W or a pointer is not a multiple of 16 (V = 1); the last lane of a row may then own
//       fewer than 16 bytes.
// ADD_SRC is a compile-time switch: without it `src` is never read and no second row is held.  No atomics, no counters, no scratch.
constexpr int IMG_RUN = 4096;                  // bytes of one output row per workgroup
constexpr int IMG_COLS = 1024;                 // field columns staged at most (24 KB)

template <bool ADD_SRC>
CFEN_DEV unsigned img_affine_byte(float y, float A, float g, float B) {
  return img_round_byte(ADD_SRC ? (y + A * g) + B : A * g + B);
}

template <int V, bool ADD_SRC>
CFEN_DEV void img_affine_apply(const float* __restrict__ field, const unsigned char* __restrict__ guide, const unsigned char* __restrict__ src,
                               unsigned char* __restrict__ dst, int h, int w, int H, int W, int nseg) {
  __shared__ __attribute__((aligned(16))) float sA[IMG_RUN];
  __shared__ __attribute__((aligned(16))) float sB[IMG_RUN];
  __shared__ float cv[IMG_COLS * 6];
  const int tid = threadIdx.x;
  const int row = blockIdx.x / nseg, sg = blockIdx.x - row * nseg;                          // row = b * H + y
  const int b = row / H, y = row - b * H;
  const int pitch = W * 3;
  const int byte0 = sg * IMG_RUN, off = byte0 + tid * 16;
  const unsigned char* grow = guide + (long long)row * pitch;
  const unsigned char* srow = ADD_SRC ? src + (long long)row * pitch : nullptr;
  union { uint4 q; unsigned u[4]; unsigned char c[16]; } gv, yv;
  if (V == 16) {
    if (off < pitch) {                                                                      // pitch % 16 == 0: a lane's 16 bytes are whole or absent
      gv.q = *reinterpret_cast<const uint4*>(grow + off);
      if (ADD_SRC) yv.q = *reinterpret_cast<const uint4*>(srow + off);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      gv.c[j] = off + j < pitch ? grow[off + j] : (unsigned char)0;
      if (ADD_SRC) yv.c[j] = off + j < pitch ? srow[off + j] : (unsigned char)0;
    }
  }
  int y0, y1;
  float fy;
  img_src_coord(y, h, H, y0, y1, fy);
  const int pfirst = byte0 / 3, plast = min((byte0 + IMG_RUN - 1) / 3, W - 1);
  int cfirst, clast, unused;
  float unusedf;
  img_src_coord(pfirst, w, W, cfirst, unused, unusedf);
  img_src_coord(plast, w, W, unused, clast, unusedf);
  const int ncols = clast - cfirst + 1;
  const bool staged = ncols <= IMG_COLS;                                                   // block-uniform
  const float* c0 = field + ((long long)b * h + y0) * w * 6;
  const float* c1 = field + ((long long)b * h + y1) * w * 6;
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
    img_src_coord(p, w, W, xa, xb, fx);
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
      if (idx >= 0 && idx < IMG_RUN) (k < 3 ? sA : sB)[idx] = l + fx * (r - l);
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
      const unsigned g = gv.u[d], s = ADD_SRC ? yv.u[d] : 0u;
      o.u[d] = img_affine_byte<ADD_SRC>((float)(s & 255u), A[0], (float)(g & 255u), Bv[0]) |
               (img_affine_byte<ADD_SRC>((float)((s >> 8) & 255u), A[1], (float)((g >> 8) & 255u), Bv[1]) << 8) |
               (img_affine_byte<ADD_SRC>((float)((s >> 16) & 255u), A[2], (float)((g >> 16) & 255u), Bv[2]) << 16) |
               (img_affine_byte<ADD_SRC>((float)(s >> 24), A[3], (float)(g >> 24), Bv[3]) << 24);
    }
    *reinterpret_cast<uint4*>(drow + off) = o.q;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (off + j < pitch)
        drow[off + j] = (unsigned char)img_affine_byte<ADD_SRC>(ADD_SRC ? (float)yv.c[j] : 0.f, sA[tid * 16 + j], (float)gv.c[j], sB[tid * 16 + j]);
  }
}

// Launch of the apply kernel K<V> inside a C entry point: the block-count check, nseg, and V = 16 where every byte pointer (`ptr_or` is the
// OR of their addresses) and the pitch are multiples of 16, V = 1 otherwise.  The kernel's arguments before (h, w, H, W, nseg) follow.
#define IMG_LAUNCH_APPLY(K, what, s, B, h, w, H, W, ptr_or, ...)                                                            \
  do {                                                                                                                       \
    const int pitch__ = (W) * 3, nseg__ = (pitch__ + IMG_RUN - 1) / IMG_RUN;                                                  \
    const long long blocks__ = (long long)(B) * (H) * nseg__;                                                                \
    CFEN_CHECK_ARG(blocks__ <= 0x7fffffffLL, what ": B = %d images of %d x %d are too large for one launch", B, H, W);        \
    if (((ptr_or) | (uintptr_t)pitch__) % 16 == 0)                                                                           \
      CFEN_LAUNCH(K<16>, dim3((unsigned)blocks__), dim3(256), 0, s, __VA_ARGS__, h, w, H, W, nseg__);                         \
    else                                                                                                                     \
      CFEN_LAUNCH(K<1>, dim3((unsigned)blocks__), dim3(256), 0, s, __VA_ARGS__, h, w, H, W, nseg__);                          \
    CFEN_CHECK_LAUNCH(what);                                                                                                 \
  } while (0)

// ---- reductions -------------------------------------------------------------------------------------------------------------------------
// The ORDER of the additions is the contract: scores are promised to be the same bits on every run, on any stream, at any batch size, so
// there are no atomics and no counters on fp64 sums anywhere; a sum goes lane butterfly -> four waves in wave order -> partials in index order.
template <typename T>
CFEN_DEV T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);      // butterfly: every lane ends with the bitwise identical total
  return v;
}

// the four waves' values red[0], red[stride], red[2 stride], red[3 stride], added left to right
CFEN_DEV double block4_sum(const double* red, int stride) { return ((red[0] + red[stride]) + red[2 * stride]) + red[3 * stride]; }

// A workgroup of 256 threads adds n partials of NP interleaved doubles each: partial i goes to thread i % 256 in ascending i, then a tree
// over the threads from 128 down to 1.  Ends behind a barrier with total k in red[k][0].
template <int NP>
CFEN_DEV void img_reduce_partials(const double* __restrict__ p, int n, double (*red)[256]) {
  const int tid = threadIdx.x;
  double s[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) s[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
#pragma unroll
    for (int k = 0; k < NP; ++k) s[k] += p[NP * i + k];
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) red[k][tid] = s[k];
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if (tid < m) {
#pragma unroll
      for (int k = 0; k < NP; ++k) red[k][tid] += red[k][tid + m];
    }
    __syncthreads();
  }
}

// ---- the SSIM tile (k_metrics, k_planes) --------------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns MT_H x MT_W = 24 x 64 window positions: it stages the (24 + 10) x (64 + 10) values under them of both images
// as fp32 on the [0,1] scale (zeros past the edge) into sa / sb, then
//   row pass   : the 11-tap filter along x over a, b, a^2, b^2, ab -> five (34 x 64) planes in hq; a wave reads 64 consecutive floats per tap;
//   column pass: a thread owns one column and MT_R = 6 consecutive rows, reads the 16 row-filtered values under them once per plane and
//                leaves the five filtered quantities of its 6 window positions in f.
// The order of every fmaf is written out here, so every kernel built on the tile forms the same bits from the same staged values.
constexpr int MT_H = 24, MT_W = 64, MT_HALO = 10, MT_TAPS = 11;
constexpr int MT_SH = MT_H + MT_HALO, MT_SW = MT_W + MT_HALO;   // staged rows / columns
constexpr int MT_R = MT_H / 4;                                   // rows per thread in the column pass (4 waves, one column per lane)

// exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, evaluated in fp64 and rounded once
[[maybe_unused]] static __constant__ const float MT_G[MT_TAPS] = {1.028380084e-03f, 7.598758135e-03f, 3.600077213e-02f, 1.093606895e-01f,
                                                                  2.130055377e-01f, 2.660117249e-01f, 2.130055377e-01f, 1.093606895e-01f,
                                                                  3.600077213e-02f, 7.598758135e-03f, 1.028380084e-03f};

// tiles along an edge of L values: the window positions L - 10 in steps of T (the last tile also owns the edge's 10 values without a window)
static inline long long metrics_tiles(int L, int T) { return ((long long)L - MT_HALO + T - 1) / T; }

// row pass: column `lane` of rows wave, wave + 4, ...  The caller puts a barrier between the two passes.
CFEN_DEV void ssim_row_pass(const float (*sa)[MT_SW], const float (*sb)[MT_SW], float (*hq)[MT_SH][MT_W], int wave, int lane) {
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
}

// column pass: column `lane`, rows wave * MT_R .. + MT_R - 1
CFEN_DEV void ssim_col_pass(const float (*hq)[MT_SH][MT_W], int wave, int lane, float (&f)[5][MT_R]) {
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
}
