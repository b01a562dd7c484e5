// PIL-exact resampling of 8-bit RGB images (resample.py builds the tables; include/cfen_resample.h states the contract).
//
// PIL resamples uint8 images in fixed point: per axis a table gives every output index xx a first source index xmin, a tap count n and n
// int32 weights k (double-precision filter weights, normalised, rounded once to 22 bits on the host); an output byte is
//     clip((2^21 + sum_{x < n} src[xmin + x] * k[x]) >> 22, 0, 255)            int32 accumulator, arithmetic shift
// and the horizontal pass is stored as uint8 before the vertical pass reads it.  Everything below is integer arithmetic: the result does not
// depend on summation order, contraction or rounding mode, and equals Image.resize byte for byte.
//
//   k_resample_h : rows x W pixels -> rows x W2.  A workgroup of 4 waves takes RS_ROWS = 4 rows x RS_TX = 64 output columns: wave r stages the
//                  run of row r that the 64 columns read ([xmin of the first, xmin + n of the last): 31 taps = 93 bytes per pixel at 3840 -> 512,
//                  overlapping between neighbours) into LDS with 16-byte loads -- the LDS image keeps the global address modulo 16, so both
//                  sides of the copy are aligned whatever the row pitch -- and the 64 x xk weights go to LDS tap-major (lanes read consecutive
//                  words).  One thread = one output pixel (3 bytes).  A table wider than RS_KCAP taps or a run longer than RS_SEG bytes (540 -> 16
//                  is 137 taps; bilinear / box at scale > ~10) takes the same loop on global memory instead: a block-uniform choice.
//   k_resample_v : every byte of an output row uses the same taps.  A wave takes 1 KiB of one output row, a lane 16 consecutive bytes, and
//                  reads one 16-byte vector per tap row -- or 16 single bytes when the row pitch 3 W2 or a base pointer is not a multiple of
//                  16; the last lane of a row may then own fewer than 16 bytes.  xmin, n and the weights are wave-uniform: scalar loads, SGPR
//                  operands.
// Two launches when both axes change, the uint8 intermediate (rows x W2) in `tmp`; no atomics, no counters, no scratch.
#include "cfen_common.hpp"

namespace {

constexpr int RS_BITS = 22;
constexpr int RS_ROWS = 4, RS_TX = 64;       // k_resample_h: rows x output columns per workgroup (one wave per row)
constexpr int RS_SEG = 2048;                 // staged bytes per row at most; + 16: the run starts at its global address modulo 16
constexpr int RS_KCAP = 32;                  // taps per output column whose weights are staged

// (the compiler may fuse this shift-then-clamp, two bytes at a time, into gfx950's v_ashr_pk_u8_i32; it does not in the kernels below.  In a
// 4-byte variant of k_resample_v it did, and that variant gave wrong bytes on the device: DESIGN section 13)
CFEN_DEV unsigned char rs_clip(int acc) {
  const int v = acc >> RS_BITS;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(256) void k_resample_h(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const int* __restrict__ bounds,
                                                    const int* __restrict__ coef, int xk, long long nrows, int W, int W2, int ntx) {
  __shared__ __attribute__((aligned(16))) unsigned char seg[RS_ROWS][RS_SEG + 16];
  __shared__ int cw[RS_KCAP * RS_TX];
  const int tid = threadIdx.x, r = tid >> 6, c = tid & 63;
  const long long rb = blockIdx.x / ntx;
  const int x0 = (int)(blockIdx.x - rb * ntx) * RS_TX;
  const int txn = min(RS_TX, W2 - x0);
  const long long row = rb * RS_ROWS + r;
  const int s0 = bounds[2 * x0];                                                         // first source pixel of the tile's run
  const int s1 = bounds[2 * (x0 + txn - 1)] + bounds[2 * (x0 + txn - 1) + 1];          // one past its last (xmin and xmin + n do not decrease)
  const int nbytes = (s1 - s0) * 3;
  const bool staged = xk <= RS_KCAP && nbytes <= RS_SEG;                                 // block-uniform
  const unsigned char* srow = src + (row < nrows ? row : 0) * (long long)W * 3;
  int lead = 0;
  if (staged) {
    for (int i = tid; i < txn * xk; i += 256) {
      const int x = i / xk, t = i - x * xk;
      cw[t * RS_TX + x] = coef[(long long)x0 * xk + i];
    }
    if (row < nrows) {
      const unsigned char* g0 = srow + (long long)s0 * 3;
      lead = (int)(reinterpret_cast<uintptr_t>(g0) & 15);
      const unsigned char* base = g0 - lead;                                             // 16-byte aligned; LDS position p <-> base + p
      const int end = lead + nbytes;
      for (int p = c * 16; p < end; p += 64 * 16) {
        if (p >= lead && p + 16 <= end) {
          *reinterpret_cast<uint4*>(&seg[r][p]) = *reinterpret_cast<const uint4*>(base + p);
        } else {
          for (int q = max(p, lead); q < min(p + 16, end); ++q) seg[r][q] = base[q];     // the ragged ends: only bytes of the run are read
        }
      }
    }
  }
  __syncthreads();
  if (row >= nrows || c >= txn) return;
  const int x = x0 + c;
  const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
  int a0 = 1 << (RS_BITS - 1), a1 = a0, a2 = a0;
  if (staged) {
    const unsigned char* p = &seg[r][lead + (xmin - s0) * 3];
    for (int t = 0; t < n; ++t) {
      const int k = cw[t * RS_TX + c];
      a0 += p[3 * t] * k;
      a1 += p[3 * t + 1] * k;
      a2 += p[3 * t + 2] * k;
    }
  } else {
    const unsigned char* p = srow + (long long)xmin * 3;
    const int* kr = coef + (long long)x * xk;
    for (int t = 0; t < n; ++t) {
      const int k = kr[t];
      a0 += p[3 * t] * k;
      a1 += p[3 * t + 1] * k;
      a2 += p[3 * t + 2] * k;
    }
  }
  unsigned char* o = dst + (row * W2 + x) * 3;
  o[0] = rs_clip(a0);
  o[1] = rs_clip(a1);
  o[2] = rs_clip(a2);
}

template <int V> struct RsVec;
template <> struct RsVec<16> { typedef uint4 type; };
template <> struct RsVec<1> { typedef unsigned char type; };

// src (B, H, pitch bytes) -> dst (B, H2, pitch bytes); pitch % V == 0 and both base pointers V-byte aligned
template <int V>
__global__ __launch_bounds__(256) void k_resample_v(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, const int* __restrict__ bounds,
                                                    const int* __restrict__ coef, int yk, int B, int H, int H2, int pitch, int nseg, long long ntasks) {
  typedef typename RsVec<V>::type vec_t;
  constexpr int NV = 16 / V;
  const long long task = __builtin_amdgcn_readfirstlane((int)((long long)blockIdx.x * 4 + (threadIdx.x >> 6)));      // (row, 1 KiB segment) of this wave
  if (task >= ntasks) return;
  const int orow = (int)(task / nseg), sg = (int)(task - (long long)orow * nseg);
  const int b = orow / H2, yy = orow - b * H2;
  const int off = sg * 1024 + (threadIdx.x & 63) * 16;
  if (off >= pitch) return;
  const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
  const int* kr = coef + (long long)yy * yk;
  const unsigned char* p = src + ((long long)b * H + ymin) * pitch + off;
  int acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 1 << (RS_BITS - 1);
  for (int t = 0; t < n; ++t, p += pitch) {
    const int k = kr[t];
    union { vec_t v[NV]; unsigned char c[16]; } u;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      if (V == 16 || off + e * V < pitch) u.v[e] = *reinterpret_cast<const vec_t*>(p + e * V);      // pitch % V == 0: a unit is whole or absent
      else u.v[e] = vec_t();
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += u.c[j] * k;
  }
  union { vec_t v[NV]; unsigned char c[16]; } o;
#pragma unroll
  for (int j = 0; j < 16; ++j) o.c[j] = rs_clip(acc[j]);
  unsigned char* q = dst + ((long long)b * H2 + yy) * pitch + off;
#pragma unroll
  for (int e = 0; e < NV; ++e)
    if (V == 16 || off + e * V < pitch) *reinterpret_cast<vec_t*>(q + e * V) = o.v[e];
}

__global__ __launch_bounds__(256) void k_resample_copy(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, long long nbytes) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nbytes; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

int rs_horizontal(const unsigned char* src, unsigned char* dst, const int* bounds, const int* coef, int xk, long long nrows, int W, int W2, hipStream_t s) {
  const int ntx = (W2 + RS_TX - 1) / RS_TX;
  const long long blocks = (nrows + RS_ROWS - 1) / RS_ROWS * ntx;
  CFEN_CHECK_ARG(blocks <= 0x7fffffffLL, "resample_u8: %lld rows x %d columns is too large for one launch", nrows, W2);
  CFEN_LAUNCH(k_resample_h, dim3((unsigned)blocks), dim3(256), 0, s, src, dst, bounds, coef, xk, nrows, W, W2, ntx);
  CFEN_CHECK_LAUNCH("resample_u8 (horizontal)");
  return CFEN_OK;
}

int rs_vertical(const unsigned char* src, unsigned char* dst, const int* bounds, const int* coef, int yk, int B, int H, int H2, int W, hipStream_t s) {
  const int pitch = W * 3, nseg = (pitch + 1023) / 1024;
  const long long ntasks = (long long)B * H2 * nseg;
  CFEN_CHECK_ARG(ntasks <= 0x7fffffffLL, "resample_u8: %d x %d rows of %d bytes is too large for one launch", B, H2, pitch);
  const dim3 grid((unsigned)((ntasks + 3) / 4));
  const uintptr_t both = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | (uintptr_t)pitch;
  if (both % 16 == 0)
    CFEN_LAUNCH(k_resample_v<16>, grid, dim3(256), 0, s, src, dst, bounds, coef, yk, B, H, H2, pitch, nseg, ntasks);
  else
    CFEN_LAUNCH(k_resample_v<1>, grid, dim3(256), 0, s, src, dst, bounds, coef, yk, B, H, H2, pitch, nseg, ntasks);
  CFEN_CHECK_LAUNCH("resample_u8 (vertical)");
  return CFEN_OK;
}

}  // namespace

// an edge of the cap squared, times 3 bytes and a batch of the cap, stays far inside 64-bit indices; row pitches and tap products fit int
#define CFEN_RESAMPLE_MAX_EDGE 65536

int cfen_resample_u8_impl(const unsigned char* src, int B, int H, int W, const int* xbounds, const int* xcoef, int xk, int W2, const int* ybounds,
                          const int* ycoef, int yk, int H2, unsigned char* tmp, unsigned char* dst, hipStream_t s) {
  CFEN_CHECK_ARG(src && dst, "resample_u8: null image pointer");
  CFEN_CHECK_ARG(B >= 1 && B <= 65536, "resample_u8: batch %d outside 1 .. 65536", B);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H2 >= 1 && W2 >= 1 && H <= CFEN_RESAMPLE_MAX_EDGE && W <= CFEN_RESAMPLE_MAX_EDGE && H2 <= CFEN_RESAMPLE_MAX_EDGE &&
                 W2 <= CFEN_RESAMPLE_MAX_EDGE, "resample_u8: sizes %d x %d -> %d x %d outside 1 .. %d", H, W, H2, W2, CFEN_RESAMPLE_MAX_EDGE);
  const bool hpass = xbounds || xcoef || xk, vpass = ybounds || ycoef || yk;
  CFEN_CHECK_ARG(!hpass || (xbounds && xcoef && xk >= 1 && xk <= 2 * CFEN_RESAMPLE_MAX_EDGE + 1), "resample_u8: the horizontal table needs bounds, weights and xk >= 1");
  CFEN_CHECK_ARG(!vpass || (ybounds && ycoef && yk >= 1 && yk <= 2 * CFEN_RESAMPLE_MAX_EDGE + 1), "resample_u8: the vertical table needs bounds, weights and yk >= 1");
  CFEN_CHECK_ARG(hpass || W2 == W, "resample_u8: no horizontal table, but W2 = %d differs from W = %d", W2, W);
  CFEN_CHECK_ARG(vpass || H2 == H, "resample_u8: no vertical table, but H2 = %d differs from H = %d", H2, H);
  CFEN_CHECK_ARG(!(hpass && vpass) || tmp, "resample_u8: both passes run: tmp (B*H*W2*3 bytes) is required");
  CFEN_CHECK_ARG(src != dst && (!(hpass && vpass) || (tmp != src && tmp != dst)), "resample_u8: src, tmp and dst must be different buffers");
  if (hpass && vpass) {
    const int rc = rs_horizontal(src, tmp, xbounds, xcoef, xk, (long long)B * H, W, W2, s);
    return rc ? rc : rs_vertical(tmp, dst, ybounds, ycoef, yk, B, H, H2, W2, s);
  }
  if (hpass) return rs_horizontal(src, dst, xbounds, xcoef, xk, (long long)B * H, W, W2, s);
  if (vpass) return rs_vertical(src, dst, ybounds, ycoef, yk, B, H, H2, W, s);
  const long long nbytes = (long long)B * H * W * 3;
  const long long g = (nbytes + 255) / 256;
  CFEN_LAUNCH(k_resample_copy, dim3((unsigned)(g > 16384 ? 16384 : g)), dim3(256), 0, s, src, dst, nbytes);
  CFEN_CHECK_LAUNCH("resample_u8 (copy)");
  return CFEN_OK;
}
