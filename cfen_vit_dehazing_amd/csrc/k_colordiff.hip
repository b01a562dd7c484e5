// CIEDE2000 colour difference of 8-bit sRGB images (include/cfen_colordiff.h states the definition and the contract; tests/ciede_ref.py restates
// it in float64).  Scored beside k_image_metrics under test.py --eval --eval_ciede2000 (metrics.ciede2000, ops.image_ciede2000).
//
//   k_ciede2000        : a workgroup (256 threads, 4 waves) owns CD_RUN = 1024 consecutive pixels of ONE image pair and stages the 256-entry
//                        sRGB-to-linear table in LDS.  A thread takes 4 consecutive pixels: 12 bytes per image, three dword loads where the
//                        image's first byte is 4-byte aligned (12 * thread keeps that alignment) and all four pixels exist, single bytes
//                        elsewhere -- the choice is made per image and per input, the bytes and so the results are the same.  The four fp32
//                        values are added in pixel order in fp64, the wave's 64 sums by a shuffle butterfly, the four waves' sums through LDS
//                        in wave order; thread 0 writes the workgroup's one partial.  The map, when asked for, is stored as 16 bytes where
//                        the image's map begins on a 16-byte boundary, as single floats elsewhere and in the tail.
//   k_ciede2000_finish : one workgroup per image adds the partials in the fixed order of img_reduce_partials (cfen_image.hpp) and divides by H W.
// Two launches; no atomics, no counters, no scratch memory (private segment 0: checked with -Rpass-analysis=kernel-resource-usage).
#include <math.h>

#include "../../include/cfen_colordiff.h"
#include "cfen_image.hpp"

namespace {

constexpr int CD_PIX = 4;                      // pixels per thread
constexpr int CD_RUN = 256 * CD_PIX;           // pixels per workgroup
constexpr int CD_MAX_EDGE = 65536;
constexpr int CD_MAX_BATCH = 65535;            // grid.y

// IEC 61966-2-1, each row divided by its own sum in fp64 and rounded once
#define CD_ROW(m0, m1, m2, k) ((float)((k) / (((m0) + (m1)) + (m2))))
constexpr float CD_XR = CD_ROW(0.4124564, 0.3575761, 0.1804375, 0.4124564), CD_XG = CD_ROW(0.4124564, 0.3575761, 0.1804375, 0.3575761),
                CD_XB = CD_ROW(0.4124564, 0.3575761, 0.1804375, 0.1804375);
constexpr float CD_YR = CD_ROW(0.2126729, 0.7151522, 0.0721750, 0.2126729), CD_YG = CD_ROW(0.2126729, 0.7151522, 0.0721750, 0.7151522),
                CD_YB = CD_ROW(0.2126729, 0.7151522, 0.0721750, 0.0721750);
constexpr float CD_ZR = CD_ROW(0.0193339, 0.1191920, 0.9503041, 0.0193339), CD_ZG = CD_ROW(0.0193339, 0.1191920, 0.9503041, 0.1191920),
                CD_ZB = CD_ROW(0.0193339, 0.1191920, 0.9503041, 0.9503041);
#undef CD_ROW
constexpr float CD_T0 = (float)((6.0 / 29.0) * (6.0 / 29.0) * (6.0 / 29.0)), CD_SLOPE = (float)(841.0 / 108.0), CD_OFF = (float)(4.0 / 29.0);
constexpr float CD_POW25_7 = 6103515625.f;     // 25^7
constexpr float CD_DEG = (float)(180.0 / 3.14159265358979323846);

struct Lab {
  float L, a, b;
};

CFEN_DEV float cd_f(float t) { return t > CD_T0 ? cbrtf(t) : t * CD_SLOPE + CD_OFF; }

CFEN_DEV Lab cd_lab(unsigned r, unsigned g, unsigned b, const float* lin) {
  const float lr = lin[r], lg = lin[g], lb = lin[b];
  const float fx = cd_f((CD_XR * lr + CD_XG * lg) + CD_XB * lb);
  const float fy = cd_f((CD_YR * lr + CD_YG * lg) + CD_YB * lb);
  const float fz = cd_f((CD_ZR * lr + CD_ZG * lg) + CD_ZB * lb);
  const bool grey = r == g && g == b;          // achromatic by definition
  Lab o;
  o.L = 116.f * fy - 16.f;
  o.a = grey ? 0.f : 500.f * (fx - fy);
  o.b = grey ? 0.f : 200.f * (fy - fz);
  return o;
}

CFEN_DEV float cd_pow7(float x) {
  const float x2 = x * x, x4 = x2 * x2;
  return x4 * x2 * x;
}

// hue in degrees in [0, 360]; 0 for the achromatic colour
CFEN_DEV float cd_hue(float b, float ap) {
  if (ap == 0.f && b == 0.f) return 0.f;
  const float h = atan2f(b, ap) * CD_DEG;
  return h < 0.f ? h + 360.f : h;
}

CFEN_DEV float cd_cos_deg(float d) { return cospif(d / 180.f); }
CFEN_DEV float cd_sin_deg(float d) { return sinpif(d / 180.f); }

CFEN_DEV float cd_de00(const Lab p, const Lab q) {
  const float C1 = sqrtf(p.a * p.a + p.b * p.b), C2 = sqrtf(q.a * q.a + q.b * q.b);
  const float c7 = cd_pow7(0.5f * (C1 + C2));
  const float G = 0.5f * (1.f - sqrtf(c7 / (c7 + CD_POW25_7)));
  const float a1 = (1.f + G) * p.a, a2 = (1.f + G) * q.a;
  const float C1p = sqrtf(a1 * a1 + p.b * p.b), C2p = sqrtf(a2 * a2 + q.b * q.b);
  const float h1 = cd_hue(p.b, a1), h2 = cd_hue(q.b, a2);
  const float dL = q.L - p.L, dC = C2p - C1p;
  const float CC = C1p * C2p;
  const bool z = CC == 0.f;
  float dh = h2 - h1;
  dh = dh > 180.f ? dh - 360.f : dh < -180.f ? dh + 360.f : dh;
  if (z) dh = 0.f;
  const float dH = 2.f * sqrtf(CC) * cd_sin_deg(0.5f * dh);
  const float Lb = 0.5f * (p.L + q.L), Cb = 0.5f * (C1p + C2p);
  const float hs = h1 + h2;
  float hb = fabsf(h1 - h2) <= 180.f ? 0.5f * hs : hs < 360.f ? 0.5f * (hs + 360.f) : 0.5f * (hs - 360.f);
  if (z) hb = hs;
  const float T = 1.f - 0.17f * cd_cos_deg(hb - 30.f) + 0.24f * cd_cos_deg(2.f * hb) + 0.32f * cd_cos_deg(3.f * hb + 6.f) -
                  0.20f * cd_cos_deg(4.f * hb - 63.f);
  const float u = (hb - 275.f) / 25.f;
  const float dth = 30.f * expf(-(u * u));
  const float cb7 = cd_pow7(Cb);
  const float Rc = 2.f * sqrtf(cb7 / (cb7 + CD_POW25_7));
  const float l50 = (Lb - 50.f) * (Lb - 50.f);
  const float Sl = 1.f + 0.015f * l50 / sqrtf(20.f + l50), Sc = 1.f + 0.045f * Cb, Sh = 1.f + 0.015f * Cb * T;
  const float Rt = -cd_sin_deg(2.f * dth) * Rc;
  const float tl = dL / Sl, tc = dC / Sc, th = dH / Sh;
  return sqrtf(fmaxf(tl * tl + tc * tc + th * th + Rt * tc * th, 0.f));
}

union CdBytes {
  unsigned u[3];
  unsigned char c[12];
};

// the thread's n <= 4 pixels of one image, from byte offset `off` of the image that starts at `img`; `vec`: img is 4-byte aligned
CFEN_DEV CdBytes cd_load(const unsigned char* __restrict__ img, long long off, int n, bool vec) {
  CdBytes v;
  v.u[0] = v.u[1] = v.u[2] = 0u;
  if (vec && n == CD_PIX) {
    const unsigned* p = reinterpret_cast<const unsigned*>(img + off);      // off = 12 * (pixel / 4): stays 4-byte aligned
    v.u[0] = p[0];
    v.u[1] = p[1];
    v.u[2] = p[2];
  } else {
#pragma unroll
    for (int j = 0; j < 3 * CD_PIX; ++j)
      if (j < 3 * n) v.c[j] = img[off + j];
  }
  return v;
}

__global__ __launch_bounds__(256) void k_ciede2000(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long long npix,
                                                   const float* __restrict__ table, float* __restrict__ map, double* __restrict__ part) {
  __shared__ float lin[256];
  __shared__ double red[4];
  const int tid = threadIdx.x, img = blockIdx.y;
  lin[tid] = table[tid];
  const unsigned char* pa = a + (long long)img * npix * 3;
  const unsigned char* pb = b + (long long)img * npix * 3;
  const long long p0 = (long long)blockIdx.x * CD_RUN + (long long)tid * CD_PIX;
  const long long left = npix - p0;
  const int n = left >= CD_PIX ? CD_PIX : left > 0 ? (int)left : 0;          // pixels this thread owns
  const bool va = (reinterpret_cast<uintptr_t>(pa) & 3) == 0, vb = (reinterpret_cast<uintptr_t>(pb) & 3) == 0;      // block-uniform
  CdBytes ca, cb;
  ca.u[0] = ca.u[1] = ca.u[2] = cb.u[0] = cb.u[1] = cb.u[2] = 0u;
  if (n > 0) {
    ca = cd_load(pa, p0 * 3, n, va);
    cb = cd_load(pb, p0 * 3, n, vb);
  }
  __syncthreads();
  float de[CD_PIX];
#pragma unroll
  for (int k = 0; k < CD_PIX; ++k)              // pixels past the end are black against black: 0, and not stored
    de[k] = cd_de00(cd_lab(ca.c[3 * k], ca.c[3 * k + 1], ca.c[3 * k + 2], lin), cd_lab(cb.c[3 * k], cb.c[3 * k + 1], cb.c[3 * k + 2], lin));
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < CD_PIX; ++k)
    if (k < n) s += (double)de[k];
  if (map != nullptr && n > 0) {
    float* m = map + (long long)img * npix + p0;
    if (n == CD_PIX && (reinterpret_cast<uintptr_t>(m) & 15) == 0) {
      const floatx4 v = {de[0], de[1], de[2], de[3]};
      *reinterpret_cast<floatx4*>(m) = v;
    } else {
#pragma unroll
      for (int k = 0; k < CD_PIX; ++k)
        if (k < n) m[k] = de[k];
    }
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) part[(long long)img * gridDim.x + blockIdx.x] = block4_sum(red, 1);
}

__global__ __launch_bounds__(256) void k_ciede2000_finish(const double* __restrict__ part, int nparts, double count, double* __restrict__ out) {
  __shared__ double red[1][256];
  const int b = blockIdx.x;
  img_reduce_partials<1>(part + (long long)b * nparts, nparts, red);
  if (threadIdx.x == 0) out[b] = red[0][0] / count;
}

bool cd_dims_ok(int B, int H, int W) { return B >= 1 && B <= CD_MAX_BATCH && H >= 1 && W >= 1 && H <= CD_MAX_EDGE && W <= CD_MAX_EDGE; }

long long cd_parts(int H, int W) { return ((long long)H * W + CD_RUN - 1) / CD_RUN; }      // <= 2^22

}  // namespace

extern "C" size_t cfen_ciede2000_bytes(int B, int H, int W) {
  if (!cd_dims_ok(B, H, W)) return 0;
  return (size_t)B * (size_t)cd_parts(H, W) * sizeof(double);
}

extern "C" int cfen_ciede2000_u8(const unsigned char* a, const unsigned char* b, int B, int H, int W, const float* table, void* scratch, float* map,
                                 double* out, void* stream) {
  CFEN_CHECK_ARG(a && b && table && scratch && out, "ciede2000_u8: null pointer (a, b, table, scratch and out are all required)");
  CFEN_CHECK_ARG(B >= 1 && B <= CD_MAX_BATCH, "ciede2000_u8: B = %d outside 1 .. %d", B, CD_MAX_BATCH);
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= CD_MAX_EDGE && W <= CD_MAX_EDGE, "ciede2000_u8: sizes H = %d, W = %d outside 1 .. %d", H, W, CD_MAX_EDGE);
  CFEN_CHECK_ARG(cfen_aligned(out, 8) && cfen_aligned(scratch, 8), "ciede2000_u8: out and scratch must be 8-byte aligned (doubles)");
  CFEN_CHECK_ARG(cfen_aligned(table, 4) && cfen_aligned(map, 4), "ciede2000_u8: table and map must be 4-byte aligned (floats)");
  const long long npix = (long long)H * W;
  const int nparts = (int)cd_parts(H, W);
  hipStream_t s = (hipStream_t)stream;
  CFEN_LAUNCH(k_ciede2000, dim3((unsigned)nparts, (unsigned)B), dim3(256), 0, s, a, b, npix, table, map, (double*)scratch);
  CFEN_CHECK_LAUNCH("ciede2000_u8");
  CFEN_LAUNCH(k_ciede2000_finish, dim3((unsigned)B), dim3(256), 0, s, (const double*)scratch, nparts, (double)npix, out);
  CFEN_CHECK_LAUNCH("ciede2000_u8 (finish)");
  return CFEN_OK;
}
