// Planar YCbCr frames <-> interleaved RGB bytes (include/cfen_yuv.h states the definition, the frame layout and the thread-to-pixel layout;
// tests/yuv_ref.py restates the definition in numpy).  Used by dehaze_video.py (cfen_vit_dehazing_amd/video.py) through ops.yuv_to_rgb_u8 /
// ops.rgb_to_yuv_u8: a y4m frame goes to the device as it is and comes back the same way.
//
//   k_yuv_to_rgb : grid (groups / 256, B).  A thread owns four consecutive linear pixel indices; the groups start at p = address of the frame's
//                  RGB bytes (mod 4), so a group's twelve output bytes are three aligned dwords.  Inside one row the thread reads its four luma
//                  bytes (a dword when aligned), the four chroma columns its pixels share from one or two chroma rows, combines them vertically
//                  (weights in quarters, 10 bits per column, four columns packed in 64 bits) and picks two columns per pixel by shifting.
//                  Groups over a row end or the frame's ends go pixel by pixel.
//   k_rgb_to_yuv : grid (luma blocks + chroma blocks, B).  Luma blocks: the same groups, three dword loads, one Y dword (and Cb, Cr dwords for
//                  4:4:4).  Chroma blocks: one chroma row per block row, a thread owns the samples (i, i + 1) of both planes: the pixels
//                  2i .. 2i + 3 (+ 2i - 1 for the co-sited filters) of one or two rows -> bytes d by the forward formula -> the filter.
// Integer arithmetic only; no LDS, no atomics, no scratch; the table travels in the kernel arguments.
#include <stdint.h>

#include "../../include/cfen_yuv.h"
#include "cfen_common.hpp"

namespace {

constexpr int YV_THREADS = 256;

CFEN_DEV int yv_clamp(int v) { return min(max(v, 0), 255); }

CFEN_DEV unsigned yv_load4(const unsigned char* p) {                  // four bytes, little endian, at any address
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const unsigned*>(p);
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

CFEN_DEV void yv_store4(unsigned char* p, unsigned v) {
  if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    *reinterpret_cast<unsigned*>(p) = v;
  } else {
    p[0] = (unsigned char)v;
    p[1] = (unsigned char)(v >> 8);
    p[2] = (unsigned char)(v >> 16);
    p[3] = (unsigned char)(v >> 24);
  }
}

CFEN_DEV unsigned yv_byte(unsigned v, int k) { return (v >> (8 * k)) & 255u; }

// one colour of the inverse / forward formula
// The empty asm hides the clamped value from the optimiser.  Without it hipcc (ROCm 7.2) fuses shift + clamp + packing of two neighbouring
// bytes into v_ashr_pk_u8_i32 and ORs bytes 2 and 3 into the same register as if its upper half were zero; on the MI355X the upper half kept
// bits of the old register (one operand of the instruction), and byte 2 of every packed dword came out wrong (tests/test_hip_yuv.py).
CFEN_DEV int yv_dot(const cfen_yuv_table& t, int row, int a, int b, int c, int add) {
  int v = yv_clamp((t.coef[3 * row] * a + t.coef[3 * row + 1] * b + t.coef[3 * row + 2] * c + add) >> 14);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
  return v;
}

// the first column an upsampled pixel x reads and its two weights (the second column is the next one, clamped)
CFEN_DEV void yv_htaps(int chroma, int x, int& c0, int& w0, int& w1) {
  const int i = x >> 1, odd = x & 1;
  if (chroma == CFEN_YUV_420JPEG) {
    c0 = odd ? i : i - 1;
    w0 = odd ? 3 : 1;
    w1 = odd ? 1 : 3;
  } else {                                                            // co-sited
    c0 = i;
    w0 = odd ? 2 : 4;
    w1 = odd ? 2 : 0;
  }
}

// Cb' and Cr' of N pixels x0 .. x0 + N - 1 of row y (N = 4: all in one row; N = 1), subsampled formats only.  NC columns are read once.
template <int N>
CFEN_DEV void yv_chroma_up(const unsigned char* __restrict__ pcb, const unsigned char* __restrict__ pcr, int chroma, int Hc, int Wc, int y, int x0,
                           int* cb, int* cr) {
  constexpr int NC = N == 4 ? 4 : 2;
  int ra, rb, wa, wb;
  if (chroma <= CFEN_YUV_420MPEG2) {
    const int j = y >> 1;
    if (y & 1) {
      ra = j, rb = min(j + 1, Hc - 1), wa = 3, wb = 1;
    } else {
      ra = max(j - 1, 0), rb = j, wa = 1, wb = 3;
    }
  } else {
    ra = rb = y, wa = 4, wb = 0;
  }
  int cbase, w0, w1;
  yv_htaps(chroma, x0, cbase, w0, w1);
  unsigned long long tb = 0ull, tr = 0ull;                             // column k of the vertical sum in bits 16k .. 16k + 15 (at most 4 * 255)
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int col = min(max(cbase + k, 0), Wc - 1);
    const size_t ia = (size_t)ra * Wc + col, ib = (size_t)rb * Wc + col;
    unsigned vb = wa * (unsigned)pcb[ia], vr = wa * (unsigned)pcr[ia];
    if (wb != 0) {
      vb += wb * (unsigned)pcb[ib];
      vr += wb * (unsigned)pcr[ib];
    }
    tb |= (unsigned long long)vb << (16 * k);
    tr |= (unsigned long long)vr << (16 * k);
  }
#pragma unroll
  for (int m = 0; m < N; ++m) {
    int c0;
    yv_htaps(chroma, x0 + m, c0, w0, w1);
    const int k0 = c0 - cbase;                                         // 0 .. NC - 2
    const int b0 = (int)((tb >> (16 * k0)) & 0xffffu), b1 = (int)((tb >> (16 * k0 + 16)) & 0xffffu);
    const int r0 = (int)((tr >> (16 * k0)) & 0xffffu), r1 = (int)((tr >> (16 * k0 + 16)) & 0xffffu);
    cb[m] = (w0 * b0 + w1 * b1 + 8) >> 4;
    cr[m] = (w0 * r0 + w1 * r1 + 8) >> 4;
  }
}

__global__ __launch_bounds__(YV_THREADS) void k_yuv_to_rgb(const unsigned char* __restrict__ frames, size_t stride, int H, int W, int Hc, int Wc,
                                                           int chroma, cfen_yuv_table t, unsigned char* __restrict__ rgb) {
  const long long npix = (long long)H * W;
  const unsigned char* __restrict__ f = frames + (size_t)blockIdx.y * stride;
  unsigned char* __restrict__ o = rgb + (size_t)blockIdx.y * (size_t)npix * 3;
  const unsigned char* __restrict__ pcb = f + npix;
  const unsigned char* __restrict__ pcr = pcb + (size_t)Hc * Wc;
  const int a = (int)(reinterpret_cast<uintptr_t>(o) & 3);              // block-uniform: groups p = a (mod 4) store on dword boundaries
  const long long p0 = 4 * ((long long)blockIdx.x * YV_THREADS + threadIdx.x) + a - 4;
  if (p0 >= npix || p0 + 4 <= 0) return;
  const int oy = t.luma_offset;
  const int y0 = (int)((unsigned long long)max(p0, 0ll) / (unsigned)W), x0 = (int)(max(p0, 0ll) - (long long)y0 * W);
  if (p0 >= 0 && p0 + 4 <= npix && x0 + 4 <= W) {                      // four pixels of one row, wholly inside the frame
    const unsigned yy = yv_load4(f + p0);
    int cb[4], cr[4];
    if (chroma == CFEN_YUV_MONO) {
#pragma unroll
      for (int m = 0; m < 4; ++m) cb[m] = cr[m] = 128;
    } else if (chroma == CFEN_YUV_444) {
      const unsigned vb = yv_load4(pcb + p0), vr = yv_load4(pcr + p0);
#pragma unroll
      for (int m = 0; m < 4; ++m) cb[m] = (int)yv_byte(vb, m), cr[m] = (int)yv_byte(vr, m);
    } else {
      yv_chroma_up<4>(pcb, pcr, chroma, Hc, Wc, y0, x0, cb, cr);
    }
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int Y = (int)yv_byte(yy, m) - oy, B = cb[m] - 128, R = cr[m] - 128;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int n = 3 * m + k;                                       // byte n of the twelve
        w[n >> 2] |= (unsigned)yv_dot(t, k, Y, B, R, 8192) << (8 * (n & 3));
      }
    }
    unsigned* dst = reinterpret_cast<unsigned*>(o + 3 * p0);           // address = rgb + 3 p0 = 4 a = 0 (mod 4)
    dst[0] = w[0];
    dst[1] = w[1];
    dst[2] = w[2];
    return;
  }
  for (int m = 0; m < 4; ++m) {
    const long long p = p0 + m;
    if (p < 0 || p >= npix) continue;
    const int y = (int)((unsigned long long)p / (unsigned)W), x = (int)(p - (long long)y * W);
    int cb = 128, cr = 128;
    if (chroma == CFEN_YUV_444) {
      cb = pcb[p];
      cr = pcr[p];
    } else if (chroma != CFEN_YUV_MONO) {
      yv_chroma_up<1>(pcb, pcr, chroma, Hc, Wc, y, x, &cb, &cr);
    }
    const int Y = (int)f[p] - oy;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[3 * p + k] = (unsigned char)yv_dot(t, k, Y, cb - 128, cr - 128, 8192);
  }
}

// the chroma bytes d[1], d[2] of pixel x (clamped to the row) of the image row starting at `row`
CFEN_DEV void yv_pixel_cbcr(const unsigned char* __restrict__ row, int W, int x, const cfen_yuv_table& t, int& dcb, int& dcr) {
  const unsigned char* q = row + 3 * (size_t)min(max(x, 0), W - 1);
  const int R = q[0], G = q[1], B = q[2];
  dcb = yv_dot(t, 1, R, G, B, (128 << 14) + 8192);
  dcr = yv_dot(t, 2, R, G, B, (128 << 14) + 8192);
}

__global__ __launch_bounds__(YV_THREADS) void k_rgb_to_yuv(const unsigned char* __restrict__ rgb, int H, int W, int Hc, int Wc, int chroma,
                                                           cfen_yuv_table t, unsigned char* __restrict__ frames, size_t stride, unsigned yblocks,
                                                           unsigned cbx) {
  const long long npix = (long long)H * W;
  const unsigned char* __restrict__ src = rgb + (size_t)blockIdx.y * (size_t)npix * 3;
  unsigned char* __restrict__ f = frames + (size_t)blockIdx.y * stride;
  const int a = (int)(reinterpret_cast<uintptr_t>(src) & 3);            // block-uniform: groups p = a (mod 4) load from dword boundaries
  const int oy = t.luma_offset;
  if (blockIdx.x < yblocks) {                                           // block-uniform: the luma plane (and the chroma planes of 4:4:4)
    const long long p0 = 4 * ((long long)blockIdx.x * YV_THREADS + threadIdx.x) + a - 4;
    if (p0 >= npix || p0 + 4 <= 0) return;
    const bool full = chroma == CFEN_YUV_444;
    if (p0 >= 0 && p0 + 4 <= npix) {
      const unsigned* q = reinterpret_cast<const unsigned*>(src + 3 * p0);      // address = rgb + 3 p0 = 4 a = 0 (mod 4)
      const unsigned w[3] = {q[0], q[1], q[2]};
      unsigned vy = 0u, vb = 0u, vr = 0u;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int R = (int)yv_byte(w[(3 * m) >> 2], (3 * m) & 3), G = (int)yv_byte(w[(3 * m + 1) >> 2], (3 * m + 1) & 3),
                  B = (int)yv_byte(w[(3 * m + 2) >> 2], (3 * m + 2) & 3);
        vy |= (unsigned)yv_dot(t, 0, R, G, B, (oy << 14) + 8192) << (8 * m);
        if (full) {
          vb |= (unsigned)yv_dot(t, 1, R, G, B, (128 << 14) + 8192) << (8 * m);
          vr |= (unsigned)yv_dot(t, 2, R, G, B, (128 << 14) + 8192) << (8 * m);
        }
      }
      yv_store4(f + p0, vy);
      if (full) {
        yv_store4(f + npix + p0, vb);
        yv_store4(f + 2 * npix + p0, vr);
      }
      return;
    }
    for (int m = 0; m < 4; ++m) {
      const long long p = p0 + m;
      if (p < 0 || p >= npix) continue;
      const int R = src[3 * p], G = src[3 * p + 1], B = src[3 * p + 2];
      f[p] = (unsigned char)yv_dot(t, 0, R, G, B, (oy << 14) + 8192);
      if (full) {
        f[npix + p] = (unsigned char)yv_dot(t, 1, R, G, B, (128 << 14) + 8192);
        f[2 * npix + p] = (unsigned char)yv_dot(t, 2, R, G, B, (128 << 14) + 8192);
      }
    }
    return;
  }
  // the subsampled chroma planes: chroma row j, samples i and i + 1
  const unsigned cblk = blockIdx.x - yblocks;
  const int j = (int)(cblk / cbx);
  const bool v2 = chroma <= CFEN_YUV_420MPEG2, cosited = chroma != CFEN_YUV_420JPEG;
  const int ya = v2 ? min(2 * j, H - 1) : j, yb = v2 ? min(2 * j + 1, H - 1) : j;
  // pixel 2i of row ya lies on a dword boundary when ya W + 2i = a (mod 4): shift the pairing by one sample when that needs 2i = 2 (mod 4)
  const int need = (int)((a - (long long)ya * W) & 3);
  const int ph = need == 2 ? 1 : 0;
  const int i = 2 * (int)((cblk % cbx) * YV_THREADS + threadIdx.x) - ph;
  if (i >= Wc) return;
  int sb0 = 0, sb1 = 0, sr0 = 0, sr1 = 0;                               // filter sums of sample i and i + 1, Cb and Cr
  for (int r = 0; r < (v2 ? 2 : 1); ++r) {
    const unsigned char* __restrict__ row = src + 3 * (size_t)(r == 0 ? ya : yb) * W;
    int db[4], dr[4];
    const unsigned char* q = row + 3 * (ptrdiff_t)(2 * i);
    if (i >= 0 && 2 * i + 3 <= W - 1 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) {
      const unsigned* q4 = reinterpret_cast<const unsigned*>(q);
      const unsigned w[3] = {q4[0], q4[1], q4[2]};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int R = (int)yv_byte(w[(3 * m) >> 2], (3 * m) & 3), G = (int)yv_byte(w[(3 * m + 1) >> 2], (3 * m + 1) & 3),
                  B = (int)yv_byte(w[(3 * m + 2) >> 2], (3 * m + 2) & 3);
        db[m] = yv_dot(t, 1, R, G, B, (128 << 14) + 8192);
        dr[m] = yv_dot(t, 2, R, G, B, (128 << 14) + 8192);
      }
    } else {
#pragma unroll
      for (int m = 0; m < 4; ++m) yv_pixel_cbcr(row, W, 2 * i + m, t, db[m], dr[m]);
    }
    if (cosited) {
      int lb, lr;
      yv_pixel_cbcr(row, W, 2 * i - 1, t, lb, lr);
      sb0 += lb + 2 * db[0] + db[1];
      sr0 += lr + 2 * dr[0] + dr[1];
      sb1 += db[1] + 2 * db[2] + db[3];
      sr1 += dr[1] + 2 * dr[2] + dr[3];
    } else {
      sb0 += db[0] + db[1];
      sr0 += dr[0] + dr[1];
      sb1 += db[2] + db[3];
      sr1 += dr[2] + dr[3];
    }
  }
  // 420jpeg: four bytes, (s + 2) >> 2;  420mpeg2: two row filters of weight 4, (s + 4) >> 3;  422: one, (s + 2) >> 2
  const int half = chroma == CFEN_YUV_420MPEG2 ? 4 : 2, sh = chroma == CFEN_YUV_420MPEG2 ? 3 : 2;
  const size_t cplane = (size_t)Hc * Wc;
  unsigned char* ob = f + npix + (size_t)j * Wc + i;                   // (not dereferenced at i = -1)
  unsigned char* orr = ob + cplane;
  const unsigned b0 = (unsigned)((sb0 + half) >> sh), b1 = (unsigned)((sb1 + half) >> sh);
  const unsigned r0 = (unsigned)((sr0 + half) >> sh), r1 = (unsigned)((sr1 + half) >> sh);
  const bool first = i >= 0, second = i + 1 < Wc;
  if (first && second && (reinterpret_cast<uintptr_t>(ob) & 1) == 0) {
    *reinterpret_cast<unsigned short*>(ob) = (unsigned short)(b0 | (b1 << 8));
  } else {
    if (first) ob[0] = (unsigned char)b0;
    if (second) ob[1] = (unsigned char)b1;
  }
  if (first && second && (reinterpret_cast<uintptr_t>(orr) & 1) == 0) {
    *reinterpret_cast<unsigned short*>(orr) = (unsigned short)(r0 | (r1 << 8));
  } else {
    if (first) orr[0] = (unsigned char)r0;
    if (second) orr[1] = (unsigned char)r1;
  }
}

bool yv_chroma_ok(int chroma) { return chroma >= CFEN_YUV_420JPEG && chroma <= CFEN_YUV_MONO; }

void yv_chroma_dims(int H, int W, int chroma, int* Hc, int* Wc) {
  *Hc = chroma == CFEN_YUV_MONO ? 0 : (chroma <= CFEN_YUV_420MPEG2 ? (H + 1) >> 1 : H);
  *Wc = chroma == CFEN_YUV_MONO ? 0 : (chroma == CFEN_YUV_444 ? W : (W + 1) >> 1);
}

bool yv_table_ok(const cfen_yuv_table& t) {
  for (int k = 0; k < 6; ++k)
    if (t.reserved[k] != 0) return false;
  for (int k = 0; k < 9; ++k)
    if (t.coef[k] < -65536 || t.coef[k] > 65536) return false;
  return t.luma_offset >= 0 && t.luma_offset <= 255;
}

// groups of four linear pixels that can touch a frame: the first may start up to three pixels in front of it
unsigned yv_group_blocks(int H, int W) {
  const long long groups = ((long long)H * W + 3) / 4 + 1;
  return (unsigned)((groups + YV_THREADS - 1) / YV_THREADS);           // <= 2^22 + 1
}

}  // namespace

extern "C" size_t cfen_yuv_frame_bytes(int H, int W, int chroma) {
  if (H < 1 || W < 1 || H > CFEN_YUV_MAX_EDGE || W > CFEN_YUV_MAX_EDGE || !yv_chroma_ok(chroma)) return 0;
  int Hc, Wc;
  yv_chroma_dims(H, W, chroma, &Hc, &Wc);
  return (size_t)H * W + 2 * (size_t)Hc * Wc;
}

#define YV_CHECK_ARGS(what)                                                                                                                  \
  CFEN_CHECK_ARG(frames && rgb, what ": null pointer (frames and rgb are both required)");                                                   \
  CFEN_CHECK_ARG(B >= 1 && B <= CFEN_YUV_MAX_BATCH, what ": B = %d outside 1 .. %d", B, CFEN_YUV_MAX_BATCH);                                  \
  CFEN_CHECK_ARG(H >= 1 && W >= 1 && H <= CFEN_YUV_MAX_EDGE && W <= CFEN_YUV_MAX_EDGE, what ": sizes H = %d, W = %d outside 1 .. %d", H, W,  \
                 CFEN_YUV_MAX_EDGE);                                                                                                         \
  CFEN_CHECK_ARG(yv_chroma_ok(chroma), what ": unknown chroma = %d (CFEN_YUV_420JPEG .. CFEN_YUV_MONO are 0 .. 4)", chroma);                  \
  CFEN_CHECK_ARG(frame_stride >= cfen_yuv_frame_bytes(H, W, chroma), what ": frame_stride = %zu is less than the %zu bytes of a frame",      \
                 frame_stride, cfen_yuv_frame_bytes(H, W, chroma));                                                                          \
  CFEN_CHECK_ARG(yv_table_ok(table), what ": bad table (reserved words must be 0, luma_offset 0 .. 255, coefficients within -65536 .. 65536)")

extern "C" int cfen_yuv_to_rgb_u8(const unsigned char* frames, size_t frame_stride, int B, int H, int W, int chroma, cfen_yuv_table table,
                                  unsigned char* rgb, void* stream) {
  YV_CHECK_ARGS("yuv_to_rgb_u8");
  int Hc, Wc;
  yv_chroma_dims(H, W, chroma, &Hc, &Wc);
  CFEN_LAUNCH(k_yuv_to_rgb, dim3(yv_group_blocks(H, W), (unsigned)B), dim3(YV_THREADS), 0, (hipStream_t)stream, frames, frame_stride, H, W, Hc, Wc,
              chroma, table, rgb);
  CFEN_CHECK_LAUNCH("yuv_to_rgb_u8");
  return CFEN_OK;
}

extern "C" int cfen_rgb_to_yuv_u8(const unsigned char* rgb, int B, int H, int W, int chroma, cfen_yuv_table table, unsigned char* frames,
                                  size_t frame_stride, void* stream) {
  YV_CHECK_ARGS("rgb_to_yuv_u8");
  int Hc, Wc;
  yv_chroma_dims(H, W, chroma, &Hc, &Wc);
  const unsigned yblocks = yv_group_blocks(H, W);
  const bool sub = chroma <= CFEN_YUV_422;
  const unsigned cbx = sub ? (unsigned)((Wc / 2 + 1 + YV_THREADS - 1) / YV_THREADS) : 0u;      // pairs of samples of a chroma row, one more for the shift
  const unsigned cblocks = sub ? (unsigned)Hc * cbx : 0u;                                       // <= 65536 * 65
  CFEN_LAUNCH(k_rgb_to_yuv, dim3(yblocks + cblocks, (unsigned)B), dim3(YV_THREADS), 0, (hipStream_t)stream, rgb, H, W, Hc, Wc, chroma, table, frames,
              frame_stride, yblocks, cbx);
  CFEN_CHECK_LAUNCH("rgb_to_yuv_u8");
  return CFEN_OK;
}
