// PNG encoding of the output images on the device (png.py, test.py --gpu_png): uint8 (B,H,W,3) images -> one finished zlib stream per image, the
// payload of the file's single IDAT chunk.  The host adds the container and its CRC-32 (png.assemble).  Format (include/cfen_hip.h, cfen_png_deflate):
//
//   78 01 | per strip: one non-final deflate block, then an empty non-final stored block | 01 00 00 FF FF | Adler-32 of the filtered scanlines
//
// A strip is R = max(1, 32768 / (3 W + 1)) rows: n <= 32768 filtered bytes (filter byte + 3 W bytes a row).  The empty stored block (000, pad to a
// byte, 00 00 FF FF) ends every strip on a byte boundary, so strips are coded independently and concatenated.  Literals only, no LZ77.
//
//   k_png_deflate : one 256-thread workgroup per (strip, image).
//     1. filter: a wave owns a row.  It scores None / Sub / Up / Average / Paeth by the sum of |signed residual| (libpng's heuristic; wave reduction,
//        ties to the lowest type) straight from the image in global memory -- the row above a strip's first row is read there too, zeros above row 0
//        -- and writes the winner's bytes to LDS (32 KB).
//     2. a thread owns a contiguous run of the n bytes (an ODD number of 32-bit words, so the lanes' LDS reads fall in distinct banks): 257-bin
//        histogram with LDS atomics, and the Adler-32 partial sums of its run.
//     3. cost of each of the K candidate tables = its header bits + histogram . lengths (exact); the first minimum wins, and is used only if
//        strictly below the stored block's 8 n + 40 bits.
//     4. dynamic block: bit length of every run, workgroup exclusive scan, then every thread packs its run into the zeroed LDS output buffer: a 64-bit
//        accumulator, whole 32-bit words with plain stores, the first and the last word of a run (shared with the neighbours) with LDS atomic OR.
//        Stored block: header bytes and a byte copy.
//     5. 16-byte stores of the buffer to the strip's own slot of the workspace, and a record (bytes, Adler A, Adler B, n).
//   k_png_finish  : one workgroup per (strip, image): the strip's offset is the sum of the byte lengths before it; it copies its slot there (dword
//        stores, the source re-aligned with a funnel shift).  Strip 0 also writes the header; the last strip also combines the Adler partials -- every
//        term is known from the strip's index, so it is a plain sum -- and writes the closing block, the checksum and the stream's length.
//
// No global atomics and no arrival counters, integer arithmetic only: the same image gives the same bytes on every call, stream and batch size.
#include "cfen_image.hpp"

namespace {

constexpr int PNG_MAX_STRIP = 32768;                     // filtered bytes per strip; also the longest scanline taken
constexpr int PNG_OUT_WORDS = (PNG_MAX_STRIP + 16) / 4;  // a strip's bytes never exceed n + 10 (stored block + empty stored block)
constexpr int PNG_SYMS = 257;
constexpr int PNG_MAX_TABLES = 16;
constexpr int PNG_TABLE_WORDS = 384, PNG_TABLE_HEADER_WORDS = 63, PNG_TABLE_CODES_AT = 64;
constexpr unsigned PNG_ADLER = 65521u;

struct PngGeom {
  int H, W, R, S, rowb, ntab;
  long long strip_stride, out_stride;
};

CFEN_DEV unsigned abs_residual(int v) {
  v &= 255;
  return (unsigned)(v < 128 ? v : 256 - v);
}

CFEN_DEV int paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

CFEN_DEV int predict(int type, int a, int b, int c) {
  return type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : paeth(a, b, c);
}

__global__ __launch_bounds__(256) void k_png_deflate(const unsigned char* __restrict__ img, PngGeom g, const unsigned* __restrict__ tables,
                                                     unsigned* __restrict__ rec, unsigned char* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) unsigned filtw[PNG_MAX_STRIP / 4];
  __shared__ __attribute__((aligned(16))) unsigned outw[PNG_OUT_WORDS];
  __shared__ unsigned hist[PNG_SYMS], tab[PNG_SYMS];
  __shared__ unsigned red[4][PNG_MAX_TABLES + 2];
  __shared__ unsigned wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const int rb3 = 3 * g.W, rowb = g.rowb;
  const int y0 = s * g.R, rows = min(g.R, g.H - y0);
  const int n = rows * rowb;                                     // 1 .. 32768
  unsigned char* filt = reinterpret_cast<unsigned char*>(filtw);
  unsigned char* outb = reinterpret_cast<unsigned char*>(outw);

  for (int i = tid; i < PNG_SYMS; i += 256) hist[i] = 0;

  // 1. filter
  for (int r = wave; r < rows; r += 4) {
    const int y = y0 + r;
    const unsigned char* cur = img + ((long long)b * g.H + y) * rb3;
    const unsigned char* up = cur - rb3;                         // read only when y > 0
    const bool has_up = y > 0;
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int i = lane; i < rb3; i += 64) {
      const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, u = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
      s0 += abs_residual(x);
      s1 += abs_residual(x - a);
      s2 += abs_residual(x - u);
      s3 += abs_residual(x - ((a + u) >> 1));
      s4 += abs_residual(x - paeth(a, u, c));
    }
    s0 = wave_sum(s0);                                           // a lane's sum stays under 128 * 32768 / 64, the wave's under 2^22
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    s4 = wave_sum(s4);
    int type = 0;
    unsigned best = s0;
    if (s1 < best) best = s1, type = 1;
    if (s2 < best) best = s2, type = 2;
    if (s3 < best) best = s3, type = 3;
    if (s4 < best) best = s4, type = 4;
    unsigned char* dst = filt + r * rowb;
    if (lane == 0) dst[0] = (unsigned char)type;
    for (int i = lane; i < rb3; i += 64) {
      const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, u = has_up ? up[i] : 0, c = (has_up && i >= 3) ? up[i - 3] : 0;
      dst[1 + i] = (unsigned char)(x - predict(type, a, u, c));
    }
  }
  __syncthreads();

  // 2. runs: words [w0, w1) of the strip belong to this thread
  const int nw = (n + 3) >> 2;
  const int L4 = ((nw + 255) >> 8) | 1;                          // odd: <= 33 words = 132 bytes
  const int w0 = min(nw, tid * L4), w1 = min(nw, w0 + L4);
  unsigned adler_a = 0, adler_b = 0;                             // adler_b <= 132 bytes * weight 32768 * 255 = 1 102 970 880 < 2^32
  for (int w = w0; w < w1; ++w) {
    const unsigned v = filtw[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * w + j;
      if (i < n) {
        const unsigned d = (v >> (8 * j)) & 255u;
        atomicAdd(&hist[d], 1u);
        adler_a += d;
        adler_b += (unsigned)(n - i) * d;
      }
    }
  }
  adler_b %= PNG_ADLER;
  __syncthreads();

  // 3. costs.  Thread t holds symbol t; thread 0 adds the end-of-block symbol and the header
  unsigned cost[PNG_MAX_TABLES];
  {
    const unsigned h = hist[tid];
#pragma unroll
    for (int k = 0; k < PNG_MAX_TABLES; ++k) {
      unsigned c = 0;
      if (k < g.ntab) {
        const unsigned* t = tables + k * PNG_TABLE_WORDS;
        c = h * ((t[PNG_TABLE_CODES_AT + tid] >> 16) & 15u);
        if (tid == 0) c += ((t[PNG_TABLE_CODES_AT + 256] >> 16) & 15u) + min(t[0], (unsigned)(32 * PNG_TABLE_HEADER_WORDS));
      }
      cost[k] = wave_sum(c);
    }
  }
  const unsigned sum_a = wave_sum(adler_a), sum_b = wave_sum(adler_b);             // <= 64 * 33660 and 64 * 65520
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < PNG_MAX_TABLES; ++k) red[wave][k] = cost[k];
    red[wave][PNG_MAX_TABLES] = sum_a;
    red[wave][PNG_MAX_TABLES + 1] = sum_b;
  }
  __syncthreads();
  int best_k = 0;
  unsigned best_cost = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < PNG_MAX_TABLES; ++k) {
    const unsigned c = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    if (k < g.ntab && c < best_cost) best_cost = c, best_k = k;
  }
  const bool dynamic = best_cost < 8u * (unsigned)n + 40u;
  const int before = dynamic ? (int)((best_cost + 3 + 7) >> 3) : n + 6;     // bytes up to the empty stored block's 00 00 FF FF
  const int len = before + 4;                                                // <= n + 10
  const int nz = ((len + 15) >> 4) * 4;                                      // words copied out
  for (int i = tid; i < nz; i += 256) outw[i] = 0;
  const unsigned* t = tables + best_k * PNG_TABLE_WORDS;
  if (dynamic)
    for (int i = tid; i < PNG_SYMS; i += 256) tab[i] = t[PNG_TABLE_CODES_AT + i] & 0x000FFFFFu;
  __syncthreads();

  if (dynamic) {
    // 4. bit length of the run, exclusive scan over the workgroup
    unsigned bits = 0;
    for (int w = w0; w < w1; ++w) {
      const unsigned v = filtw[w];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * w + j < n) bits += tab[(v >> (8 * j)) & 255u] >> 16;
    }
    unsigned incl = bits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned base = 0;
    for (int q = 0; q < wave; ++q) base += wtot[q];
    const unsigned hdr = min(t[0], (unsigned)(32 * PNG_TABLE_HEADER_WORDS));
    const unsigned start = hdr + base + incl - bits;
    // header: whole words are nobody else's; the last, partial one is shared with thread 0's first symbols
    const int hw = (int)(hdr >> 5);
    if (tid < hw) outw[tid] = t[1 + tid];
    if (tid == hw && (hdr & 31u)) atomicOr(&outw[hw], t[1 + hw] & ((1u << (hdr & 31u)) - 1u));
    // pack
    int ow = (int)(start >> 5);
    int nb = (int)(start & 31u);
    unsigned long long acc = 0;
    bool first = true;
    for (int w = w0; w <= w1; ++w) {
      unsigned v = 0;
      int cnt = 0;
      if (w < w1) {
        v = filtw[w];
        cnt = min(4, n - 4 * w);
      } else if (tid == 255) {
        v = 256, cnt = -1;                                       // the end-of-block symbol follows the last run
      }
      for (int j = 0; j < (cnt < 0 ? 1 : cnt); ++j) {
        const unsigned e = tab[cnt < 0 ? 256u : ((v >> (8 * j)) & 255u)];
        acc |= (unsigned long long)(e & 0xFFFFu) << nb;
        nb += (int)(e >> 16);
        if (nb >= 32) {
          if (first)
            atomicOr(&outw[ow], (unsigned)acc);
          else
            outw[ow] = (unsigned)acc;
          first = false;
          ++ow;
          acc >>= 32;
          nb -= 32;
        }
      }
    }
    if (acc) atomicOr(&outw[ow], (unsigned)acc);
    if (tid == 0) {                                              // the empty stored block: its three header bits and the pad are zeros already
      atomicOr(&outw[(before + 2) >> 2], 0xFFu << (8 * ((before + 2) & 3)));
      atomicOr(&outw[(before + 3) >> 2], 0xFFu << (8 * ((before + 3) & 3)));
    }
  } else {
    if (tid == 0) {
      outb[1] = (unsigned char)(n & 255);
      outb[2] = (unsigned char)(n >> 8);
      outb[3] = (unsigned char)(~n & 255);
      outb[4] = (unsigned char)((~n >> 8) & 255);
      outb[before + 2] = 0xFF;
      outb[before + 3] = 0xFF;
    }
    for (int i = tid; i < n; i += 256) outb[5 + i] = filt[i];
  }
  __syncthreads();

  // 5. out
  const long long slot = (long long)b * g.S + s;
  uint4* dst = reinterpret_cast<uint4*>(slots + slot * g.strip_stride);
  const uint4* src = reinterpret_cast<const uint4*>(outw);
  for (int i = tid; i < (nz >> 2); i += 256) dst[i] = src[i];
  if (tid == 0) {
    const unsigned a = (red[0][PNG_MAX_TABLES] + red[1][PNG_MAX_TABLES] + red[2][PNG_MAX_TABLES] + red[3][PNG_MAX_TABLES]) % PNG_ADLER;
    const unsigned bsum = (red[0][PNG_MAX_TABLES + 1] + red[1][PNG_MAX_TABLES + 1] + red[2][PNG_MAX_TABLES + 1] + red[3][PNG_MAX_TABLES + 1]) % PNG_ADLER;
    *reinterpret_cast<uint4*>(rec + slot * 4) = make_uint4((unsigned)len, a, bsum, (unsigned)n);
  }
}

__global__ __launch_bounds__(256) void k_png_finish(const unsigned* __restrict__ rec, const unsigned char* __restrict__ slots, PngGeom g,
                                                    unsigned char* __restrict__ out, int* __restrict__ out_lengths) {
  __shared__ unsigned long long red[3][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, b = blockIdx.y;
  const unsigned* r = rec + (long long)b * g.S * 4;
  const bool last = s == g.S - 1;
  // bytes before this strip; on the last strip also the Adler sums.  The stream of strips j has
  //   A = 1 + sum_j A_j,  B = N + sum_j (B_j + A_j rem_j),  rem_j = filtered bytes after strip j,  N = all filtered bytes   (mod 65521)
  // -- Adler's combine step unrolled; B_j already weighs a byte by its distance to the end of its strip.  A term is below 2^33, a thread adds at
  // most S / 256 of them into 64 bits.
  unsigned long long off = 0, sa = 0, sb = 0;
  const long long N = (long long)g.H * g.rowb, nfull = (long long)g.R * g.rowb;
  for (int j = tid; j < (last ? g.S : s); j += 256) {
    const uint4 q = *reinterpret_cast<const uint4*>(r + 4 * j);
    if (j < s) off += q.x;
    if (last) {
      const long long end = min(N, (j + 1) * nfull);
      sa += q.y;
      sb += q.z + (unsigned long long)q.y * (unsigned long long)((N - end) % PNG_ADLER);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    off += __shfl_xor(off, m, 64);
    sa += __shfl_xor(sa, m, 64);
    sb += __shfl_xor(sb, m, 64);
  }
  if (lane == 0) red[0][wave] = off, red[1][wave] = sa, red[2][wave] = sb;
  __syncthreads();
  off = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  const int len = (int)r[4 * s];
  unsigned char* base = out + (long long)b * g.out_stride;
  unsigned char* d = base + 2 + off;
  const unsigned char* sp = slots + ((long long)b * g.S + s) * g.strip_stride;     // 16-byte aligned
  // d + head is 4-byte aligned; destination word k holds source bytes head + 4 k .. + 3, two source words funnel-shifted by the constant 8 * head
  const int head = min(len, (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3));
  const int nwords = (len - head) >> 2;
  if (tid < head) d[tid] = sp[tid];
  const unsigned* sw = reinterpret_cast<const unsigned*>(sp);
  unsigned* dw = reinterpret_cast<unsigned*>(d + head);
  for (int k = tid; k < nwords; k += 256) {
    const unsigned lo = sw[k];
    dw[k] = head ? (lo >> (8 * head)) | (sw[k + 1] << (32 - 8 * head)) : lo;      // sw[k + 1] ends below len + 4: inside the slot (n + 16)
  }
  for (int i = head + 4 * nwords + tid; i < len; i += 256) d[i] = sp[i];
  if (tid == 0 && s == 0) base[0] = 0x78, base[1] = 0x01;
  if (tid == 0 && last) {
    const unsigned a = (unsigned)((1 + red[1][0] + red[1][1] + red[1][2] + red[1][3]) % PNG_ADLER);
    const unsigned bb = (unsigned)(((unsigned long long)(N % PNG_ADLER) + red[2][0] + red[2][1] + red[2][2] + red[2][3]) % PNG_ADLER);
    unsigned char* e = d + len;
    e[0] = 0x01, e[1] = 0x00, e[2] = 0x00, e[3] = 0xFF, e[4] = 0xFF;
    e[5] = (unsigned char)(bb >> 8), e[6] = (unsigned char)(bb & 255), e[7] = (unsigned char)(a >> 8), e[8] = (unsigned char)(a & 255);
    out_lengths[b] = (int)(2 + off + len + 9);
  }
}

bool png_geom(int B, int H, int W, int ntab, PngGeom* g) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)3 * W + 1 > PNG_MAX_STRIP) return false;
  const int rowb = 3 * W + 1, R = PNG_MAX_STRIP / rowb, S = (H + R - 1) / R;
  const long long strip = (((long long)min(R, H) * rowb + 16 + 15) / 16) * 16;
  const long long stride = ((2 + (long long)H * rowb + 10LL * S + 9 + 15) / 16) * 16;
  if (stride > 0x7FFFFFF0LL) return false;                       // the stream's length is an int
  *g = PngGeom{H, W, R, S, rowb, ntab, strip, stride};
  return true;
}

inline size_t png_record_bytes(int B, int S) { return (((size_t)B * S * 16 + 255) / 256) * 256; }

}  // namespace

size_t cfen_png_workspace_bytes_impl(int B, int H, int W, size_t* strip_bytes, size_t* out_stride) {
  PngGeom g;
  if (!png_geom(B, H, W, 1, &g)) return 0;
  if (strip_bytes) *strip_bytes = (size_t)g.strip_stride;
  if (out_stride) *out_stride = (size_t)g.out_stride;
  return png_record_bytes(B, g.S) + (size_t)B * g.S * (size_t)g.strip_stride;
}

int cfen_png_deflate_impl(const unsigned char* images, int B, int H, int W, const void* tables, int n_tables, void* workspace, unsigned char* out,
                          int* out_lengths, hipStream_t s) {
  CFEN_CHECK_ARG(images && tables && workspace && out && out_lengths, "png_deflate: null pointer");
  CFEN_CHECK_ARG(B >= 1 && B <= 65535, "png_deflate: batch %d outside 1 .. 65535", B);
  CFEN_CHECK_ARG(H >= 1 && W >= 1, "png_deflate: empty image %d x %d", H, W);
  CFEN_CHECK_ARG((long long)3 * W + 1 <= PNG_MAX_STRIP, "png_deflate: a scanline of width %d (1 + 3 W bytes) is longer than the %d-byte strip", W, PNG_MAX_STRIP);
  CFEN_CHECK_ARG(n_tables >= 1 && n_tables <= PNG_MAX_TABLES, "png_deflate: %d tables outside 1 .. %d", n_tables, PNG_MAX_TABLES);
  PngGeom g;
  CFEN_CHECK_ARG(png_geom(B, H, W, n_tables, &g), "png_deflate: a %d x %d image makes a stream of 2 GiB or more", H, W);
  CFEN_CHECK_ARG(((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                 "png_deflate: images, workspace and out must be 16-byte aligned");
  CFEN_CHECK_ARG(((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(out_lengths)) & 3) == 0,
                 "png_deflate: tables and out_lengths must be 4-byte aligned");
  unsigned* rec = static_cast<unsigned*>(workspace);
  unsigned char* slots = static_cast<unsigned char*>(workspace) + png_record_bytes(B, g.S);
  const dim3 grid((unsigned)g.S, (unsigned)B);
  CFEN_LAUNCH(k_png_deflate, grid, dim3(256), 0, s, images, g, (const unsigned*)tables, rec, slots);
  CFEN_CHECK_LAUNCH("png_deflate");
  CFEN_LAUNCH(k_png_finish, grid, dim3(256), 0, s, (const unsigned*)rec, (const unsigned char*)slots, g, out, out_lengths);
  CFEN_CHECK_LAUNCH("png_finish");
  return CFEN_OK;
}
