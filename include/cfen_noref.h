/* No-reference statistics of a hazy image and its dehazed output on the device: an extension of the C ABI of libcfen_hip.so with a header of its
 * own.
 *
 * include/cfen_hip.h, include/cfen_resample.h, include/cfen_guided.h, include/cfen_colordiff.h and cfen_abi_version() are unchanged by it; the
 * conventions are the same: raw device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments and
 * CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).
 * No global atomics, no arrival counters: the same bits at every batch size, on every stream and for every byte alignment of the inputs.
 *
 * Every function declared here is run between guard bands by tests/test_hip_noref.py; tests/test_noref_host.py carries this header's ledger and
 * tests/noref_ref.py restates the definition in numpy (integers for everything but the gradient sum, float64 there).
 *
 * DEFINITION.  Inputs: `hazy` and `out`, each (B, H, W, 3) uint8, and a radius r in 0 .. 16.  For each image X of the two (side 0 = hazy,
 * side 1 = out), with R, G, B the three bytes of a pixel:
 *   luma          Y = (77 R + 150 G + 29 B + 128) >> 8, integer arithmetic; 77 + 150 + 29 = 256, so Y lies in 0 .. 255.
 *   dark channel  D(p) = min over q in the (2r + 1) x (2r + 1) window around p, clipped to the image, of min(R, G, B)(q)  (He, Sun and Tang
 *                 2009).  dark_sum = sum over p of D(p), an exact integer.
 *   histogram     hist[v] = number of pixels with Y = v, v = 0 .. 255.
 *   gradient sum  over the (H - 1)(W - 1) positions (y, x) with y < H - 1 and x < W - 1:
 *                   dx = Y[y, x + 1] - Y[y, x], dy = Y[y + 1, x] - Y[y, x], g = sqrt(0.5 * (dx^2 + dy^2))
 *                 with dx^2 + dy^2 an exact integer, the product with 0.5 and the square root in fp64 (correctly rounded, no fast-math);
 *                 grad_sum = sum of g in fp64 in a fixed order (below); 0 when H == 1 or W == 1.
 * and for the pair:
 *   sat_in        number of pixels with Y_hazy in {0, 255}
 *   sat_new       number of pixels with Y_out in {0, 255} and Y_hazy not in {0, 255}  (the numerator of sigma of Hautiere et al. 2008)
 *
 * OUTPUTS.  counts (B, 2, 259) uint64: counts[b][s][0 .. 255] = hist of side s, counts[b][s][256] = dark_sum of side s, counts[b][s][257] =
 * sat_in for s = 0 and sat_new for s = 1, counts[b][s][258] = 0 (reserved).  grad (B, 2) fp64: grad_sum of side s.  dark_hazy / dark_out, each
 * NULL or (B, H, W) uint8: the map D of that side.  The scores (metrics.noref_from_stats) are formed on the host in float64.
 *
 * LAUNCHES AND ORDER.  Two launches.
 *   1. One workgroup (256 threads) per tile of CFEN_NOREF_TILE_W x CFEN_NOREF_TILE_H pixels of one image pair, tiles in row-major order.  It
 *      reads the tile of both images once with a halo of r pixels (one pixel to the right and below where r = 0), clipped to the image; keeps
 *      min(R, G, B) and Y in LDS; takes the row minimum, then the column minimum; builds both histograms, dark_sum and the saturation counts
 *      with LDS integer atomics (integers: the order does not matter).  Thread t owns the tile pixels i = t, t + 256, ... (row i / TILE_W,
 *      column i % TILE_W) and adds their g in that order in fp64; the 64 sums of a wave are added by a shuffle butterfly (offsets 32, 16, ..,
 *      1), the four waves' sums in wave order ((w0 + w1) + w2) + w3.  The workgroup writes ONE record of CFEN_NOREF_RECORD_BYTES bytes to
 *      scratch: uint32 [2][258] (256 bins, dark_sum, sat of each side) followed by fp64 [2] (the two gradient partials).
 *   2. Per image and side: every integer column is the sum of the records' entries (uint64); the gradient sum is formed as thread t adding the
 *      partials of records t, t + 256, ... in that order, then a fixed tree over the 256 threads (stride 128, 64, .., 1).
 * Bytes are fetched with dword loads wherever four consecutive pixels lie inside the image: a group of four pixels whose first linear index p
 * satisfies p = address of the image's first byte (mod 4) starts on a 4-byte boundary, so the grouping is chosen per image at run time from
 * the alignment of its first byte; single-byte loads at the ends.  Both paths deliver the same bytes. */
#ifndef CFEN_NOREF_H
#define CFEN_NOREF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_NOREF_TILE_W 64
#define CFEN_NOREF_TILE_H 64
#define CFEN_NOREF_RECORD_BYTES 2080 /* 2 * 258 * 4 + 2 * 8 */
#define CFEN_NOREF_MAX_RADIUS 16

/* Bytes of scratch cfen_noref_u8 needs: B * ceil(H / CFEN_NOREF_TILE_H) * ceil(W / CFEN_NOREF_TILE_W) * CFEN_NOREF_RECORD_BYTES.
 * 0 when B is outside 1 .. 65535, H or W outside 1 .. 65536 or radius outside 0 .. 16. */
size_t cfen_noref_bytes(int B, int H, int W, int radius);

/* hazy, out: (B, H, W, 3) uint8, no alignment needed.  scratch: cfen_noref_bytes(B, H, W, radius) bytes, 8-byte aligned; its contents on entry
 * do not matter.  counts: B * 2 * 259 uint64, 8-byte aligned.  grad: B * 2 doubles, 8-byte aligned.  dark_hazy, dark_out: NULL or (B, H, W)
 * uint8, no alignment needed.  Two launches.
 * CFEN_ERR_ARG, and nothing is launched or written, for: B outside 1 .. 65535, H or W outside 1 .. 65536, radius outside 0 .. 16, a NULL hazy,
 * out, scratch, counts or grad, a misaligned scratch, counts or grad. */
int cfen_noref_u8(const unsigned char* hazy, const unsigned char* out, int B, int H, int W, int radius, void* scratch,
                  unsigned long long* counts, double* grad, unsigned char* dark_hazy /* may be NULL */, unsigned char* dark_out /* may be NULL */,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
