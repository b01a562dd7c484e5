/* Full-reference scores of a YCbCr stream against a ground-truth stream, plane by plane, on the samples as they are stored: what
 * dehaze_video.py --eval_gt reports (PSNR-Y/U/V, SSIM per plane, a temporal error).  An extension of the C ABI of libcfen_hip.so with a header
 * of its own.
 *
 * include/cfen_hip.h, every other header and cfen_abi_version() are unchanged by it; the conventions are those of include/cfen_yuv.h and
 * include/cfen_flicker.h: raw device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments -- before
 * any launch -- and CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL =
 * the default stream).  No global atomics, no arrival counters: the same bits at every batch size, on every stream and for every pointer
 * alignment and frame stride.
 *
 * Every function declared here is run between guard bands by tests/test_hip_plane_metrics.py; tests/test_planes_host.py carries this header's
 * ledger and tests/planes_ref.py restates the definition in numpy.
 *
 * INPUTS.
 * - a, b: B frames each in y4m payload layout: the Y plane H x W, then (every format but CFEN_YUV_MONO) Cb and Cr of Hc x Wc samples each, at
 *   the chroma geometry of include/cfen_yuv.h (CFEN_YUV_*): Wc = (W + 1) >> 1 for the 4:2:0 formats and 4:2:2, W for 4:4:4; Hc = (H + 1) >> 1
 *   for the 4:2:0 formats, H otherwise.  Frame k starts at a + k * stride_a (b + k * stride_b).
 * - One byte per sample at depth 8.  Two little-endian bytes at depths 9 .. 16.
 * - top = 2^depth - 1.  A stored value above top reads as top.
 * - Frame k of a (likewise of b) compares against frame k - 1 of the same buffer as its previous frame.  Frame 0 uses a_prev / b_prev, one
 *   frame each in the same layout; both NULL means that frame 0 has no previous frame.
 *
 * OUTPUT.  out is [B][3 planes][4] 8-byte words; the planes are Y, Cb, Cr in this order.
 * - word 0, uint64: SSE = sum (a - b)^2 over the plane.  Exact integer.
 * - word 1, uint64: DT = sum |(a - a_prev) - (b - b_prev)| over the plane: the temporal error, how far the output's frame-to-frame change is
 *   from the ground truth's own.  Exact integer.  0 when there is no previous frame.
 * - word 2, double: mean SSIM of the plane, with cfen_image_metrics' definition (include/cfen_hip.h) on one channel:
 *     x = (float)v / (float)top, one IEEE division;
 *     11 x 11 Gaussian window, sigma 1.5, valid convolution, C1 = 0.01^2, C2 = 0.03^2;
 *     fp32 map arithmetic, fixed-order fp64 sums, the mean over the (h - 10)(w - 10) window positions of the h x w plane.
 *   The fp32 maps are formed from the centred values x - 0.5: the variances and the covariance are those of x (a shift does not change them)
 *   and cancel less, the luminance term uses mu + 0.5.  The value defined is the same; its fp32 rounding is smaller.
 *   A plane with h < 11 or w < 11 gets NaN here.  Its integers are still written.
 * - word 3, uint64: the plane's sample count h w, or 0 for a plane the format does not have (Cb and Cr of CFEN_YUV_MONO; their SSE and DT are
 *   0 and their SSIM is NaN).
 *
 * HOW IT IS COMPUTED.  Two launches, as cfen_image_metrics.
 *   1. grid (tiles, plane, B), workgroups of 256 threads.  A workgroup owns 24 x 64 window positions of one plane of one frame pair: it stages
 *      the (24 + 10) x (64 + 10) samples under them of both frames in LDS as fp32 (zeros past the plane), and on the way adds (a - b)^2 and the
 *      temporal term of the samples the tile OWNS -- [y0, y0 + 24) x [x0, x0 + 64), the last tile row / column up to the plane's edge, so every
 *      sample is counted exactly once -- in 64-bit integers; then the row and column passes of cfen_image_metrics form its SSIM map values,
 *      summed in fp64.  A plane too small for a window still has one tile.  Per tile (ssim sum, SSE, DT) go to scratch; the chroma planes have
 *      fewer tiles than the grid is wide, and the workgroups past a plane's last tile leave at once.
 *   2. grid (3, B): one workgroup per plane adds the tiles' SSIM sums in the fixed order of cfen_image_metrics' finish (partial i to thread
 *      i % 256 in ascending i, then a tree over the threads), the integers in uint64, and writes the four words.
 * Samples are read one by one (1- or 2-byte loads, consecutive lanes on consecutive samples), so no pointer needs more than its sample's
 * alignment. */
#ifndef CFEN_PLANES_H
#define CFEN_PLANES_H

#include <stddef.h>

#include "cfen_yuv.h" /* CFEN_YUV_420JPEG .. CFEN_YUV_MONO, CFEN_YUV_MAX_EDGE, CFEN_YUV_MAX_BATCH */

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_PLANES_MIN_DEPTH 8
#define CFEN_PLANES_MAX_DEPTH 16
#define CFEN_PLANES_WORDS 12 /* 8-byte words of `out` per frame: 3 planes x 4 */

/* Bytes of scratch cfen_plane_metrics needs: 24 per tile, B * (tiles(H, W) + 2 tiles(Hc, Wc)) tiles (no chroma tiles for CFEN_YUV_MONO) with
 * tiles(h, w) = max(1, ceil((h - 10) / 24)) * max(1, ceil((w - 10) / 64)).  0 when B is outside 1 .. 65535, H or W outside 1 .. 65536,
 * H W > 2^31 or chroma is not one of CFEN_YUV_*. */
size_t cfen_plane_metrics_bytes(int B, int H, int W, int chroma);

/* a, b: B frames each, stride_a / stride_b bytes apart; a_prev, b_prev: both NULL or both set: the frame pair before frame 0.  scratch:
 * cfen_plane_metrics_bytes(B, H, W, chroma) bytes, 8-byte aligned; out: B * 12 8-byte words, 8-byte aligned; what scratch and out hold on
 * entry does not matter, and what scratch holds afterwards is of no use to the caller.  The inputs may overlap each other in any way (a
 * stream scored against itself); scratch and out may overlap nothing.  Two launches.
 * CFEN_ERR_ARG, and nothing is launched or written, for: a NULL a, b, scratch or out; exactly one of a_prev, b_prev set; B outside 1 .. 65535;
 * H or W outside 1 .. 65536; H W > 2^31 (so that the uint64 SSE cannot overflow at 16 bits); an unknown chroma; a depth outside 8 .. 16;
 * stride_a or stride_b below the frame size (H W + 2 Hc Wc samples); at a depth above 8 an odd a, b, a_prev, b_prev, stride_a or stride_b;
 * an out or scratch that is not 8-byte aligned. */
int cfen_plane_metrics(const void* a, size_t stride_a, const void* b, size_t stride_b, const void* a_prev, const void* b_prev, int B, int H,
                       int W, int chroma, int depth, void* scratch, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
