/* Planar YCbCr frames of 9 to 16 bits per sample (the payload of a deep YUV4MPEG2 stream: C420p10, C444p12, Cmono16, ...) <-> planar float32 RGB
 * in [-1, 1] on the device: an extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, every other header and cfen_abi_version() are unchanged by it; the conventions are those of include/cfen_yuv.h: raw device
 * pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments and CFEN_ERR_HIP (-2) for a failed launch with the
 * message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).  One launch each, no workspace, no atomics, no
 * scratch memory: the same bits at every batch size, on every stream and for every frame stride.
 *
 * Every function declared here is run between guard bands by tests/test_hip_yuv16.py; tests/test_yuv16_host.py carries this header's ledger and
 * tests/yuv16_ref.py restates the definition in numpy.
 *
 * DEFINITION.
 *
 * Samples and frame layout
 * - Samples are unsigned 16-bit little-endian, `depth` d in 9..16, value in the low d bits.
 * - A stored value above 2^d - 1 is read as 2^d - 1.
 * - Frame layout and chroma geometry are those of include/cfen_yuv.h, with two bytes per sample.
 * - s = d - 8, top = 2^d - 1, chroma centre c = 1 << (d - 1).
 * - The luma offset oy is 16 << s for limited range and 0 for full range.
 * - The RGB full scale peak is 255 << s for limited range and top for full range.
 *
 * Tables
 * - Tables are in units of 2^-20, built by yuv.tables(matrix, full_range, shift=20).
 * - The rule is the one of the 8-bit tables: rint, with forward row sums repaired on the largest entry so that the luma row sums to
 *   round(ys/255 * 2^20) and the chroma rows to 0.
 * - 14-bit coefficients would be off by up to 6 levels at 16 bits.
 * - At 2^-20 the integer result is within 0.5 + 3 top 2^-21 of float64.  That is at most 0.594 at 16 bits and 0.501 at 10 bits.
 *
 * Arithmetic
 * - All sums are 64-bit integers.  The inverse sums reach 38 bits at d = 16, so 32-bit sums overflow.
 * - >> is an arithmetic shift.
 *
 * To RGB
 * - q[k] = clamp((inv[k] . (Y - oy, Cb' - c, Cr' - c) + 2^19) >> 20, 0, peak).
 * - Cb', Cr' are brought to 4:4:4 by exactly the integer rule of cfen_yuv.h ((sum wy wx c + 8) >> 4, the same taps per format).
 * - The float written is (float)(2q - peak) / (float)peak: one correctly rounded fp32 division.
 * - The output is planar (B,3,H,W) float32, the layout the generator takes.
 * - Mono uses Cb' = Cr' = c.
 *
 * From RGB
 * - The input is (B,3,H,W) float32.
 * - t = x * 0.5f + 0.5f.  This is exact up to one rounding whether or not it is contracted to an FMA.
 * - t = min(max(t, 0), 1), with NaN -> 0.
 * - q = (int)rintf(t * (float)peak), half to even.
 * - This rounds to nearest, unlike the truncation of tensor2im (util/util.py of the reference, cfen_tensor2im_u8 here): there is no reference
 *   for deep output, and rounding is right -- truncation biases every sample down by half a level on average.
 * - d[k] = clamp((fwd[k] . (R,G,B) + (o_k << 20) + 2^19) >> 20, 0, top) with o = oy, c, c.
 * - Y = d[0].
 * - The chroma planes come from the values d[1], d[2] by the same down filters as cfen_yuv.h (two roundings, same order).
 *
 * THREAD-TO-PIXEL LAYOUT.  One launch each, workgroups of 256 threads, grid (blocks per frame, B).
 *   cfen_yuv16_to_rgb_f32   a thread owns four consecutive LINEAR pixel indices p .. p + 3 of one frame.  The groups start where the first float
 *                           plane of the frame is on a 16-byte boundary (chosen per frame at run time): the four floats of a plane leave as one
 *                           16-byte store when that plane's address is aligned, as four dword stores otherwise; the four luma samples (and the
 *                           Cb, Cr samples of 4:4:4) come as one 8-byte load when their address is aligned, as four 2-byte loads otherwise.  A
 *                           group inside one row reads the chroma columns its pixels share (two rows for 4:2:0) once.  Groups over a row end or
 *                           the frame's ends go pixel by pixel.  Both ways compute the same bits.
 *   cfen_rgb_f32_to_yuv16   the first blocks of a frame own the luma plane the same way: four linear pixels per thread, 16-byte loads per float
 *                           plane where aligned, one 8-byte store of Y (and of Cb, Cr for 4:4:4) where aligned.  The remaining blocks own the
 *                           subsampled chroma planes: a block works on one chroma row, a thread on two neighbouring samples (i, i + 1) of both
 *                           planes, i.e. on the pixels 2i .. 2i + 3 (+ 2i - 1 for the co-sited filters) of one or two image rows, 16-byte loads
 *                           where aligned and inside the row (the pairing is shifted by one sample per row when that makes it so); the two samples
 *                           of a plane leave as one 4-byte store where aligned.  Every output sample is written by exactly one thread. */
#ifndef CFEN_YUV16_H
#define CFEN_YUV16_H

#include <stddef.h>

#include "cfen_yuv.h" /* CFEN_YUV_420JPEG .. CFEN_YUV_MONO, CFEN_YUV_MAX_EDGE, CFEN_YUV_MAX_BATCH */

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_YUV16_MIN_DEPTH 9
#define CFEN_YUV16_MAX_DEPTH 16
#define CFEN_YUV16_MAX_COEF (1 << 22)

/* passed BY VALUE: nothing of it lives in device memory */
typedef struct cfen_yuv16_table {
  int coef[9];      /* 3 x 3, row-major, units of 2^-20, each within +-2^22: the forward table for cfen_rgb_f32_to_yuv16, the inverse for the other */
  int luma_offset;  /* oy: 16 << (depth - 8) limited range, 0 full range */
  int peak;         /* the RGB full scale: 255 << (depth - 8) limited range, 2^depth - 1 full range */
  int depth;        /* 9 .. 16 */
  int reserved[4];  /* must be 0 */
} cfen_yuv16_table;

/* Payload bytes of one frame: 2 (H W + 2 Hc Wc), twice cfen_yuv_frame_bytes.  0 when H or W is outside 1 .. 65536 or chroma is not one of
 * CFEN_YUV_*. */
size_t cfen_yuv16_frame_bytes(int H, int W, int chroma);

/* frames: B frames, frame_stride bytes apart; rgb: (B, 3, H, W) float32.  One launch.
 * CFEN_ERR_ARG, and nothing is launched or written, for: a NULL frames or rgb, B outside 1 .. 65535, H or W outside 1 .. 65536, an unknown
 * chroma, a depth outside 9 .. 16, a peak outside 1 .. top, a luma_offset outside 0 .. top, a coefficient outside -2^22 .. 2^22, a nonzero
 * reserved word, frame_stride < cfen_yuv16_frame_bytes(H, W, chroma), an odd frames pointer or frame_stride (samples are 2-byte aligned; a y4m
 * payload always is), an rgb pointer that is not 4-byte aligned. */
int cfen_yuv16_to_rgb_f32(const void* frames, size_t frame_stride, int B, int H, int W, int chroma, cfen_yuv16_table table, float* rgb,
                          void* stream);

/* rgb: (B, 3, H, W) float32; frames: B frames, frame_stride bytes apart.  Writes every payload byte of every frame and no byte of the
 * frame_stride - frame_bytes gap behind it.  One launch.  The same argument errors. */
int cfen_rgb_f32_to_yuv16(const float* rgb, int B, int H, int W, int chroma, cfen_yuv16_table table, void* frames, size_t frame_stride,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
