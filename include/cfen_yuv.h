/* Planar YCbCr frames (the payload of a YUV4MPEG2 stream) <-> interleaved RGB bytes on the device: an extension of the C ABI of libcfen_hip.so
 * with a header of its own.
 *
 * include/cfen_hip.h, include/cfen_resample.h, include/cfen_guided.h, include/cfen_colordiff.h, include/cfen_noref.h and cfen_abi_version()
 * are unchanged by it; the conventions are the same: raw device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1)
 * for bad arguments and CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t;
 * NULL = the default stream).  No floating point, no atomics, no scratch memory, no workspace: the same bits at every batch size, on every
 * stream and for every byte alignment of either buffer.
 *
 * Every function declared here is run between guard bands by tests/test_hip_yuv.py; tests/test_yuv_host.py carries this header's ledger and
 * tests/yuv_ref.py restates the definition in numpy.
 *
 * FRAME LAYOUT.  A frame is H x W luma bytes followed, for every format but mono, by the Cb and then the Cr plane of Hc x Wc bytes each, with no
 * padding: the payload of a FRAME of a .y4m file as it is.  Wc = (W + 1) >> 1 for the 4:2:0 formats and 4:2:2, W for 4:4:4; Hc = (H + 1) >> 1
 * for the 4:2:0 formats, H otherwise.  Odd sizes are legal.  Frame b of a batch starts at frames + b * frame_stride.
 *
 * DEFINITION.  All arithmetic is on 32-bit integers, >> is an arithmetic shift, clamp(v) = min(max(v, 0), 255).  t = table.coef is a 3 x 3
 * matrix in units of 2^-14, row-major; oy = table.luma_offset.
 *   to RGB     R|G|B   = clamp((t[k] . (Y - oy, Cb' - 128, Cr' - 128) + 8192) >> 14), with Cb', Cr' the chroma planes brought to 4:4:4:
 *              c' = (sum wy wx c + 8) >> 4 over two rows and two columns of the plane, weights in quarters:
 *                vertical    4:2:0, j = y >> 1:  y even: rows (max(j - 1, 0), j), weights (1, 3);  y odd: rows (j, min(j + 1, Hc - 1)), (3, 1)
 *                            4:2:2, 4:4:4:       row y, weight 4
 *                horizontal  CFEN_YUV_420JPEG (centre-sited): the vertical rule applied to x
 *                            CFEN_YUV_420MPEG2, CFEN_YUV_422 (co-sited), i = x >> 1:  x even: column i, weight 4;  x odd: columns
 *                            (i, min(i + 1, Wc - 1)), weights (2, 2)
 *                            CFEN_YUV_444: column x, weight 4
 *              CFEN_YUV_MONO: Cb' = Cr' = 128.
 *   from RGB   d = clamp((t[k] . (R, G, B) + (o << 14) + 8192) >> 14) per pixel, o = oy, 128, 128 for k = 0, 1, 2.  Y = d[0].  The chroma
 *              planes come from the BYTES d[1], d[2] (two roundings, in this order):
 *                CFEN_YUV_420JPEG    (sum over dy, dx in {0, 1} of d[min(2j + dy, H - 1)][min(2i + dx, W - 1)] + 2) >> 2
 *                co-sited row filter h[y][i] = d[y][max(2i - 1, 0)] + 2 d[y][2i] + d[y][min(2i + 1, W - 1)]
 *                CFEN_YUV_420MPEG2   (h[min(2j, H - 1)][i] + h[min(2j + 1, H - 1)][i] + 4) >> 3
 *                CFEN_YUV_422        (h[y][i] + 2) >> 2
 *                CFEN_YUV_444        d itself;  CFEN_YUV_MONO writes Y only.
 *
 * THREAD-TO-PIXEL LAYOUT.  One launch each, workgroups of 256 threads, grid (blocks per frame, B).
 *   cfen_yuv_to_rgb_u8   a thread owns four consecutive LINEAR pixel indices p .. p + 3 of one frame (p = y W + x; a group may run over the end
 *                        of a row).  The groups start at p = address of the frame's first RGB byte (mod 4), chosen per frame at run time: then
 *                        the group's twelve RGB bytes start on a 4-byte boundary and leave as three dword stores; its four luma bytes come as one
 *                        dword load when their address is aligned as well, as four byte loads otherwise.  A group inside one row reads the four
 *                        chroma columns (two rows for 4:2:0) its pixels share, once.  Groups that cross a row end or the frame's ends go pixel by
 *                        pixel with byte accesses.  Both ways compute the same bytes.
 *   cfen_rgb_to_yuv_u8   the first blocks of a frame own the luma plane the same way: four linear pixels per thread, the groups chosen so that
 *                        the twelve RGB bytes come as three dword loads; the four Y bytes (and, for 4:4:4, Cb and Cr bytes) leave as one dword
 *                        store per plane whose address is aligned, as byte stores otherwise.  The remaining blocks own the subsampled chroma
 *                        planes: a block works on one chroma row, a thread on two neighbouring samples (i, i + 1) of both planes, i.e. on the
 *                        pixels 2i .. 2i + 3 of one or two image rows, read as three dwords per row where that address is aligned and inside the
 *                        row (the pairing is shifted by one sample per row when that makes it so), by bytes otherwise, plus the pixel 2i - 1 for
 *                        the co-sited filters.  Every output byte is written by exactly one thread. */
#ifndef CFEN_YUV_H
#define CFEN_YUV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_YUV_420JPEG 0  /* C420jpeg: 4:2:0, chroma sited between the pixels both ways (JPEG, MPEG-1) */
#define CFEN_YUV_420MPEG2 1 /* C420mpeg2: 4:2:0, chroma on the even columns, between the rows */
#define CFEN_YUV_422 2      /* C422: chroma on the even columns of every row */
#define CFEN_YUV_444 3      /* C444 */
#define CFEN_YUV_MONO 4     /* Cmono: luma only */
#define CFEN_YUV_MAX_EDGE 65536
#define CFEN_YUV_MAX_BATCH 65535

/* passed BY VALUE: nothing of it lives in device memory */
typedef struct cfen_yuv_table {
  int coef[9];      /* 3 x 3, row-major, units of 2^-14: the forward table for cfen_rgb_to_yuv_u8, the inverse table for cfen_yuv_to_rgb_u8 */
  int luma_offset;  /* oy: 16 limited range, 0 full range */
  int reserved[6];  /* must be 0 */
} cfen_yuv_table;

/* Payload bytes of one frame: H W + 2 Hc Wc.  0 when H or W is outside 1 .. 65536 or chroma is not one of CFEN_YUV_*. */
size_t cfen_yuv_frame_bytes(int H, int W, int chroma);

/* frames: B frames, frame_stride bytes apart; rgb: (B, H, W, 3) uint8.  No alignment is needed for either.  One launch.
 * CFEN_ERR_ARG, and nothing is launched or written, for: a NULL frames or rgb, B outside 1 .. 65535, H or W outside 1 .. 65536, an unknown
 * chroma, frame_stride < cfen_yuv_frame_bytes(H, W, chroma), a nonzero reserved word, a luma_offset outside 0 .. 255 or a coefficient outside
 * -65536 .. 65536 (the 32-bit sums cannot overflow inside that range). */
int cfen_yuv_to_rgb_u8(const unsigned char* frames, size_t frame_stride, int B, int H, int W, int chroma, cfen_yuv_table table,
                       unsigned char* rgb, void* stream);

/* rgb: (B, H, W, 3) uint8; frames: B frames, frame_stride bytes apart.  Writes every payload byte of every frame and no byte of the
 * frame_stride - frame_bytes gap behind it.  One launch.  The same argument errors. */
int cfen_rgb_to_yuv_u8(const unsigned char* rgb, int B, int H, int W, int chroma, cfen_yuv_table table, unsigned char* frames,
                       size_t frame_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif
