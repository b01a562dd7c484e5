/* Flicker along the motion: how much a stream of frames changes from one frame to the next where the hazy input itself did not change, measured
 * along block vectors.  An extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, the other extension headers (include/cfen_motion.h and include/cfen_temporal.h among them) and cfen_abi_version() are
 * unchanged by it; the conventions are those of include/cfen_noref.h and include/cfen_motion.h: raw device pointers, no allocation, no
 * synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments -- before any launch -- and CFEN_ERR_HIP (-2) for a failed launch with the
 * message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).  No global atomics, no arrival counters.
 *
 * Every function declared here is run between guard bands by tests/test_hip_flicker.py; tests/test_flicker_host.py carries this header's ledger
 * and tests/flicker_ref.py restates the definition in numpy.
 *
 * DEFINITION.  All frames are at the working resolution h x w of temporal.working_size(H, W, down): down = 1 takes the frames as they are,
 * otherwise ops.resample_u8(., (h, w), filter="box") is used, as Stabiliser does.
 *   I_t   the hazy guide, (h, w, 3) uint8
 *   F_t   a target frame of the same shape: the network's bytes, or the bytes that leave
 *   Bk    in {8, 16, 32}, the block edge
 *   v_b   = (dy, dx), the int16 vector of the block b that holds pixel p; a NULL vec means all zeros
 *   q     = p + v_b; it is NOT clamped
 *   tol   in 0 .. 255, the tolerance
 * Per pixel p of frame t:
 *   covered(p) <=> q lies inside the frame
 *   dI(p) = sum_c |I_t(p, c) - I_{t-1}(q, c)|         defined for covered pixels
 *   dF(p) = sum_c |F_t(p, c) - F_{t-1}(q, c)|         defined for covered pixels
 *   eF(p) = sum_c (F_t(p, c) - F_{t-1}(q, c))^2       defined for covered pixels
 *   matched(p) <=> covered(p) and dI(p) <= 3 * tol
 * The mask depends on the hazy input only, so every target scored on the same clip is compared over the same pixels.
 *
 * Per frame the call writes eight uint64 values:
 *   0 n_cov   1 n_match   2 sum_matched dI   3 sum_matched dF   4 sum_matched eF   5 sum_covered dF   6 sum_covered dI   7 0 (reserved)
 * The predecessor of frame k of a call is frame k - 1 of that call; for frame 0 it is prev_guide / prev_tgt.  The B frames are independent, so
 * one call on n frames is bitwise n calls of one frame.  Any int16 in vec is safe: a source outside the frame is simply uncovered.
 *
 * The host forms the scores in float64 (flicker.scores_from_sums):
 *   flicker = sums[3] / (3 * sums[1])                 in levels
 *   hazy    = sums[2] / (3 * sums[1])                 the floor that motion and noise leave in the input
 *   ewarp   = sums[4] / (3 * sums[1] * 255^2)         the warping error of Lai et al. 2018 on the [0, 1] scale
 *   covered = sums[0] / (h * w)       matched = sums[1] / (h * w)
 * All scores are nan where n_match = 0.  A frame pair with matched < 0.5 is a cut: it is marked in its row and left out of every pooled mean.
 * Pooled means over a clip are sum_rows sums[k] / (3 * sum_rows sums[1]) over the rows that are no cut.
 *
 * HOW IT IS COMPUTED.  Everything is integer, so there is exactly one right answer and it is the same bits on every run, stream and batch size.
 *   1. A workgroup of 256 threads takes one tile of CFEN_FLICKER_TILE x CFEN_FLICKER_TILE pixels of one frame; tiles start at multiples of 64,
 *      so every block of 8, 16 or 32 pixels lies inside one tile.  It writes ONE record of CFEN_FLICKER_RECORD_BYTES bytes to scratch: eight
 *      uint32 in the order of the table above.  The TILE is sized for the type: a tile holds at most 4096 pixels, and the largest entry, sum
 *      eF of an all-0 frame against an all-255 frame, is 4096 * 3 * 255^2 = 799 027 200 < 2^32.
 *   2. Per frame: entry k of sums is the sum of entry k of the frame's records, in uint64.
 * The p side is contiguous: its bytes are fetched with dword loads wherever four consecutive pixels lie inside the frame, in groups of four
 * linear pixel indices whose first index satisfies p = address of the guide frame's first byte (mod 4) -- such a group starts on a 4-byte
 * boundary -- so the grouping is chosen per frame at run time; the target frame uses dword loads on the same groups when its first byte has the
 * same address (mod 4), single bytes otherwise; single bytes at the ends.  The gathered q side uses byte loads.  All paths give the same sums. */
#ifndef CFEN_FLICKER_H
#define CFEN_FLICKER_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_FLICKER_TILE 64
#define CFEN_FLICKER_RECORD_BYTES 32 /* 8 * 4 */

/* Bytes of scratch cfen_flicker_u8 needs: B * ceil(h / 64) * ceil(w / 64) * CFEN_FLICKER_RECORD_BYTES.  0 when B is outside 1 .. 65536, h or w
 * outside 1 .. 16384, or the B frames hold more than 2^31 - 1 tiles (too many for one launch). */
size_t cfen_flicker_bytes(int B, int h, int w);

/* guide, tgt: (B, h, w, 3) uint8; prev_guide, prev_tgt: (h, w, 3) uint8; none needs any alignment.  vec: NULL or (B, bh, bw, 2) int16 with
 * bh = ceil(h / block), bw = ceil(w / block), 4-byte aligned.  scratch: cfen_flicker_bytes(B, h, w) bytes, 8-byte aligned; sums: B * 8 uint64,
 * 8-byte aligned; what scratch and sums hold on entry does not matter.  h, w in 1 .. 16384; B in 1 .. 65536; block in {8, 16, 32}; tol in
 * 0 .. 255.  tgt may be the same pointer as guide, and prev_tgt the same as prev_guide: that scores the input against itself; the inputs may
 * overlap each other in any way.  The outputs, scratch and sums, may overlap nothing.  Two launches.
 * CFEN_ERR_ARG, and nothing is launched or written, for anything else. */
int cfen_flicker_u8(const unsigned char* guide, const unsigned char* prev_guide, const unsigned char* tgt, const unsigned char* prev_tgt,
                    const short* vec /* may be NULL */, int B, int h, int w, int block, int tol, void* scratch, unsigned long long* sums,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
