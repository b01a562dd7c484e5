/* Motion compensation for the temporal stabilisation of include/cfen_temporal.h: an extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, the other extension headers (include/cfen_temporal.h among them) and cfen_abi_version() are unchanged by it; the conventions
 * are those of include/cfen_temporal.h: raw device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments
 * -- before any launch -- and CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t;
 * NULL = the default stream).  No atomics, no counters.
 *
 * Every function declared here is run between guard bands by tests/test_hip_motion.py; tests/test_motion_host.py carries this header's ledger.
 *
 * DEFINITION.  The recursion of include/cfen_temporal.h compares frame t with frame t-1 pixel by pixel, so a moving camera switches it off
 * everywhere.  Here each block of the frame is looked up in the previous frame first, and the recursion's state and the previous hazy frame
 * are fetched from there.  All quantities live at the working resolution h x w of include/cfen_temporal.h; I_t is the (h, w, 3) uint8 hazy
 * guide of frame t.
 *
 * SEARCH.  Block edge Bk in {8, 16, 32}, range R in 1 .. 16.  There are bh = ceil(h / Bk) by bw = ceil(w / Bk) blocks; edge blocks are partial,
 * with n_b pixels.  For a block and a candidate v = (dy, dx) in [-R, R]^2:
 *         SAD(v) = sum_{p in block} sum_c |I_t(p, c) - I_{t-1}(clamp(p + v), c)|          each coordinate clamped to the frame; an exact integer
 *                                                                                         below 2^20
 *         cost(v) = 16 * SAD(v) + bias * (|dy| + |dx|) * 3 * n_b                           bias an integer in 0 .. 255: sixteenths of a level of
 *                                                                                         mean absolute difference per pixel of displacement;
 *                                                                                         cost stays below 2^26
 * The block's vector is the candidate with the lexicographically smallest (cost, |dy| + |dx|, dy, dx).  Everything is integer, so there is
 * exactly one right answer.
 *
 * WARP, a pure gather.  For pixel p in block b:
 *         prev_out(p) = prev_guide(clamp(p + v_b))          state_out(p, 0..5) = state(clamp(p + v_b), 0..5)
 *
 * THE COMPENSATED RECURSION.  For every frame after the first of a stream:
 *   1 v = search(I_t, I_{t-1});
 *   2 (I^w, S^w) = warp(v, I_{t-1}, S_{t-1});
 *   3 the existing cfen_temporal_blend with B = 1: guide = I_t, prev_guide = I^w, state = S^w (read and written in place), have_state = 1;
 *   4 S^w is now S_t (two state buffers, swapped).
 * The first frame is the existing have_state = 0 call.
 *
 * Two consequences are exact:
 *   a zero vector field makes the warp a copy, so the compensated step equals the uncompensated step bit for bit; in particular consecutive
 *     identical hazy frames give SAD(0) = 0, which wins every tie, and the run equals the uncompensated one bitwise;
 *   the result does not depend on how frames are grouped into batches. */
#ifndef CFEN_MOTION_H
#define CFEN_MOTION_H

#ifdef __cplusplus
extern "C" {
#endif

/* The search for B consecutive frames in ONE launch: guide = I (B, h, w, 3) uint8, prev_guide (h, w, 3) uint8 -> vec (B, bh, bw, 2) int16 = (dy, dx)
 * of every block and sad (B, bh, bw) int32 = SAD of the winner.  The predecessor of frame k is frame k - 1 of the call, of frame 0 it is
 * prev_guide; the searches of the B frames are independent.  guide and prev_guide need no alignment; vec and sad are 4-byte aligned.
 * block in {8, 16, 32}; range 1 .. 16; bias 0 .. 255; h, w in 1 .. 16384; B in 1 .. 65536; no two of guide, prev_guide, vec and sad may overlap. */
int cfen_motion_search_u8(const unsigned char* guide, const unsigned char* prev_guide, int B, int h, int w, int block, int range, int bias,
                          short* vec, int* sad, void* stream);

/* The warp of ONE frame: vec (bh, bw, 2) int16 as written above (any int16 is safe: the coordinates are clamped), prev_guide (h, w, 3) uint8 and state
 * (h, w, 6) fp32 -> prev_out (h, w, 3) uint8 and state_out (h, w, 6) fp32.  One launch.  state and state_out are 16-byte aligned, vec is 4-byte
 * aligned, prev_guide and prev_out need no alignment.  block in {8, 16, 32}; h, w in 1 .. 16384.  Inputs and outputs must not overlap, because
 * neighbouring blocks read each other's pixels: no two of vec, prev_guide, state, prev_out and state_out may overlap. */
int cfen_motion_warp(const short* vec, const unsigned char* prev_guide, const float* state, int h, int w, int block, unsigned char* prev_out,
                     float* state_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
