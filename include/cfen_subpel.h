/* Sub-pixel motion compensation for the temporal stabilisation: the block vectors of include/cfen_motion.h refined to half or quarter pixels, and
 * the warp that fetches between pixels.  An extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, the other extension headers (include/cfen_motion.h and include/cfen_temporal.h among them) and cfen_abi_version() are
 * unchanged by it; the conventions are those of include/cfen_motion.h: raw device pointers, no allocation, no synchronisation, 0 on success,
 * CFEN_ERR_ARG (-1) for bad arguments -- before any launch -- and CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(),
 * launches on `stream` (a hipStream_t; NULL = the default stream).  No atomics, no counters.
 *
 * Every function declared here is run between guard bands by tests/test_hip_subpel.py; tests/test_subpel_host.py carries this header's ledger
 * and tests/subpel_ref.py restates the definition in numpy.
 *
 * DEFINITION.  The search of include/cfen_motion.h finds one WHOLE-pixel vector per block at the working resolution h x w, which is 1 / S of the
 * frame: a camera that moves a few full-resolution pixels per frame moves a fraction of a working pixel, every block is misaligned by up to
 * half a pixel, and the blend's motion test switches the recursion off on every edge.  Here the vectors are refined to 1 / Q pixel and the
 * previous frame and the state are fetched bilinearly.  All quantities live at the working resolution h x w.
 *
 * VECTORS.  Units are quarter pixels.  Q in {2, 4} is the refinement (`subpel`).
 *
 * SAMPLING the previous frame at a quarter-pixel position (y4, x4) (integers, may be negative):
 *         y0 = y4 >> 2 (arithmetic shift, i.e. the floor) and fy = y4 & 3; the same for x.
 *         The four taps are p00 = I_{t-1}(clamp(y0), clamp(x0)), p01 at clamp(x0+1), p10 at clamp(y0+1), and p11 at both; each coordinate is
 *         clamped to the frame on its own.
 *         S(y4, x4, c) = ((4-fy)(4-fx)*p00 + (4-fy)*fx*p01 + fy*(4-fx)*p10 + fy*fx*p11 + 8) >> 4
 * S is an exact integer in 0..255.  At fy = fx = 0 it is the pixel itself.
 *
 * REFINEMENT.  It is exhaustive, so there is exactly one right answer.  Take block b with whole-pixel vector v0 = (dy, dx) from
 * cfen_motion_search_u8; each component is read clamped to +-2048 so that the result fits int16.
 *         The candidates are v4 = 4*v0 + (ey, ex)*(4/Q) for ey, ex in -(Q-1) .. Q-1: 9 candidates at Q = 2 and 49 at Q = 4, all within
 *         +-3/4 pixel of v0.
 *         SAD4(v4) = sum_{p in block} sum_c |I_t(p, c) - S(4p + v4, c)|                    below 2^20
 *         cost4(v4) = 64*SAD4 + bias*(|dy4| + |dx4|)*3*n_b                                 below 2^28 for the vectors the search writes (at most
 *                                                                                         16 pixels); for a whole-pixel candidate it is 4 x the
 *                                                                                         cost of include/cfen_motion.h
 * The block's vector is the candidate with the lexicographically smallest (cost4, |dy4| + |dx4|, dy4, dx4).  Partial edge blocks count only their
 * n_b valid pixels.  Everything is integer.
 *
 * WARP.  For pixel p in block b, with (y4, x4) = 4p + v4_b:
 *         prev_out(p, c) = S(4p + v4_b, c)
 *         and for each of the six state floats, in fp32 with fx = (x4 & 3)/4 and fy = (y4 & 3)/4 (both exact) and s00 .. s11 the state at the
 *         four taps:
 *                 t0 = s00 + fx*(s01 - s00)
 *                 t1 = s10 + fx*(s11 - s10)
 *                 state_out = t0 + fy*(t1 - t0)
 * A multiply and the add after it may fuse.  Nothing else about the order is free.
 *
 * THE RECURSION is that of include/cfen_motion.h with `refine` after `search` and this warp in place of cfen_motion_warp:
 *   1 v = search(I_t, I_{t-1});  1' v4 = refine(I_t, I_{t-1}, v);
 *   2 (I^w, S^w) = warp_subpel(v4, I_{t-1}, S_{t-1});
 *   3 the existing cfen_temporal_blend with B = 1, unchanged: guide = I_t, prev_guide = I^w, state = S^w (in place), have_state = 1;
 *   4 S^w is now S_t.
 *
 * Three consequences are exact:
 *   a vec4 whose entries are all multiples of 4 makes the warp equal to cfen_motion_warp with vec4/4 (the state is finite, so
 *     0*(s01 - s00) adds exactly);
 *   identical consecutive hazy frames give SAD4(0) = 0, which wins every tie: the run then equals the whole-pixel and the uncompensated run;
 *   the result does not depend on how frames are grouped into batches.
 *
 * Not here: a longer interpolation filter, the warp fused into the blend, sub-pixel vectors for the flicker score of include/cfen_flicker.h
 * (which keeps its own whole-pixel search), streams of more than 8 bits. */
#ifndef CFEN_SUBPEL_H
#define CFEN_SUBPEL_H

#ifdef __cplusplus
extern "C" {
#endif

/* The refinement for B consecutive frames in ONE launch: guide = I (B, h, w, 3) uint8, prev_guide (h, w, 3) uint8 and vec (B, bh, bw, 2) int16 as
 * cfen_motion_search_u8 writes it (any int16 is safe: read clamped to +-2048, coordinates clamped to the frame) -> vec4 (B, bh, bw, 2) int16 =
 * (dy4, dx4) in quarter pixels and sad4 (B, bh, bw) int32 = SAD4 of the winner.  The predecessor of frame k is frame k - 1 of the call, of frame 0
 * it is prev_guide; the frames are independent.  guide and prev_guide need no alignment; vec, vec4 and sad4 are 4-byte aligned.
 * block in {8, 16, 32}; subpel in {2, 4}; bias 0 .. 255; h, w in 1 .. 16384; B in 1 .. 65536; no two of guide, prev_guide, vec, vec4 and sad4 may
 * overlap. */
int cfen_motion_refine_u8(const unsigned char* guide, const unsigned char* prev_guide, const short* vec, int B, int h, int w, int block, int subpel,
                          int bias, short* vec4, int* sad4, void* stream);

/* The warp of ONE frame: vec4 (bh, bw, 2) int16 in quarter pixels (any int16 is safe), prev_guide (h, w, 3) uint8 and state (h, w, 6) fp32 ->
 * prev_out (h, w, 3) uint8 and state_out (h, w, 6) fp32.  One launch.  state and state_out are 16-byte aligned, vec4 is 4-byte aligned, prev_guide
 * and prev_out need no alignment.  block in {8, 16, 32}; h, w in 1 .. 16384.  No two of vec4, prev_guide, state, prev_out and state_out may
 * overlap. */
int cfen_motion_warp_subpel(const short* vec4, const unsigned char* prev_guide, const float* state, int h, int w, int block, unsigned char* prev_out,
                            float* state_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
