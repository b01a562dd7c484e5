/* Temporal stabilisation of a dehazed video stream on the device: an extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, the other extension headers and cfen_abi_version() are unchanged by it; the conventions are those of include/cfen_guided.h:
 * raw device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments -- before any launch -- and
 * CFEN_ERR_HIP (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).
 * No atomics, no counters.
 *
 * Every function declared here is run between guard bands by tests/test_hip_temporal.py; tests/test_temporal_host.py carries this header's ledger.
 *
 * DEFINITION.  include/cfen_guided.h fits, per pixel and channel, the local affine model P ~ a I + b between the hazy bytes I and the output P.
 * Under the scattering model a = 1/t and b = -A (1 - t) / t, so smoothing (a, b) over time ties the transmission and the airlight of neighbouring
 * frames together.  The output is corrected by the CHANGE in coefficients, not replaced by a I + b: the network's own detail stays, and where
 * nothing is smoothed the bytes are the network's, bit for bit.
 *
 * For every frame t:  G_t (H, W, 3) uint8 the full-size hazy RGB bytes, Y_t (H, W, 3) uint8 the full-size dehazed RGB bytes.
 *   1 working resolution.  S an integer >= 1.  For S = 1, I_t = G_t and P_t = Y_t; otherwise both are PIL's box resize (cfen_resample_u8, the
 *     box filter) to h x w = ceil(H / S) x ceil(W / S).
 *   2 this frame's coefficients.  c_t = cfen_guided_coef_u8(I_t, P_t, radius, eps255), (h, w, 6) fp32, as include/cfen_guided.h defines them.
 *   3 motion.  Over the same clipped window Omega(p), with N(p) pixels:
 *         D_t(p) = sum_{q in Omega(p)} sum_c |I_t(q, c) - I_{t-1}(q, c)|          an exact integer, below 2^20 for r <= 16
 *     in fp32  d = float(D) / float(3 N)        keep = clamp(1 - d / motion, 0, 1)        k = strength * keep
 *   4 recursion, per pixel and per each of the six planes, in fp32:
 *         S_t = c_t + k * (S_{t-1} - c_t)          Delta_t = S_t - c_t
 *     The first frame of a stream (have_state = 0) has S_0 = c_0 and Delta_0 = 0.
 *   5 apply.  DA and DB are planes 0..2 and 3..5 of Delta_t upsampled to H x W exactly as include/cfen_guided.h upsamples: the source coordinate
 *     of output index y is ((2y+1) h - H) / (2H) clamped below at 0, in INTEGERS, y0 = floor, y1 = min(y0 + 1, h - 1), fy = the remainder divided
 *     once in fp32; vertically first, cv(x) = c(y0, x) + fy * (c(y1, x) - c(y0, x)), then horizontally cv(x0) + fx * (cv(x1) - cv(x0)).
 *         v = (float(Y_t) + DA * G_t) + DB          dst = uint8(clamp(floor(v + 0.5), 0, 255))
 * The compiler may fuse a multiply and the add that follows it; nothing else about the order above is free.
 *
 * Three consequences are exact:
 *   two identical consecutive frames (same G, same Y), the first of them the first of a stream, give Delta = 0 and dst == Y;
 *   a cut (d >= motion everywhere) gives k = 0, S_t = c_t and dst == Y;
 *   strength = 0 gives dst == Y for every input. */
#ifndef CFEN_TEMPORAL_H
#define CFEN_TEMPORAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* Steps 3 and 4 for B consecutive frames in ONE launch: guide = I (B, h, w, 3) uint8, coef = c (B, h, w, 6) fp32 -> delta (B, h, w, 6) fp32, and
 * state (h, w, 6) fp32 = S, read when have_state = 1 and always written (S of the call's last frame).  A workgroup owns 16 x 16 pixels and walks
 * the B frames in order with S in registers: the predecessor of frame k is frame k - 1 of the call, of frame 0 it is prev_guide (h, w, 3) uint8,
 * which is only read.  have_state = 0: frame 0 is the first of a stream; prev_guide (may be NULL) and what state holds are not looked at.
 * coef, state and delta are 16-byte aligned; guide and prev_guide need no alignment.  radius 1 .. 16; h, w in 1 .. 16384; B in 1 .. 65536; motion
 * finite and > 0; strength in [0, 1); have_state 0 or 1; no two of guide, prev_guide, coef, state and delta may overlap. */
int cfen_temporal_blend(const unsigned char* guide, const unsigned char* prev_guide, const float* coef, int B, int h, int w, int radius,
                        float motion, float strength, int have_state, float* state, float* delta, void* stream);

/* Step 5, the full-resolution half: delta (B, h, w, 6) fp32 as written above, guide_hi = G and src_hi = Y (B, H, W, 3) uint8 -> dst (B, H, W, 3)
 * uint8.  One launch.  delta is 16-byte aligned; guide_hi, src_hi and dst need no alignment: dst may be a lane of a larger slab; 16-byte loads
 * and stores are chosen at run time where 3 W and all three pointers allow, single bytes elsewhere.  h, w, H, W in 1 .. 16384; B in 1 .. 65536;
 * no two of delta, guide_hi, src_hi and dst may overlap. */
int cfen_temporal_apply_u8(const float* delta, int B, int h, int w, const unsigned char* guide_hi, const unsigned char* src_hi, int H, int W,
                           unsigned char* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
