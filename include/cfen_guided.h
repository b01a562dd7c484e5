/* Guided upsampling of 8-bit RGB images on the device (He & Sun, "Fast Guided Filter"): an extension of the C ABI of libcfen_hip.so with a
 * header of its own.
 *
 * include/cfen_hip.h, include/cfen_resample.h and cfen_abi_version() are unchanged by it; the conventions are the same: raw device pointers, no
 * allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments and CFEN_ERR_HIP (-2) for a failed launch with the message
 * in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).  No atomics, no counters.
 *
 * Every function declared here is run between guard bands by tests/test_hip_guided.py, which also carries this header's ledger.
 *
 * DEFINITION.  Per image and per channel c in {R, G, B}, independently (the guide of channel c is channel c of the hazy image):
 *   inputs   I (h, w, 3) uint8: the low-resolution hazy bytes, exactly what the forward was fed
 *            P (h, w, 3) uint8: the low-resolution output
 *            G (H, W, 3) uint8: the full-resolution hazy image
 *            radius r, eps255 = eps * 255^2
 *   window   Omega(p): the (2r+1)^2 square around p, clipped to the image; N(p) is its pixel count
 *   sums     over Omega(p): S_I = sum I, S_P = sum P, S_II = sum I^2, S_IP = sum I P: exact integers, below 2^27 for r <= 16
 *            C = N S_IP - S_I S_P and V = N S_II - S_I^2, exact in int64 (below 2^37 for r <= 16)
 *   in fp32  a = float(C) / (float(V) + eps255 * float(N^2))
 *            b = (float(S_P) - a * float(S_I)) / float(N)
 *   smoothed abar(p) = (sum_{q in Omega(p)} a(q)) / N(p)        bbar(p) = (sum_{q in Omega(p)} b(q)) / N(p)
 *            (fp32; the kernel sums a window row by row, each row from left to right, then the rows from top to bottom)
 *   upsample to H x W, bilinear with half-pixel centres and edge clamp -- what F.interpolate(mode='bilinear', align_corners=False) computes.
 *            Per axis the source coordinate of output index y is the exact rational ((2y+1) h - H) / (2H), clamped below at 0, computed in
 *            INTEGERS (sizes are limited to 16384 so that int32 holds it): y0 = floor, y1 = min(y0 + 1, h - 1), fy = the remainder divided
 *            once in fp32, float(num - y0 * 2H) / float(2H).  Vertically first, per coefficient column x:
 *                cv(x) = c(y0, x) + fy * (c(y1, x) - c(y0, x))
 *            then horizontally:   Cbar = cv(x0) + fx * (cv(x1) - cv(x0))                 for c = abar and c = bbar, giving Abar and Bbar
 *   output   v = Abar * G + Bbar          dst = uint8(clamp(floor(v + 0.5), 0, 255))
 * eps is in squared units of the [0, 1] intensity scale and must be finite and > 0: with V = 0 that keeps a = 0 and never produces a NaN.
 * The compiler may fuse a multiply and the add that follows it; nothing else about the order above is free. */
#ifndef CFEN_GUIDED_H
#define CFEN_GUIDED_H

#ifdef __cplusplus
extern "C" {
#endif

/* The low-resolution half: guide = I and src = P, both (B, h, w, 3) uint8 -> coef (B, h, w, 6) fp32 = [abar_R, abar_G, abar_B, bbar_R, bbar_G,
 * bbar_B] per pixel.  tmp (B, h, w, 6) fp32 receives the unsmoothed [a_R, a_G, a_B, b_R, b_G, b_B].  Two launches.
 * tmp and coef are 16-byte aligned; guide and src need no alignment.  radius 1 .. 16; h, w in 1 .. 16384; B in 1 .. 65536; eps255 finite
 * and > 0; guide, src, tmp and coef must not overlap. */
int cfen_guided_coef_u8(const unsigned char* guide, const unsigned char* src, int B, int h, int w, int radius, float eps255,
                        float* tmp, float* coef, void* stream);

/* The full-resolution half: coef (B, h, w, 6) fp32 as written above, guide_hi = G (B, H, W, 3) uint8 -> dst (B, H, W, 3) uint8.  One launch.
 * coef is 16-byte aligned; guide_hi and dst need no alignment: dst may be a lane of a larger slab; 16-byte loads and stores are chosen at run
 * time where 3 W and both pointers allow, single bytes elsewhere.  h, w, H, W in 1 .. 16384; B in 1 .. 65536; coef, guide_hi and dst must not
 * overlap. */
int cfen_guided_apply_u8(const float* coef, int B, int h, int w, const unsigned char* guide_hi, int H, int W,
                         unsigned char* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
