/* CIEDE2000 colour difference of 8-bit sRGB images on the device: an extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, include/cfen_resample.h, include/cfen_guided.h and cfen_abi_version() are unchanged by it; the conventions are the same: raw
 * device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments and CFEN_ERR_HIP (-2) for a failed launch
 * with the message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).  No atomics, no counters: the same bits
 * at every batch size, on every stream and for every alignment of the inputs.
 *
 * Every function declared here is run between guard bands by tests/test_hip_ciede.py; tests/test_ciede_host.py carries this header's ledger and
 * tests/ciede_ref.py restates the definition in float64.
 *
 * DEFINITION.  Inputs: two (B, H, W, 3) uint8 sRGB images a (colour 1) and b (colour 2).  Per pixel of each image:
 *   1. lin[v], v = 0 .. 255: with c = v / 255, c / 12.92 if c <= 0.04045, otherwise ((c + 0.055) / 1.055)^2.4; evaluated in fp64 and rounded to
 *      fp32 once.  The caller builds the table (metrics.srgb_linear_table()) and hands it over as a device pointer.
 *   2. t = Mn (lin[R], lin[G], lin[B]) with Mn the IEC 61966-2-1 matrix
 *          0.4124564 0.3575761 0.1804375
 *          0.2126729 0.7151522 0.0721750
 *          0.0193339 0.1191920 0.9503041
 *      each row divided by its own sum ((m0 + m1) + m2) in fp64 and rounded to fp32 once: the white point is the matrix's own white, byte white
 *      is L = 100.  t_x = (Mn00 lin[R] + Mn01 lin[G]) + Mn02 lin[B], and so on.
 *   3. f(t) = cbrt(t) if t > (6/29)^3, otherwise t * 841 / 108 + 4 / 29.
 *   4. L = 116 f_y - 16, a = 500 (f_x - f_y), b = 200 (f_y - f_z).
 *   5. A pixel with R = G = B is achromatic by definition: a = b = 0 exactly (an integer test on the bytes).  Without it a grey lands at
 *      |a|, |b| ~ 6e-5 in fp32, its hue is noise, and the mean-hue term of the formula turns that into errors of 0.03 against saturated colours.
 *      The smallest chroma of any other byte colour is 0.277, at (2, 3, 3).
 * Delta E 00 follows Sharma, Wu and Dalal, "The CIEDE2000 Color-Difference Formula: Implementation Notes, Supplementary Test Data, and
 * Mathematical Observations" (2005), with kL = kC = kH = 1:
 *   C_i = sqrt(a_i^2 + b_i^2), Cbar = (C_1 + C_2) / 2, G = 0.5 (1 - sqrt(Cbar^7 / (Cbar^7 + 25^7))), a'_i = (1 + G) a_i, C'_i = sqrt(a'_i^2 + b_i^2)
 *   h'_i = atan2(b_i, a'_i) in degrees in [0, 360), and 0 where a'_i = b_i = 0
 *   dL' = L_2 - L_1, dC' = C'_2 - C'_1
 *   dh' = h'_2 - h'_1 wrapped into (-180, 180] (minus 360 above 180, plus 360 below -180); 0 where C'_1 C'_2 = 0
 *   dH' = 2 sqrt(C'_1 C'_2) sin(dh' / 2)
 *   Lbar' = (L_1 + L_2) / 2, Cbar' = (C'_1 + C'_2) / 2
 *   hbar' = (h'_1 + h'_2) / 2 if |h'_1 - h'_2| <= 180; else (h'_1 + h'_2 + 360) / 2 if h'_1 + h'_2 < 360, (h'_1 + h'_2 - 360) / 2 if not;
 *           h'_1 + h'_2 where C'_1 C'_2 = 0
 *   T = 1 - 0.17 cos(hbar' - 30) + 0.24 cos(2 hbar') + 0.32 cos(3 hbar' + 6) - 0.20 cos(4 hbar' - 63)
 *   dtheta = 30 exp(-((hbar' - 275) / 25)^2), R_C = 2 sqrt(Cbar'^7 / (Cbar'^7 + 25^7)), R_T = -sin(2 dtheta) R_C
 *   S_L = 1 + 0.015 (Lbar' - 50)^2 / sqrt(20 + (Lbar' - 50)^2), S_C = 1 + 0.045 Cbar', S_H = 1 + 0.015 Cbar' T
 *   dE = sqrt(max(0, (dL'/S_L)^2 + (dC'/S_C)^2 + (dH'/S_H)^2 + R_T (dC'/S_C) (dH'/S_H)))
 * Per pixel everything is fp32.  The compiler may fuse a multiply with the add that follows it; no fast-math, no approximate intrinsics; sines
 * and cosines of degrees are taken as sinpi / cospi of degrees / 180.
 *
 * OUTPUTS.  out[b] = (sum over the pixels of image b of the fp32 per-pixel values, in fp64 and in a fixed order) / (H W).  If `map` is not NULL,
 * map (B, H, W) fp32 receives the per-pixel values. */
#ifndef CFEN_COLORDIFF_H
#define CFEN_COLORDIFF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch cfen_ciede2000_u8 needs for B pairs of H x W images: one double per workgroup (1024 consecutive pixels of one pair).
 * 0 when B is outside 1 .. 65535 or H or W outside 1 .. 65536. */
size_t cfen_ciede2000_bytes(int B, int H, int W);

/* a, b: (B, H, W, 3) uint8, no alignment needed (dword loads are chosen at run time per image where its first byte is 4-byte aligned, single
 * bytes elsewhere and in the tail).  table: the 256 fp32 values of step 1, 4-byte aligned.  scratch: cfen_ciede2000_bytes(B, H, W) bytes, 8-byte
 * aligned; its contents on entry do not matter.  map: NULL or (B, H, W) fp32, 4-byte aligned (16-byte stores where an image's map begins on a
 * 16-byte boundary).  out: B doubles, 8-byte aligned.  Two launches.
 * CFEN_ERR_ARG, and nothing is launched or written, for: B outside 1 .. 65535, H or W outside 1 .. 65536, a NULL a, b, table, scratch or out,
 * a misaligned table, scratch, map or out. */
int cfen_ciede2000_u8(const unsigned char* a, const unsigned char* b, int B, int H, int W, const float* table, void* scratch,
                      float* map /* may be NULL */, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
