/* LayerNorm over token rows that carry padding slots.  An extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h, the other extension headers and cfen_abi_version() are unchanged by it; the conventions are those of include/cfen_hip.h: raw
 * device pointers, no allocation, no synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments -- before any launch -- and CFEN_ERR_HIP
 * (-2) for a failed launch with the message in cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).
 *
 * The function declared here is run between guard bands by tests/test_hip_bounds.py (test_guard_bands_padnorm); tests/test_padnorm_host.py carries
 * this header's ledger and tests/padnorm_ref.py restates the definition, and the arithmetic of the kernel, in float32 on the CPU.
 *
 * WHY.  The v5 generator runs its LViT blocks on 6 / 12 / 24 channels.  Those maps live at a channel stride of 8 / 16 / 24 (16-byte pixel
 * vectors), so a token row of p * p pixels has D = p * p * cs slots of which Dn = p * p * C are real: slot s is real iff s % cs < C.  The net's
 * launch plan has always normalised such rows; cfen_layernorm of include/cfen_hip.h cannot say which slots are real, so nothing outside the net
 * could reach that path.
 *
 * DEFINITION.  For every row x of D slots, with R = {s : s % cs < C} and Dn = |R| = D / cs * C:
 *         mean = sum_{s in R} x_s / Dn            var = sum_{s in R} (x_s - mean)^2 / Dn
 *         y_s = (x_s - mean) / sqrt(var + eps) * gamma_s + beta_s      for s in R
 *         y_s = beta_s                                                for s not in R   (packing.pack_vit_shrunk gives those slots gamma = beta = 0)
 * What a padding slot of X holds is never used: not in the statistics, not in y.  Statistics are in fp32 from centred values, exactly as for
 * cfen_layernorm; no term of the size of mean^2 is ever formed.  With C == cs the call is cfen_layernorm, bit for bit. */
#ifndef CFEN_PADNORM_H
#define CFEN_PADNORM_H

#ifdef __cplusplus
extern "C" {
#endif

/* X, Y: (M, D) of dtype (0 = fp32, 1 = fp16), 16-byte aligned, row stride D; gamma, beta: D floats.  One launch.
 * Refused: C < 1, C > cs, cs < 1, D % cs != 0, and what cfen_layernorm refuses (M or D < 1, D no multiple of the 16-byte vector -- 4 fp32 or 8 fp16
 * elements -- or above 2048, a null or misaligned pointer, an unknown dtype).  X and Y may not overlap. */
int cfen_layernorm_padded(int dtype, const void* X, void* Y, const float* gamma, const float* beta, int M, int D, int cs, int C, float eps,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
