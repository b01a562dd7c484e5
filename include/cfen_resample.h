/* PIL-exact resampling of 8-bit RGB images on the device: an extension of the C ABI of libcfen_hip.so with a header of its own.
 *
 * include/cfen_hip.h and cfen_abi_version() are unchanged by it; the conventions are the same: raw device pointers, no allocation, no
 * synchronisation, 0 on success, CFEN_ERR_ARG (-1) for bad arguments and CFEN_ERR_HIP (-2) for a failed launch with the message in
 * cfen_last_error(), launches on `stream` (a hipStream_t; NULL = the default stream).
 *
 * Every function declared here is run between guard bands by tests/test_hip_resample.py, which also carries this header's ledger. */
#ifndef CFEN_RESAMPLE_H
#define CFEN_RESAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Image.resize((W2, H2)) of PIL for B contiguous (H, W, 3) uint8 images: src (B,H,W,3) -> dst (B,H2,W2,3), byte for byte what PIL computes for
 * the filter the tables were built for (cfen_vit_dehazing_amd/resample.py: coefficients).
 *
 * A table describes one axis.  bounds: int32 (out, 2) = (xmin, n) per output index; coef: int32 (out, ksize) weights scaled by 2^22, row xx
 * valid in [0, n).  An output byte is clip((2^21 + sum_{x < n} src[xmin + x] * coef[xx][x]) >> 22, 0, 255) with an int32 accumulator and an
 * arithmetic shift.  The horizontal pass runs first and is stored as uint8; the vertical pass reads that.
 *   xbounds = xcoef = NULL, xk = 0, W2 = W : no horizontal pass        ybounds = ycoef = NULL, yk = 0, H2 = H : no vertical pass
 *   neither pass: dst is a copy of src.
 *
 * The tables are TRUSTED, they live on the device and cannot be checked here: 0 <= xmin, n >= 0, xmin + n <= the source extent of the axis,
 * n <= ksize, xmin and xmin + n do not decrease with the output index, and 255 * sum |coef[xx]| + 2^21 < 2^31 for every row (resample.py
 * guarantees all of it).  A table that breaks the first three makes the kernels read outside src.
 *
 * tmp: B*H*W2*3 bytes, read and written only when both passes run (may be NULL otherwise).  src, tmp and dst must not overlap.  No pointer
 * needs any alignment: dst may be a lane of a larger slab; wider loads and stores are chosen at run time where pitch and pointers allow.
 * B <= 65536; H, W, H2, W2 in 1 .. 65536. */
int cfen_resample_u8(const unsigned char* src, int B, int H, int W,
                     const int* xbounds, const int* xcoef, int xk, int W2,
                     const int* ybounds, const int* ycoef, int yk, int H2,
                     unsigned char* tmp, unsigned char* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
