/* cfen_hip.h -- C ABI of the MI355X-native CFEN-ViT dehazing inference path (libcfen_hip.so).
 *
 * Drop-in boundary for the generator forward of phoenixtreesky7/CFEN-ViT-Dehazing
 *   models/networks_iid_hlgvit_crs_gd4_cfs_v3.py:392-1020   dec_ipt.forward
 * called by the reference at models/model_iid_dehazing.py:143 (`self.netG(self.real_B)`), plus the
 * standalone deformable-convolution operator of dcn/src/deform_conv_cuda.cpp.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the current HIP device unless stated otherwise;
 *   - `dtype` selects storage + MFMA input type: CFEN_F32 (exact fp32 MFMA) or CFEN_F16 (fp16 storage,
 *     fp32 accumulate); biases / norm parameters / affine tables are always fp32;
 *   - feature maps are NHWC with an explicit channel stride `cs`; token matrices are row-major;
 *   - padding lanes (channels C .. cs - 1 of every pixel) of an OUTPUT map: the convolutions (cfen_conv2d, cfen_head_conv5) and the input layout
 *     kernels (cfen_nchw_to_nhwc, cfen_u8hwc_to_nhwc) store the whole channel stride, and the lanes past the last channel are exact zeros
 *     (for the convolutions because packing.py zero-fills the weight rows and the scale / shift entries of the padded output channels, and
 *     given residuals whose padding is zero).  The kernels that move tokens into a map -- cfen_unpatchify, the fold outputs of cfen_mlp_block /
 *     cfen_mlp_stream_block / cfen_gemm_chain, cfen_lvit_window -- and cfen_upsample4 store the C channels only and leave the padding lanes
 *     UNTOUCHED: a caller that needs zeros there zeroes the map once.  cfen_net_forward uses them only on maps with cs == C (24 / 48 / 96
 *     channels); its maps with padding (12 channels in 16) are all written by convolutions, so the workspace needs no zeroing;
 *   - scratch and workspace contents are irrelevant before a call unless the function says otherwise (cfen_gemm_splitk's arrival counters);
 *   - all functions are asynchronous on `stream` (a hipStream_t passed as void*), allocate nothing,
 *     return 0 on success or a negative CFEN_ERR_* code; cfen_last_error() gives the message.
 *   - no exceptions cross this boundary.
 */
#ifndef CFEN_HIP_H
#define CFEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFEN_F32 0
#define CFEN_F16 1

#define CFEN_OK 0
#define CFEN_ERR_ARG (-1)   /* invalid argument / unsupported shape      */
#define CFEN_ERR_HIP (-2)   /* HIP runtime reported an error             */
#define CFEN_ERR_STATE (-3) /* missing parameter, workspace too small... */

int cfen_abi_version(void);
const char* cfen_last_error(void);
/* Process-wide tuning knobs for benchmarking kernel variants ("gemm.kernel", "net.tail_fused", ...); the defaults are what ships.
 * Every key, its shipped default, the values it takes and what they select are ONE table: cfen_vit_dehazing_amd/csrc/cfen_tune_knobs.hpp
 * (plain text rows with a comment each; ship it beside this header as the knobs' documentation -- INTEGRATION.md).  At run time the library
 * itself answers which keys exist and what their defaults are (cfen_tune_key, cfen_tune_query), and a refusal names the values a knob takes.
 * The knobs are read when a forward is enqueued or a graph is built.  None of the three calls touches the GPU; none is thread safe.
 *   cfen_tune        sets a knob.  Unknown key, or a value the knob's rule refuses: CFEN_ERR_ARG, nothing changes.  Some rules store a
 *                    normalised value (on / off knobs store value != 0, "embed.lds" stores value & 7).
 *   cfen_tune_query  reads a knob's current value and its shipped default (either pointer may be NULL); CFEN_ERR_ARG for an unknown key.
 *   cfen_tune_key    the key of knob number `index` (0, 1, ...), NULL past the last one. */
int cfen_tune(const char* key, int value);
int cfen_tune_query(const char* key, int* value, int* shipped_default);
const char* cfen_tune_key(int index);

/* ---- whole generator: replaces define_G (v3:93-100) + dec_ipt.forward (v3:392-1020) ------------- */
typedef struct cfen_net cfen_net;

typedef struct cfen_net_config {
  int32_t batch;            /* images per forward on this GPU                                   */
  int32_t n_feats;          /* options/base_options.py:110                                     */
  int32_t hidden_dim_ratio; /* options/base_options.py:104                                     */
  int32_t patch_size;       /* LViT window edge in feature-map pixels, base_options.py:96      */
  int32_t load_size;        /* edge of the half-resolution map xf, base_options.py:16          */
  int32_t num_heads;        /* base_options.py:192                                             */
  int32_t dtype;            /* CFEN_F32 | CFEN_F16                                             */
  int32_t reserved;         /* bit 0: single-lane launch plan; bits 8..15: generator variant (models/model_iid_dehazing.py:84-92):
                               0 networks_iid_hlgvit_crs_gd4_cfs_v3 (image edge 2*load_size), 1 networks_iid_hlgvit_crs_gd4_cfs
                               (full-resolution head, no ds_conv_e01 / us_conv_d01*, image edge = load_size)                    */
} cfen_net_config;

int cfen_net_create(cfen_net** out, const cfen_net_config* cfg);
void cfen_net_destroy(cfen_net* net);
/* bytes of device scratch the caller must pass to cfen_net_forward (256-byte aligned).  The workspace belongs to ONE net: the first forward on a
 * (workspace address, size) pair zeroes its synchronisation words with a launch on the caller's stream, graph capture zeroes them synchronously; the
 * caller must not write into the workspace between forwards, and hands a new net a workspace of its own (stage maps of the last forward live there:
 * cfen_net_stage). */
size_t cfen_net_workspace_bytes(const cfen_net* net);
/* register one packed parameter (layout: cfen_vit_dehazing_amd/packing.py); the pointer must stay
 * valid for the life of the net.  `nbytes` is checked against what the layer needs.               */
int cfen_net_set_param(cfen_net* net, const char* name, const void* dev_ptr, size_t nbytes);
/* ActNorm2d first-call initialisation (models/actnorm.py:25-37).  Mark `layer` (a conv / conv-transpose layer followed by
 * ActNorm2d, packing.py names) as uninitialised: the next EAGER cfen_net_forward runs it raw (`ones` [Cout_pad] of 1.0f as scale,
 * `conv_bias` [Cout_pad] as shift), takes per-channel statistics of that output over the whole batch, overwrites the layer's
 * registered "<layer>.scale" / "<layer>.shift" tables in place with the folded ActNorm epilogue and stores the raw parameters
 * an_out[0][c] = weight = -0.5 log(max(var_unbiased, 0.2)), an_out[1][c] = bias = -mean  (an_out is [2][Cout_pad] fp32), then runs the
 * layer normally -- the outputs of that forward are those of the reference's first forward.  Capture / profile refuse while
 * layers are pending.                                                                                                         */
int cfen_net_actnorm_pending(cfen_net* net, const char* layer, const float* ones, const float* conv_bias, float* an_out);
int cfen_net_actnorm_pending_count(const cfen_net* net);
/* Input format of cfen_net_forward / _graph_capture / _profile: 0 (default) x is fp32 NCHW in [-1,1]; 1: x is uint8 HWC
 * (B,H,W,3) as decoded from the image file, normalised (v/255 - 0.5)/0.5 on the device by the plan's first launch
 * (ToTensor + Normalize(0.5, 0.5), data/base_dataset.py:44-46).  Pass the uint8 pointer through the `x` argument.            */
int cfen_net_set_input_u8(cfen_net* net, int enabled);
/* Output format of cfen_net_forward / _graph_capture / _profile: 0 (default) xr / xs / xd are fp32 NCHW; 1: each of the three is uint8 HWC
 * (B,H,W,3) -- util.tensor2im of the fp32 result ((x + 1) / 2 * 255 in fp32, truncating cast, no clamp, the 1-channel xs tiled to 3;
 * util/util.py:12-24), written by the tails' last launch instead of a cfen_tensor2im_u8 pass over fp32 planes.  Pass the uint8 pointers through
 * the xr / xs / xd arguments (16-byte aligned).  CFEN_ERR_ARG when the tails do not run on the Toeplitz 7x7 kernel (fp32 nets, image edges that are
 * not multiples of 64): take fp32 outputs and cfen_tensor2im_u8 there.                                                                          */
int cfen_net_set_output_u8(cfen_net* net, int enabled);
/* enabled: the forward writes xr / xs / xd as fp16 NCHW (same shapes and [xr | xs | xd] order as the fp32 outputs, 2 bytes per element) from the fused tail launch --
 * the wire type of the sharded run's output all-gather (reference analogue: nn.DataParallel's gather, networks_iid_hlgvit_crs_gd4_cfs_v3.py:77-83), without a
 * conversion pass.  Values = the fp32 outputs rounded to nearest even.  CFEN_ERR_ARG where the tails do not run on the fused kernel (fp32 nets, image edges that
 * are not multiples of 64); cfen_net_forward then fails if the plan falls back to the separate tail launches ("net.tail_fused" != 2, "net.keep_stages").        */
int cfen_net_set_output_f16(cfen_net* net, int enabled);
/* names still missing, written as a ';'-separated list into buf; returns the count                */
int cfen_net_missing_params(const cfen_net* net, char* buf, size_t buflen);
/* x: (B,3,H,W) fp32 NCHW in [-1,1];  xr: (B,3,H,W), xs: (B,1,H,W), xd: (B,3,H,W) fp32 NCHW        */
int cfen_net_forward(cfen_net* net, const float* x, float* xr, float* xs, float* xd, void* workspace, size_t workspace_bytes,
                     void* stream);
/* The same launch plan as an explicit hipGraph: kernel nodes with dependency edges (the branches that eager mode
 * runs on internal side streams -- GViT beside LViT, S decoder beside R decoder -- become parallel graph branches).
 * All pointers are baked in; replay with cfen_net_graph_launch on any stream.  Returns an id in *graph_id.     */
int cfen_net_graph_capture(cfen_net* net, const float* x, float* xr, float* xs, float* xd, void* workspace, size_t workspace_bytes,
                           int32_t* graph_id);
int cfen_net_graph_launch(cfen_net* net, int32_t graph_id, void* stream);
/* one forward with a HIP event pair around every kernel launch on `stream` (synchronises the stream at
 * the end -- not graph-capturable).  Classes: 0 token GEMMs, 1 attention, 2 LayerNorm, 3 patchify /
 * unpatchify / upsample / layout, 4 convolutions, 5 InstanceNorm / CFSM2G, 6 fused token MLP.  Per class: summed kernel
 * milliseconds, algorithmic FLOPs (2*MAC) of those launches, number of launches.                  */
#define CFEN_NUM_KERNEL_CLASSES 7
int cfen_net_profile(cfen_net* net, const float* x, float* xr, float* xs, float* xd, void* workspace, size_t workspace_bytes,
                     void* stream, double* ms_per_class, double* flops_per_class, int32_t* launches_per_class, int nclass);
/* per-launch detail of the latest cfen_net_profile: entry `index` (launch order) -> layer / block-step label (owned by
 * the net, valid until the next profile), kernel class, algorithmic FLOPs, milliseconds.  Returns CFEN_ERR_STATE past
 * the last entry.                                                                                   */
int cfen_net_profile_entry(const cfen_net* net, int index, const char** label, int32_t* kernel_class, double* flops, double* ms);
/* ... and the DEVICE KERNEL(S) that launch ran (the kernel template as instantiated, e.g. "k_gemm_dma<T, 1, 3>"; several joined by " + ") with its
 * algorithmic bytes where the net prices it against HBM (token GEMMs: weights + tokens in + tokens out; 0 otherwise) */
int cfen_net_profile_entry_kernel(const cfen_net* net, int index, const char** kernel, double* bytes);
/* device pointer + geometry of a named top-level stage output (SURVEY Appendix D names) inside the
 * workspace of the LAST forward; NHWC, element type = net dtype.                                  */
int cfen_net_stage(const cfen_net* net, const char* name, const void** ptr, int32_t* C, int32_t* cs, int32_t* H, int32_t* W);
/* Device addresses of the 3 error words of the persistent GViT chains (csrc/k_gvit.hip): a word becomes 1 if a grid-barrier wait ever gave up
 * (never expected: the teams fit the chip); outputs of that forward are then invalid.  Valid after the first forward. */
int cfen_net_chain_error_words(const cfen_net* net, const void** words, int n);
/* 2*MAC count of one forward per image (SURVEY 8d closed form), for roofline reporting             */
double cfen_net_flops_per_image(const cfen_net* net);

/* ---- individual operators (unit-tested against the oracle; also what cfen_net_forward launches) -- */

/* Y[m][n] = act(sum_k X[m][k] W[n][k] + bias[n]) + R[m][n] + P[m % period][n]      (nn.Linear family) */
int cfen_gemm_nt(int dtype, const void* X, int ldx, const void* W, int ldw, const float* bias, const void* R, int ldr, const void* P,
                 int period, void* Y, int ldy, int M, int N, int K, int relu, void* stream);
/* Linear after a LayerNorm with the LayerNorm folded into the GEMM (TransformerEncoderLayer norm1 -> in_proj, norm2 -> linear1: v3:1383-1389):
 *   Y[m][n] = act(rstd_m (sum_k X[m][k] Wl[n][k] - mean_m s[n]) + bias[n]),  mean_m / rstd_m = LayerNorm statistics of row m of X over K,
 * with Wl = W * gamma (columns), s[n] = sum_k Wl[n][k] of the ROUNDED Wl, bias = W beta + b -- what cfen_net_forward runs for the blocks
 * that have no fused kernel (GViT, LViT level 3).  K * element size must be a multiple of 128 bytes; eps must be 1e-5. */
int cfen_gemm_ln(int dtype, const void* X, int ldx, const void* Wl, int ldw, const float* s, const float* bias, void* Y, int ldy, int M, int N,
                 int K, int relu, float eps, void* stream);
/* The same GEMMs with K cut into `nsplit` slices that run as separate workgroups (few tokens against a big matrix: the launch is bound by the
 * bytes one workgroup streams).  Every slice parks its fp32 partial tile in `scratch`; the workgroup that arrives last on the tile's counter adds
 * the slices in index order and applies the epilogue -- one launch, deterministic, no float atomics.  lnf_s != NULL: W is the LayerNorm-folded Wl of
 * cfen_gemm_ln.  scratch: 4096 bytes of arrival counters, which must be ZERO before the first call and are left zero by every call, followed by
 * ceil(N/96) * ceil(M/32) * nsplit * 14336 bytes of partial slabs.  K * element size / 128 must be divisible by nsplit.   (v3:1364, 1388-1389, 1173) */
int cfen_gemm_splitk(int dtype, const void* X, int ldx, const void* W, int ldw, const float* lnf_s, const float* bias, const void* R, int ldr, void* Y,
                      int ldy, int M, int N, int K, int relu, int nsplit, void* scratch, size_t scratch_bytes, void* stream);
/* head.0.0 read straight from the network input (csrc/k_head5.hip): out = act(conv5x5(in, pad 2) * scale + shift) as a 16-channel-stride NHWC
 * CFEN_F16 map; in = (B,3,H,W) fp32 NCHW (in_u8 = 0: what model.set_input hands over, models/model_iid_dehazing.py:143) or (B,H,W,3) uint8
 * (in_u8 = 1: ToTensor + Normalize(0.5, 0.5) folded in, data/base_dataset.py:44-46).  w5: [16][5][8][4] halfs (packing.pack_head5).  H % 8 == 0,
 * W % 64 == 0.  Replaces cfen_nchw_to_nhwc / cfen_u8hwc_to_nhwc + cfen_conv2d for that layer (v3:123-127, common.py:11-14). */
int cfen_head_conv5(int dtype, int in_u8, const void* in, const void* w5, const float* scale, const float* shift, void* out, int B, int H, int W,
                    int cs_out, int act, void* stream);
/* Persistent GEMM chain (csrc/k_gvit.hip): up to 5 DEPENDENT token GEMMs  y_p = act(x_p W_p^T + bias) + residual + pos[m % period]  (or the
 * LayerNorm-folded form of cfen_gemm_ln when lnf_s != NULL) run by ONE launch of `team` workgroups (one per CU) that keep their CUs and meet at a
 * grid barrier between phases -- the nn.Linear chains of a GViT instance: linear_encoding -> in_proj, and out_proj -> linear1 -> linear2 ->
 * mlp_head.0 -> mlp_head.3 (+ fold) (v3:1143,1166,1364,1386-1389,1173,1186).  CFEN_F16 only.  w_stream: the [N][K] weight as MFMA fragment stream
 * [N/16][K/32][64 lanes][8 halfs] (packing.pack_stream_tiles); N % 128 == 0, K % 64 == 0; nsplit > 1 cuts K into slices reduced inside the launch
 * (not with lnf_s).  fold = 1: y is the NHWC map (fold_H x fold_W pixels, channel stride fold_cs) the M tokens tile with fold_p x fold_p patches of
 * fold_C channels, feature n = (i, j, c).  A phase may read what an earlier phase of the same call wrote.  sync_ws: 8192 bytes of synchronisation
 * words (the call zeroes the ones it needs; word 1 is set to 1 if a wait ever gave up -- results are then invalid) followed by the split-K slabs:
 * ceil(M/128) * max(N/128 * nsplit) * 65536 bytes.  team * 1 <= 256: every workgroup must be resident for the grid barrier. */
typedef struct cfen_chain_phase {
  const void* x; const void* w_stream; const float* bias; const float* lnf_s; const void* residual; const void* pos; void* y;
  int32_t ldx, ldr, ldy, period, N, K, relu, nsplit, fold;
} cfen_chain_phase;
typedef struct cfen_chain_args {
  cfen_chain_phase phase[5];
  int32_t nphases, M;
  int32_t fold_H, fold_W, fold_cs, fold_C, fold_p;
  void* sync_ws; size_t sync_ws_bytes;
} cfen_chain_args;
int cfen_gemm_chain(int dtype, const cfen_chain_args* a, int team, void* stream);
/* LViT token embedding without a token buffer: tok = patchify(fmap) (window partition + unfold, as cfen_patchify with pool 1)
 * is gathered by the GEMM's loader;  Y[m][n] = sum_k tok[m][k] W[n][k] + bias[n] + tok[m][n] + pos[m % period][n],
 * D = p*p*C, W is [D][D] (ldw), Y is [M][D] (ldy).                                        (v3:1140-1143, 1166) */
int cfen_embed_gather(int dtype, const void* fmap, int B, int H, int W, int C, int cs, int ws, int p, const void* weight, int ldw,
                      const float* bias, const void* pos, int period, void* Y, int ldy, void* stream);
/* LViT front half in one launch (D = p*p*C in {96, 192}): tok = patchify(fmap);  y = We tok + be + tok + pos[m % S] -> x1 [M][D];
 * qkv = Wqkv LayerNorm(y) -> qkv [M][3D].  We [D][D] and Wqkv [3D][D] with the k axis in packing.kperm32 order for CFEN_F16.
 *                                                                                      (v3:1140-1143, 1166, 1364-1371) */
typedef struct cfen_embed_qkv_args {
  const void* fmap; int32_t B, H, W, C, cs, ws, p;
  const void* we; const float* be; const void* pos;
  const float* ln_gamma; const float* ln_beta;
  const void* wqkv;
  void* x1; void* qkv;
  float eps;
  int32_t head_major_heads;   /* 0: qkv is [M][3D] row-major; > 0 (= number of heads): qkv is written per (window, head),
                                 [(window * heads + head) * 3 + {q, k, v}][S][D / heads] -- the input of cfen_attention_head_major */
} cfen_embed_qkv_args;
int cfen_embed_qkv(int dtype, const cfen_embed_qkv_args* a, void* stream);
/* The same front half for D = 384 (LViT level 3; CFEN_F16, token count a multiple of 128) on the fragment-stream ring of cfen_mlp_stream_block:
 * `we` / `wqkv` are ROW-TILE fragment streams (packing.pack_stream_rows of the kperm32-slotted matrices): [rows / 32][2 row tiles][D / 32 k-chunks][1 KiB]. */
int cfen_embed_qkv_stream(int dtype, const cfen_embed_qkv_args* a, void* stream);
/* LayerNorm over the last dim (eps as given), gamma/beta fp32                       (v3:1370-1371) */
int cfen_layernorm(int dtype, const void* X, void* Y, const float* gamma, const float* beta, int M, int D, float eps, void* stream);
/* softmax(QK^T/sqrt(dh))V per (sequence, head); QKV is [nseq*S][3*heads*dh], out [nseq*S][heads*dh]  (v3:1364) */
int cfen_attention(int dtype, const void* qkv, void* out, int nseq, int S, int heads, int dh, void* stream);
/* the same attention reading the head-major qkv layout of cfen_embed_qkv (head_major_heads = heads): the q, k and v of one
 * (sequence, head) are contiguous [S][dh] blocks.  CFEN_F16, dh = 24, S in {64, 256} (every LViT window of the 512x512 configs) or 1024 (the
 * 1024x1024 configuration: K and V of a head stay in LDS, keys in blocks of 256 with the running-maximum rescale);
 * out stays [nseq*S][heads*dh] row-major.                                                                       (v3:1364) */
int cfen_attention_head_major(int dtype, const void* qkv, void* out, int nseq, int S, int heads, int dh, void* stream);
/* Fused token MLP block (D in {96,192}; H a multiple of 64 (fp16) / 32 (fp32)):
 *   y1 = x + W2a relu(W1a LN(x) + b1a) + b2a  (LN skipped when ln_gamma is NULL);  y2 = y1 + W2b relu(W1b y1 + b1b) + b2b
 *   (second stage skipped when W1b is NULL).  With att / w_proj ([M][D] / [D][D], natural k order) x is first replaced by
 *   x + w_proj att, the attention block's output projection and residual.  Output: token-major `y` and/or folded into the NHWC map `fmap`
 *   (F.fold + Join2x2: map H x W, channels C with stride cs, window ws, patch p).  Weights [H][D] / [D][H] with
 *   the k axis in packing.kperm32 order for CFEN_F16 (natural order for CFEN_F32).   (v3:1387-1389, 1173, 1186) */
typedef struct cfen_mlp_args {
  const void* x; void* y; void* fmap;
  const void* att; const void* w_proj;   /* optional prologue x <- x + w_proj att (out_proj + residual, v3:1386); both NULL = none */
  const float* ln_gamma; const float* ln_beta;
  const void* w1a; const float* b1a; const void* w2a; const float* b2a;
  const void* w1b; const float* b1b; const void* w2b; const float* b2b;
  int64_t M;
  int32_t D, H;
  float eps;
  int32_t mapH, mapW, C, cs, ws, p;
} cfen_mlp_args;
int cfen_mlp_block(int dtype, const cfen_mlp_args* a, void* stream);
/* The same block for the embedding dims the register-resident kernel cannot hold at two waves per SIMD (CFEN_F16; D = 384 with H <= 1536: LViT
 * level 3 / GViT level 1, and D = 192 with H <= 768), one wave per SIMD on the whole register file, weights as FRAGMENT STREAMS
 * (packing.pack_stream_pair / pack_stream_sq): wa_stream / wb_stream = [H/32][W1 slice, W2 slice][D/16 fragments][1 KiB], a fragment = the
 * 16 x 32 MFMA A operand in lane order (lane l: 16 bytes of row l & 15, k quarter l >> 4), k axes in packing.kperm32 order;
 * wp_stream = [D/32][D/16][1 KiB], natural k order.  Same arithmetic as cfen_mlp_block.                (v3:1386-1389, 1173, 1186) */
typedef struct cfen_mlp_stream_args {
  const void* x; void* y; void* fmap;
  const void* att; const void* wp_stream;
  const float* ln_gamma; const float* ln_beta;
  const void* wa_stream; const float* b1a; const float* b2a;
  const void* wb_stream; const float* b1b; const float* b2b;
  int64_t M;
  int32_t D, H;
  float eps;
  int32_t mapH, mapW, C, cs, ws, p;
} cfen_mlp_stream_args;
int cfen_mlp_stream_block(int dtype, const cfen_mlp_stream_args* a, void* stream);
/* One whole LViT block per workgroup-window (CFEN_F16, C = 24, p = 2, 32-pixel windows: 256 tokens of dim 96, 4 heads of 24):
 * map in -> Crop2x2 + unfold + linear_encoding + pos -> pre-LN MHA -> FFN -> mlp_head -> fold + Join2x2 -> map out, with q / k / v, the
 * attention output and both hidden activations never leaving the chip (K and V of the window live in LDS).  `w_stream`: every weight
 * matrix of the block as one stream of 1 KiB MFMA fragments in consumption order, packing.pack_lvit_window.                                                              (v3:1025-1056, 1136-1189, 1382-1390) */
typedef struct cfen_lvit_args {
  const void* fmap; void* out;
  int32_t B, H, W, C, cs_in, cs_out, ws, p;
  const void* w_stream; const float* be; const void* pos;
  const float* ln1_gamma; const float* ln1_beta;
  const float* ln2_gamma; const float* ln2_beta;
  const float* b1a; const float* b2a;
  const float* b1b; const float* b2b;
  int32_t hidden;
  float eps;
} cfen_lvit_args;
int cfen_lvit_window(int dtype, const cfen_lvit_args* a, void* stream);
/* window partition + unfold (+ optional 4x4 mean pool) / fold + window join          (v3:1025-1056,1140,1186,1274)
 * patchify reads channels 0 .. C - 1 of every pixel (cs >= C) and writes every token element; unpatchify writes channels 0 .. C - 1 of every pixel
 * and leaves the padding lanes C .. cs - 1 untouched. */
int cfen_patchify(int dtype, const void* fmap, void* tokens, int B, int H, int W, int C, int cs, int ws, int p, int pool, void* stream);
int cfen_unpatchify(int dtype, const void* tokens, void* fmap, int B, int H, int W, int C, int cs, int ws, int p, void* stream);
/* two successive bilinear x2 upsamples, align_corners=False; writes channels 0 .. C - 1 of every output pixel, padding lanes C .. cs_out - 1 are left
 * untouched                                                                             (v3:1323) */
int cfen_upsample4(int dtype, const void* small, void* out, int B, int h, int w, int C, int cs_in, int cs_out, void* stream);
int cfen_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int C, int H, int W, int cs, void* stream);
/* pre / post-processing on the device:
 * uint8 (B,H,W,3) image -> NHWC T, channels zero-padded to cs, v -> ((v/255) - 0.5) / 0.5   (ToTensor + Normalize, data/base_dataset.py:44-46)
 * (1|3,H,W) fp32 in [-1,1] -> (H,W,3) uint8, (x+1)/2*255 truncated, 1 channel tiled to 3    (tensor2im, util/util.py:12-24)              */
int cfen_u8hwc_to_nhwc(int dtype, const unsigned char* in, void* out, int B, int H, int W, int cs, void* stream);
int cfen_tensor2im_u8(const float* in, unsigned char* out, int C, int H, int W, void* stream);

/* Overlapping-tile inference of images of any size (tiled.py).  The image size is baked into the generator (learned positional tables and
 * F.fold(..., img_dim): v3:1125-1127, 1186, 1321), so an H x W image runs as T x T tiles, T = cfg.image_size, through the unchanged forward.
 * Tile plan per axis of extent L with overlap o (0 <= o <= T/2): n = 1 if L <= T else 1 + ceil((L - T) / (T - o)) tiles at origins
 * p_j = (j (L - T)) // (n - 1) (p_0 = 0 when n = 1), numbered row-major t = i nx + j.  Tile pixel (u, v) of tile (i, j) is source pixel
 * (mirror(p_i + u, H), mirror(q_j + v, W)), mirror = numpy 'reflect' (edge pixel not repeated; only where L < T).
 *
 * gather: tiles [t0, t0 + B) into the network's input slab; tile indices >= ny nx repeat the last tile (a full last batch).  A pure copy.
 *   u8 = 1: src (H,W,3) uint8 -> dst (B,T,T,3) uint8 (a cfen_net_set_input_u8 net's input);  u8 = 0: src (3,H,W) fp32 -> dst (B,3,T,T) fp32.
 *   T % 16 == 0; dst 16-byte aligned; the grid must tile the image (L <= T: n = 1; else n >= 2 and n T >= L).                                      */
int cfen_tile_gather(int u8, const void* src, void* dst, int H, int W, int T, int ny, int nx, int t0, int B, void* stream);
/* blend: the tile outputs back into the H x W image.  arena = the forwards' own output slabs back to back, dtype 0 fp32 / 1 fp16 (output_f16 nets):
 *   slab s holds tiles [s B, s B + B) as [xr (B,3,T,T) | xs (B,1,T,T) | xd (B,3,T,T)] (7 B T T elements), tile t in slab t / B, slot t % B;
 *   ceil(ny nx / B) slabs.  ny / nx must be the plan's tile counts for this overlap.
 * dtype is a bit field: bits 0..7 the arena element type (0 fp32, 1 fp16); bits 8..23 lane0 (default 0), the lane within its slab of the image's
 *   tile 0 when the image shares its slabs with other images (tiled.pack_plan); bits 24 and up must be zero.  arena then points at the slab that
 *   holds tile 0, tile t lives at global slot g = lane0 + t (slab g / B, lane g % B), and the image needs ceil((lane0 + ny nx) / B) slabs from
 *   that pointer.  CFEN_ERR_ARG on an element type other than 0 / 1, on high bits that are set, and on lane0 >= B.  lane0 = 0 is the plain call.
 * Per output pixel: the tile value unchanged where one tile covers it; else sum(w v) / sum(w) in fp32 over the covering tiles in increasing t,
 *   w = w(u) w(v), w(u) = min(1, (min(u, e - 1 - u) + 1) / (o + 1)), e = min(T, L).  No atomics: bitwise reproducible.
 * out_u8 = 0: xr (3,H,W), xs (1,H,W), xd (3,H,W) fp32.  out_u8 = 1: xr / xs / xd each (H,W,3) uint8, tensor2im's arithmetic of the fp32 value
 *   ((x+1)/2*255 truncated, xs tiled to 3 channels; util/util.py:12-24).  Outputs 16-byte aligned.                                                */
int cfen_tile_blend(int dtype, const void* arena, int B, int T, int H, int W, int ny, int nx, int overlap, int out_u8, void* xr, void* xs, void* xd,
                    void* stream);

/* Geometric self-ensemble (x8) of the generator (ensemble.py; the reference's Model.forward_x8, models/vit_model.py:102-147): the output is the
 * mean over the eight flips / transposes of the input.  With v = flip W, h = flip H, t = swap H and W, variant i = b0 + 2 b1 + 4 b2 of a T x T
 * plane x is x_i = t^b2(h^b1(v^b0(x))) (v applied first); every output plane y_i of the forward of x_i is mapped back as v^b0(h^b1(t^b2(y_i))) and
 * the result is the fp32 sum of the eight in increasing i, times 0.125f -- no other arithmetic, no atomics: bitwise reproducible.
 *
 * expand: image m of the M images at src into the network's batch-8 input slab dst, in variant order.  A pure copy.
 *   u8 = 1: src (M,T,T,3) uint8 -> dst (8,T,T,3) uint8;  u8 = 0: src (M,3,T,T) fp32 -> dst (8,3,T,T) fp32.
 * merge: M forward output slabs back to back, dtype 0 fp32 / 1 fp16; slab m = [xr (8,3,T,T) | xs (8,1,T,T) | xd (8,3,T,T)] (56 T T elements) of
 *   the eight variants of image m.  out_u8 = 0: xr (M,3,T,T), xs (M,1,T,T), xd (M,3,T,T) fp32.  out_u8 = 1: xr / xs / xd each (M,T,T,3) uint8,
 *   tensor2im's arithmetic of the fp32 value ((x+1)/2*255 truncated, xs tiled to 3 channels; util/util.py:12-24).
 * T % 16 == 0, 16 <= T <= 8192; 1 <= M <= 4096; every pointer 16-byte aligned.                                                                   */
int cfen_x8_expand(int u8, const void* src, void* dst, int M, int m, int T, void* stream);
int cfen_x8_merge(int dtype, const void* arena, int M, int T, int out_u8, void* xr, void* xs, void* xd, void* stream);

/* Image quality of an output against its ground truth, per image pair, in one fused pass (csrc/k_metrics.hip; metrics.py, test.py --eval).
 * Both images are scored on the [0,1] scale in fp32, data range L = 1:
 *   u8 = 1: a, b (B,H,W,3) uint8, v -> v / 255 (C must be 3);  u8 = 0: a, b (B,C,H,W) fp32, C 1 or 3, v -> (v - lo) / (hi - lo), e.g. (-1, 1)
 *           for the generator's float outputs (lo / hi are ignored for uint8).
 *   SSIM: pytorch_msssim.ssim(window_size = 11, size_average = True, val_range = 1) of the reference (pytorch_msssim/__init__.py:19-70): 11 x 11
 *         Gaussian window, sigma 1.5, normalised; VALID convolution (no padding); C1 = 0.01^2, C2 = 0.03^2; the mean over all C (H - 10) (W - 10)
 *         window positions.  H, W >= 11: the reference shrinks its window for smaller images, this library refuses them (CFEN_ERR_ARG).
 *   SSE : the sum over all C H W values of (255 (a - b))^2, i.e. on the 0..255 scale in both formats; for uint8 input it is summed in integers and
 *         is exact.  PSNR = 10 log10(255^2 C H W / SSE) = 10 log10(1 / MSE on the [0,1] scale) is left to the caller (metrics.py; inf when SSE = 0):
 *         the standard definition over the RGB values, not the Y channel -- the reference has no PSNR code.
 * out: [B][2] doubles on the device, (SSE, SSIM mean) per pair, 8-byte aligned.  scratch: cfen_image_metrics_bytes(B, C, H, W) bytes of device
 * memory, 8-byte aligned, contents irrelevant before and after (one (SSE, SSIM sum) pair per workgroup tile; 0 for dimensions the call refuses).
 * No atomics, fixed summation order in fp64: the same inputs give the same bits on every call, stream and batch size.                        */
size_t cfen_image_metrics_bytes(int B, int C, int H, int W);
int cfen_image_metrics(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                       void* stream);

/* Multi-scale SSIM of the same image pairs (csrc/k_metrics.hip; metrics.py, test.py --eval --eval_metrics psnr,ssim,msssim): the reference's
 * pytorch_msssim.msssim(img1, img2, window_size = 11, size_average = True, val_range = 1, normalize = None) (pytorch_msssim/__init__.py:73-107).
 * Inputs, u8, lo / hi and the [0,1] mapping are those of cfen_image_metrics.
 *   Pyramid: level 0 is the mapped image.  Level l + 1 is F.avg_pool2d(level l, (2, 2)): the mean of each 2 x 2 block in fp32,
 *            (((a + b) + c) + d) * 0.25f with a, b the upper and c, d the lower pair.  Odd sizes floor: H_{l+1} = H_l / 2, W_{l+1} = W_l / 2 in
 *            integers, the last row / column is dropped.  Both images are pooled.
 *   Levels : at each of the five levels the same 11 x 11 Gaussian window (sigma 1.5, normalised) as a VALID convolution, C1 = 0.01^2, C2 = 0.03^2,
 *            and two means over all C (H_l - 10) (W_l - 10) window positions:
 *              ssim_l  the mean of the SSIM map of cfen_image_metrics,
 *              cs_l    the mean of (2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2).
 *   Value  : MS-SSIM = cs_0^w_0 cs_1^w_1 cs_2^w_2 cs_3^w_3 ssim_4^w_4, w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333).  The device returns the
 *            ten level values; the powers and the product are the caller's, in float64 (metrics.msssim_from_levels).  With normalize = None the
 *            reference gives NaN when one of the five terms it uses is negative, and so does metrics.py.
 *   Size   : level 4 must hold one window, so min(H, W) >= 176 = 11 * 2^4.  The reference shrinks its window for smaller images; this library
 *            refuses them (CFEN_ERR_ARG, the message names 176).
 * out: [B][11] doubles on the device, 8-byte aligned: SSE, then (ssim_l, cs_l) for l = 0 .. 4.  out[b][0] and out[b][1] are bit for bit what
 * cfen_image_metrics writes for the same input, so one call serves PSNR, SSIM and MS-SSIM.  scratch: cfen_image_msssim_bytes(B, C, H, W) bytes of
 * device memory, 8-byte aligned, contents irrelevant before and after (per workgroup tile of every level one (SSE, SSIM sum, cs sum) triple, then
 * levels 1 .. 4 of both images as planar fp32; 0 for dimensions the call refuses).  Five level launches and one finish on `stream`.
 * No atomics, fixed summation order in fp64: the same inputs give the same bits on every call, stream and batch size.                        */
size_t cfen_image_msssim_bytes(int B, int C, int H, int W);
int cfen_image_msssim(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                      void* stream);

/* PNG encoding of uint8 images on the device (csrc/k_png.hip; png.py, test.py --gpu_png): per image one finished zlib stream, the payload of the
 * single IDAT chunk of an 8-bit RGB, non-interlaced PNG.  The caller adds signature, IHDR, the IDAT framing with its CRC-32, and IEND.
 *   stream : 78 01 | per strip: one non-final deflate block, then an empty non-final stored block (000, pad to a byte, 00 00 FF FF) |
 *            01 00 00 FF FF | Adler-32 of the filtered scanlines, big-endian.
 *   strips : R = max(1, 32768 / (3 W + 1)) rows, the last may be shorter; a scanline longer than 32768 bytes is refused (CFEN_ERR_ARG): encode that
 *            image on the host.
 *   filter : per row the type among None, Sub, Up, Average, Paeth with the smallest sum of |signed residual| (v < 128 ? v : 256 - v), ties to the
 *            lowest type; the row above row 0 is zeros.
 *   block  : literals only.  The first cheapest of the n_tables candidate codes as a dynamic-Huffman block (cost = header bits + histogram . lengths,
 *            the end-of-block symbol counted once), used only if strictly below a stored block's 8 n + 40 bits, n the strip's filtered bytes.
 * images: (B,H,W,3) uint8, contiguous.  tables: n_tables (1 .. 16) x 384 uint32 words on the device, per table
 *   word 0        bits of the block header (BFINAL 0, BTYPE 2, HLIT 257, HDIST 1 with that code's length 0, the code-length code, the lengths),
 *   words 1..63   those bits, packed from the least significant bit of word 1 on,
 *   words 64..320 symbol 0..255 and end-of-block: (length << 16) | code, the code bit-reversed for LSB-first packing; every length 1 .. 15 and the
 *                 code complete (png.py makes them); words 321..383 zero.
 * workspace: cfen_png_workspace_bytes(B, H, W, &strip_bytes, &out_stride) bytes, contents irrelevant before and after: a 16-byte record and a slot of
 *   strip_bytes (n + 16 rounded up to 16, the stored worst case) per strip.  0 for dimensions the call refuses.
 * out: B x out_stride bytes, the stream of image b from out + b * out_stride; out_lengths[b]: its length in bytes.  images, workspace and out
 * 16-byte aligned.  No atomics on global memory, integer arithmetic: the same image gives the same bytes on every call, stream and batch size.   */
size_t cfen_png_workspace_bytes(int B, int H, int W, size_t* strip_bytes, size_t* out_stride);
int cfen_png_deflate(const unsigned char* images, int B, int H, int W, const void* tables, int n_tables, void* workspace, unsigned char* out,
                     int* out_lengths, void* stream);

/* Conv2d / ConvTranspose2d(4,2,1) as implicit GEMM with fused affine + activation + residuals.
 * kind 0: Conv2d(k, stride, pad) over nsrc (1..3) channel-concatenated inputs (src0 | src1 | src2, the concat is never
 * materialised: v3:488 torch.cat((local, global), 1); crs_gd4:854 cat of three); kind 1: ConvTranspose2d k4 s2 p1.
 * weight: packed [nphase][Cout_pad][Kpad] (packing.py); scale/shift: [Cout_pad] fp32.
 * wlayout 0: k = tap*Cin + c (any geometry).  wlayout 1 ("rows", LDS-tiled kernel): stride 1, pad k/2, one source,
 * Cout <= 16, H % 8 == 0, W % 64 == 0, pixel stride 16/32/64 bytes; each kernel row is padded with zero taps to a
 * multiple of 64 bytes: k = (ky*KSP + kx)*cs_in + c, KSP = ceil(k*cs_in*esz/64)*64/(cs_in*esz), Kpad = k*KSP*cs_in.
 * wlayout 1 with kind 1 (fp16, Hin % 4 == 0, Win % 32 == 0, (cs_in, Cout_pad) in {(24,16),(48,32),(96,48)}): every tap's
 * channels zero-padded to a multiple of 64 bytes: [4 phases][Cout_pad][4 taps][CP], CP = ceil(cs_in*esz/64)*64/esz.        */
typedef struct cfen_conv_args {
  int32_t kind, k, stride, pad, reflect, nsrc;
  int32_t B, Hin, Win, Cin, cs_in;
  int32_t Cout, Cout_pad, Kpad, cs_out;
  int32_t act;            /* 0 none, 1 ReLU, 2 tanh */
  int32_t out_nchw_f32;   /* write (B,Cout,H,W) fp32 instead of NHWC */
  int32_t cs_res;
  int32_t wlayout;        /* 0 tap-major, 1 rows (see above), 2 Toeplitz 7x7 (fp16, cs_in 16, Cout <= 4, fp32 NCHW output, H % 16 == 0,
                             W % 64 == 0): [16 rows = co*4 + dxo][7][10 taps][16], w[co][ky][kx' - dxo][ci], Kpad 1120 */
  const void* src0;
  const void* src1;
  const void* weight;
  const float* scale;
  const float* shift;
  const void* res0;
  const void* res1;
  void* out;
  const void* src2;       /* third concatenated input (nsrc == 3), else NULL */
} cfen_conv_args;
int cfen_conv2d(int dtype, const cfen_conv_args* a, void* stream);

/* stats_ws of the two functions below: cfen_stats_workspace(B, C) bytes of fp32 scratch, contents irrelevant before and after the call */
size_t cfen_stats_workspace(int B, int C);
/* InstanceNorm2d(affine=False) + ReLU in place                                        (v3:292-302) */
int cfen_instnorm_relu(int dtype, void* x, float* stats_ws, int B, int HW, int C, int cs, float eps, void* stream);
/* CFSM2G: out = x0 + x1*g1 + x2*g2, gates from global avg/max pools of x0+x1+x2          (v3:1481-1517)
 * w: fp32 [avg_cf1, avg_cf2, max_cf1, max_cf2] x {W0 (C/4 x C), W2 (C x C/4)}                      */
int cfen_cfsm2g(int dtype, const void* x0, const void* x1, const void* x2, void* out, const float* w, float* stats_ws, int B, int HW,
                int C, int cs, void* stream);

/* ---- deformable convolution (replaces the pybind module of dcn/src/deform_conv_cuda.cpp:681-695) ---- */
/* deform_conv_forward_cuda (dcn/src/deform_conv_cuda.cpp:151-156): NCHW tensors; note the reference passes W before H for
 * kernel/stride/pad/dilation here.  `columns` is the reference's scratch tensor of that name: device memory of at least
 * cfen_deform_conv_columns_bytes() bytes, 16-byte aligned (the kernel keeps an NHWC copy of the input and tap-major weights
 * there -- the column matrix itself is never materialised; the reference's `ones` buffer has no counterpart).  With columns ==
 * NULL (or too small, or C/group not a multiple of the 16-byte channel vector) a slower kernel gathers from the NCHW planes. */
size_t cfen_deform_conv_columns_bytes(int dtype, int B, int Cin, int H, int W, int Cout, int kH, int kW, int group);
int cfen_deform_conv_forward(int dtype, const void* input, const void* weight, const void* offset, void* output, int B, int Cin, int H,
                             int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW, int dilationH, int group,
                             int deformable_group, int im2col_step, void* columns, size_t columns_bytes, void* stream);
/* (extension, round 6) the same with `input` laid out [B][H][W][Cin] -- the memory of a torch channels_last tensor: the NHWC copy the kernel samples from is the input
 * itself, the layout pre-pass only re-orders the weights (12-14 us of a 107 us call at (8, 24, 256, 256)).  Needs `columns` (for the weights) and Cin / group a multiple
 * of the 16-byte channel vector: CFEN_ERR_ARG otherwise.  offset / mask / output stay NCHW as in the reference.                                                    */
int cfen_deform_conv_forward_nhwc(int dtype, const void* input, const void* weight, const void* offset, void* output, int B, int Cin, int H,
                                  int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW, int dilationH, int group,
                                  int deformable_group, int im2col_step, void* columns, size_t columns_bytes, void* stream);
int cfen_modulated_deform_conv_forward_nhwc(int dtype, const void* input, const void* weight, const void* bias, const void* offset,
                                            const void* mask, void* output, int B, int Cin, int H, int W, int Cout, int kernel_h, int kernel_w,
                                            int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int group,
                                            int deformable_group, int with_bias, void* columns, size_t columns_bytes, void* stream);
/* modulated_deform_conv_cuda_forward (dcn/src/deform_conv_cuda.cpp:486-492): h before w; bias may be NULL; columns as above */
int cfen_modulated_deform_conv_forward(int dtype, const void* input, const void* weight, const void* bias, const void* offset,
                                       const void* mask, void* output, int B, int Cin, int H, int W, int Cout, int kernel_h, int kernel_w,
                                       int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int group,
                                       int deformable_group, int with_bias, void* columns, size_t columns_bytes, void* stream);

/* ---- deformable convolution, backward direction ----
 * NCHW tensors of `dtype`, arithmetic in fp32.  `columns`: device scratch of at least cfen_deform_conv_backward_bytes() bytes, 16-byte
 * aligned (required: NHWC / transposed operand copies, the column-gradient matrix, fp32 accumulators).  gradInput / gradOffset / grad_mask
 * are OVERWRITTEN; gradWeight / grad_bias are ACCUMULATED INTO (the reference's addmm_ with beta = 1: its Python side passes zeros).
 * grad_input is summed with fp32 atomics like the reference's col2im (dcn/src/deform_conv_cuda_kernel.cu:322): reproducible up to
 * summation order. */
size_t cfen_deform_conv_backward_bytes(int B, int Cin, int H, int W, int Cout, int kH, int kW, int Hout, int Wout, int group);
/* col2im variant switch (process-wide, for A/B runs and tests): 1 (default) accumulates grad_input per 16 x 16 output-pixel tile in LDS, parks
 * each tile's footprint in `columns` and sums the overlapping footprints per input pixel in a fixed order; 2 flushes the tiles with global
 * atomics instead; 0 sends every add to global memory as the reference does; returns the previous setting */
int cfen_deform_conv_backward_set_lds(int enabled);
/* deform_conv_backward_input_cuda (dcn/src/deform_conv_cuda.cpp:260-265): W before H, as in the forward */
int cfen_deform_conv_backward_input(int dtype, const void* input, const void* offset, const void* gradOutput, void* gradInput, void* gradOffset,
                                    const void* weight, int B, int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW,
                                    int padH, int dilationW, int dilationH, int group, int deformable_group, int im2col_step, void* columns,
                                    size_t columns_bytes, void* stream);
/* deform_conv_backward_parameters_cuda (dcn/src/deform_conv_cuda.cpp:370-376): gradWeight += scale * d loss / d weight */
int cfen_deform_conv_backward_parameters(int dtype, const void* input, const void* offset, const void* gradOutput, void* gradWeight, int B,
                                         int Cin, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW,
                                         int dilationH, int group, int deformable_group, float scale, int im2col_step, void* columns,
                                         size_t columns_bytes, void* stream);
/* modulated_deform_conv_cuda_backward (dcn/src/deform_conv_cuda.cpp:566-574): h before w; `bias` is unused (shape only in the reference) */
int cfen_modulated_deform_conv_backward(int dtype, const void* input, const void* weight, const void* bias, const void* offset, const void* mask,
                                        void* grad_input, void* grad_weight, void* grad_bias, void* grad_offset, void* grad_mask,
                                        const void* grad_output, int B, int Cin, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h,
                                        int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int group, int deformable_group,
                                        int with_bias, void* columns, size_t columns_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFEN_HIP_H */
