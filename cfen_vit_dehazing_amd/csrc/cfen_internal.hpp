// Internal launcher prototypes shared by cfen_api.cpp and cfen_net.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "cfen_tune_knobs.hpp"   // int& cfen_tune_<knob>(): every kernel-variant knob, with its default and what it selects

struct ConvDesc;

int cfen_gemm_impl(int dtype, const void* X, int ldx, const void* W, int ldw, const float* bias, const void* R, int ldr, const void* P,
                   int period, void* Y, int ldy, int M, int N, int K, int relu, hipStream_t s);
int cfen_zero_words_impl(void* p, size_t nwords, hipStream_t s);   // k_tokens.hip
int cfen_zero_async(void* p, size_t bytes, hipStream_t s);   // memset 0 on a lane (eager, or a node of the graph being recorded)
float& cfen_gemm_lnf_eps();   // LayerNorm eps used by the LN-folded GEMMs (1e-5, the only value the generator uses)
// Y = tok W^T + bias + tok + P[m % period]  with tok = the patch tokens of an NHWC map, gathered by the GEMM's loader
// (window partition + unfold + linear_encoding + residual + position add in one launch; v3:1025-1056,1140-1143,1166)
struct CfenTokGather { const void* map; int B, H, W, C, cs, ws, p; };
int cfen_embed_gather_impl(int dtype, const CfenTokGather* tg, const void* W, int ldw, const float* bias, const void* P, int period,
                           void* Y, int ldy, int M, hipStream_t s);
// LViT front half fused (k_embed.hip): gather + linear_encoding + residual + position + LayerNorm + qkv projection
struct CfenEmbedQkvArgs {
  const void* fmap; int B, H, W, C, cs, ws, p;        // NHWC map the patch tokens are gathered from
  const void* We; const float* be; const void* pos;   // [D][D] (k axis in packing.kperm32 order for fp16), [D], [S][D]
  const float* ln_g; const float* ln_b;
  const void* Wqkv;                                   // [3D][D], k axis as We
  void* X1; void* QKV;                                // [M][D], [M][3D]
  long long M; int D; float eps;
  int hm_heads;   // > 0: QKV is written head-major, [(window * heads + head) * 3 + {q,k,v}][S][D / heads] (k_attention_hm's input)
};
bool cfen_embed_qkv_supported(int D);
int cfen_embed_qkv_impl_g(int dtype, int ng, const CfenEmbedQkvArgs* a, hipStream_t s);
// the same front half for D = 384 on the fragment-stream ring (k_stream.hip); We / Wqkv are packing.pack_stream_rows streams
bool cfen_front3_supported(int dtype, int D, long long M);
int cfen_front3_impl_g(int dtype, int ng, const CfenEmbedQkvArgs* a, hipStream_t s);
// grouped launches (cfen_common.hpp: CFEN_MAX_GROUPS problems of identical geometry, one launch)
struct CfenGemmPtrs {
  const void* X; const void* W; const float* bias; const void* R; const void* P; void* Y; const void* gmap;
  // LayerNorm folded into the GEMM (k_gemm_dma only): X is the un-normalised row x, W = W0 * gamma (columns scaled on the host),
  // lnf_s[n] = sum_k W[n][k], bias = W0 beta + b0:  Y = act(rstd_m (x W^T - mean_m lnf_s) + bias) + ...; mean / rstd of every row are
  // accumulated by the workgroup from the X tiles it stages anyway.  null = plain GEMM.
  const float* lnf_s;
  // W is stored tile-major instead of row-major: [ceil(N / 96)][K * sizeof(T) / 128][96 rows][128 bytes], rows past N zero (packing.pack_wtile).
  // One K-step of a 96-feature tile is then ONE contiguous 12 KB run of HBM instead of 96 pieces of 128 bytes a whole row apart --
  // what the few-token GViT GEMMs (weights streamed once from HBM, 0.5 GB per forward) are bound by.  k_gemm_dma with 96-feature tiles only.
  int wtile = 0;
  void* ymap = nullptr;   // fold: Y goes into this NHWC map (geometry = cfen_gemm_impl_g's `yg`), see GemmArgs::ymap
};
int cfen_gemm_impl_g(int dtype, int ng, const CfenGemmPtrs* gp, int ldx, int ldw, int ldr, int period, int ldy, int M, int N, int K, int relu,
                     const CfenTokGather* tg, hipStream_t s, float* const* splitk_ws, size_t splitk_ws_bytes, const CfenTokGather* yg = nullptr,
                     int force_nsplit = 0);
// tg: geometry only, the maps are gp[g].gmap.  splitk_ws (may be null): one scratch per problem for split-K: CFEN_SPLITK_COUNTERS arrival
// counters (unsigned, ZERO before the first use; every launch leaves them zero) followed by the fp32 partial slabs.
// force_nsplit: 0 = shape rule, 1 = never split, > 1 = exactly this many K slices (tests)
constexpr int CFEN_SPLITK_COUNTERS = 1024;
int cfen_patchify_impl_g(int dtype, int ng, const void* const* fmap, void* const* tok, int B, int H, int W, int C, int cs, int ws, int p, int pool,
                         int inverse, hipStream_t s);
int cfen_upsample4_impl_g(int dtype, int ng, const void* const* small, void* const* out, int B, int h, int w, int C, int cs_in, int cs_out,
                          hipStream_t s);
int cfen_attention_impl_g(int dtype, int ng, const void* const* qkv, void* const* out, int nseq, int S, int heads, int dh, hipStream_t s);
int cfen_layernorm_impl_g(int dtype, int ng, const void* const* X, void* const* Y, const float* const* g, const float* const* b, int M, int D,
                          float eps, hipStream_t s, int cs = 0, int C = 0);   // cs > 0: rows of D / cs pixels whose first C of cs slots are real (include/cfen_padnorm.h)
// window attention on the head-major qkv layout (see CfenEmbedQkvArgs::hm_heads); fp16, head_dim 24, S in {64, 256}
bool cfen_attention_hm_supported(int dtype, int S, int dh);
int cfen_attention_hm_impl_g(int dtype, int ng, const void* const* qkv, void* const* out, int nseq, int S, int heads, int dh, hipStream_t s);
int cfen_attention_impl(int dtype, const void* qkv, void* out, int nseq, int S, int heads, int dh, hipStream_t s);
int cfen_layernorm_impl(int dtype, const void* X, void* Y, const float* g, const float* b, int M, int D, float eps, hipStream_t s);
int cfen_patchify_impl(int dtype, const void* fmap, void* tok, int B, int H, int W, int C, int cs, int ws, int p, int pool, int inverse,
                       hipStream_t s);
int cfen_upsample4_impl(int dtype, const void* small, void* out, int B, int h, int w, int C, int cs_in, int cs_out, hipStream_t s);
int cfen_nchw_to_nhwc_impl(int dtype, const float* in, void* out, int B, int C, int H, int W, int cs, hipStream_t s);
int cfen_tensor2im_u8_impl(const float* in, unsigned char* out, int C, int H, int W, hipStream_t s);
// overlapping-tile inference (k_tile.hip)
size_t cfen_image_metrics_bytes_impl(int B, int C, int H, int W);
int cfen_image_metrics_impl(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                            hipStream_t s);
size_t cfen_image_msssim_bytes_impl(int B, int C, int H, int W);
int cfen_image_msssim_impl(int u8, const void* a, const void* b, int B, int C, int H, int W, float lo, float hi, void* scratch, double* out,
                           hipStream_t s);
size_t cfen_png_workspace_bytes_impl(int B, int H, int W, size_t* strip_bytes, size_t* out_stride);
int cfen_png_deflate_impl(const unsigned char* images, int B, int H, int W, const void* tables, int n_tables, void* workspace, unsigned char* out,
                          int* out_lengths, hipStream_t s);
int cfen_tile_gather_impl(int u8, const void* src, void* dst, int H, int W, int T, int ny, int nx, int t0, int B, hipStream_t s);
int cfen_tile_blend_impl(int dtype, const void* arena, int B, int T, int H, int W, int ny, int nx, int overlap, int out_u8, void* xr, void* xs,
                         void* xd, hipStream_t s);
// PIL-exact uint8 resampling (k_resample.hip; include/cfen_resample.h)
int cfen_resample_u8_impl(const unsigned char* src, int B, int H, int W, const int* xbounds, const int* xcoef, int xk, int W2, const int* ybounds,
                          const int* ycoef, int yk, int H2, unsigned char* tmp, unsigned char* dst, hipStream_t s);
// geometric self-ensemble (k_ensemble.hip)
int cfen_x8_expand_impl(int u8, const void* src, void* dst, int M, int m, int T, hipStream_t s);
int cfen_x8_merge_impl(int dtype, const void* arena, int M, int T, int out_u8, void* xr, void* xs, void* xd, hipStream_t s);
int cfen_u8hwc_to_nhwc_impl(int dtype, const unsigned char* in, void* out, int B, int H, int W, int cs, hipStream_t s);
int cfen_conv_impl(int dtype, const ConvDesc* d, hipStream_t s);
// LDS-tiled stride-1 path (k_conv_tile.hip); weights in the "rows" layout, d->Kpad == cfen_conv_tile_kpad
bool cfen_conv_tile_supported(int dtype, int kind, int k, int stride, int pad, int nsrc, int cs_in, int Cout_pad, int H, int W);
int cfen_conv_tile_kpad(int dtype, int k, int cs_in);
int cfen_conv_tile_impl(int dtype, const ConvDesc* d, int k, hipStream_t s);
// head conv5x5 + ResBlock in one launch, intermediates in LDS (k_conv_tile.hip: k_head_fused); fp16, 12 head channels
bool cfen_head_fused_supported(int dtype, int cs_in, int C, int H, int W);
int cfen_head_fused_impl(int dtype, const void* in, void* out, const void* w5, const float* s5, const float* t5, const void* wa, const float* sa,
                         const float* ta, const void* wb, const float* sb, const float* tb, int B, int H, int W, hipStream_t s);
bool cfen_convT_tile_supported(int dtype, int cs_in, int Cout_pad, int Hin, int Win);
int cfen_convT_tile_kpad(int dtype, int cs_in);
int cfen_convT_tile_impl(int dtype, const ConvDesc* d, hipStream_t s);
int cfen_conv_impl_g(int dtype, int ng, const ConvDesc* d, hipStream_t s);
bool cfen_conv_up4_supported(int dtype, int ng, int B, int H, int W, int Cin, int cs_low, int Cout_pad, int Kpad);
int cfen_conv_tile_impl_g(int dtype, int ng, const ConvDesc* d, int k, hipStream_t s);
int cfen_convT_tile_impl_g(int dtype, int ng, const ConvDesc* d, hipStream_t s);
// 7x7, <= 4 output channels, fp32 NCHW output: Toeplitz-expanded weights [16][7][10 taps][16] (k_conv_tile.hip: k_conv7_tz)
bool cfen_conv7_tz_supported(int dtype, int k, int stride, int pad, int nsrc, int cs_in, int Cout, int out_nchw_f32, int H, int W);
int cfen_conv7_tz_kpad();
int cfen_conv7_tz_impl_g(int dtype, int ng, const ConvDesc* d, hipStream_t s);
size_t cfen_stats_workspace_bytes(int B, int C);
int cfen_instnorm_relu_impl(int dtype, void* x, float* part, int B, int HW, int C, int cs, float eps, hipStream_t s);
// ActNorm2d first-call init from the raw layer output x (NHWC, B images): per-channel statistics over the batch -> folded
// (scale, shift) epilogue table + raw (weight, bias) in an_out[2][Cpad]                      (models/actnorm.py:25-37)
int cfen_actnorm_init_impl(int dtype, const void* x, float* part, int B, int HW, int C, int cs, int Cpad, const float* conv_bias, float* scale,
                           float* shift, float* an_out, hipStream_t s);
int cfen_cfsm2g_impl(int dtype, const void* x0, const void* x1, const void* x2, void* out, const float* w, float* part, int B, int HW,
                     int C, int cs, hipStream_t s);
// what-if probe: a launch that holds `wgs` x `ng` CUs for `usec` microseconds ("net.gvit_dummy_*": CU-time experiments, results invalid)
int cfen_occupy_impl(int wgs, int ng, int usec, int do_stream, const void* src, size_t src_bytes, void* sink, hipStream_t s);
// Persistent GEMM chain (k_gvit.hip): up to 5 dependent GEMM phases Y = epi(X W^T) run by ONE launch of `team` workgroups per problem that
// meet at a grid barrier between phases.  W: fragment streams (packing.pack_stream_tiles).  fp16.
struct CfenChainPhase {
  const void* X; const void* W; const float* bias; const float* lnf_s; const void* R; const void* P; void* Y;
  int ldx, ldr, ldy, period, N, K, relu, nsplit, fold;
};
struct CfenChainArgs {
  CfenChainPhase ph[5];
  int nph, M;
  int fH, fW, fcs, fC, fp;     // fold geometry of the phases with fold = 1 (Y = NHWC map of fH x fW pixels, fp x fp patches of fC channels at stride fcs)
  unsigned* bar;               // grid-barrier counter, ZERO before the launch (one word per launch)
  unsigned* cnt; int ncnt;     // split-K arrival counters (zero; every launch leaves them zero)
  float* part; size_t part_bytes;   // split-K slabs
  unsigned* err;               // set to 1 when a wait gave up (never expected)
};
size_t cfen_gvit_chain_part_bytes(int M, int maxN, int max_nsplit);
int cfen_gvit_chain_impl_g(int dtype, int ng, const CfenChainArgs* ca, int team, hipStream_t s);
// head.0.0 (conv 5x5, 3 -> 12 channels) read straight from the fp32 NCHW input or the uint8 HWC image (k_head5.hip); w5 = packing.pack_head5
bool cfen_head5_supported(int dtype, int Cout_pad, int cs_out, int H, int W);
int cfen_head5_impl(int dtype, int in_u8, const void* in, const void* w5, const float* scale, const float* shift, void* out, int B, int H, int W,
                    int cs_out, int act, hipStream_t s);
// head.0.1 ResBlock (conv3x3 + ReLU + conv3x3 + skip) in one launch, the hidden map in LDS (k_fuse.hip); fp16, 16-channel-stride maps
bool cfen_resblock_fused_supported(int dtype, int cs, int C, int H, int W);
int cfen_resblock_fused_impl(int dtype, const void* in, void* out, const void* wa, const float* sa, const float* ta, const void* wb, const float* sb,
                             const float* tb, int B, int H, int W, hipStream_t s);
// us_conv_d01* (ConvTranspose 24 -> 12 + ActNorm + ReLU) + the tail's 3x3 in one grouped launch, the map between them in LDS (k_fuse.hip)
struct CfenUpConv3 {
  const void* in; int B, Hin, Win, cs_in;                      // (B, Hin, Win, cs_in) fp16 map, cs_in * 2 <= 64 bytes
  const void* wT; const float* sT; const float* tT; int actT;  // ConvTranspose: "<layer>.wr" [4][16][4 x 32], epilogue table, activation
  const void* w3; const float* s3; const float* t3; int act3;  // 3x3: "<layer>.wr" [16][3][2][32]
  void* out;                                                   // (B, 2 Hin, 2 Win, 16) output of the 3x3
  void* up_out;                                                // optional: the ConvTranspose output map (same shape), written for parity tests
};
bool cfen_up_conv3_fused_supported(int dtype, int cs_in, int Cup_pad, int cs_up, int C3_pad, int Hin, int Win);
int cfen_up_conv3_fused_impl_g(int dtype, int ng, const CfenUpConv3* u, hipStream_t s);
// the whole tail in one launch: ConvTranspose + 3x3 + reflect-pad 7x7 + tanh, both intermediate maps in LDS (k_tail.hip); d7 = the 7x7's descriptor as for cfen_conv7_tz_impl_g
struct ConvDesc;
bool cfen_tail_fused_supported(int dtype, int cs_in, int Cup_pad, int cs_up, int C3_pad, int Hin, int Win, int Cout7, int out_mode);
int cfen_tail_fused_impl_g(int dtype, int ng, const CfenUpConv3* u, const ConvDesc* d7, hipStream_t s);
// out (B, h, w, cs_out) = 4 x 4 mean of in (B, 4h, 4w, cs_in): GViT's avgpool . avgpool as a map (k_tokens.hip: k_pool4)
int cfen_pool4_impl_g(int dtype, int ng, const void* const* in, void* const* out, int B, int h, int w, int C, int cs_in, int cs_out, hipStream_t s);
