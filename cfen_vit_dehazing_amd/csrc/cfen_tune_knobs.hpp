// THE table of the process-wide kernel-variant knobs (cfen_tune, include/cfen_hip.h): one row per knob, and the only place where a
// knob's identifier, key, shipped default, accepted values and meaning are written down.
//
//   CFEN_KNOB(ident, "key", shipped default, rule)
//
// Included plainly (cfen_internal.hpp does) it declares the accessors `int& cfen_tune_<ident>()` the launchers read.  cfen_tune.cpp
// includes it again with its own CFEN_KNOB for the storage, the key lookup and the validation behind cfen_tune / cfen_tune_query /
// cfen_tune_key.  A new knob is one new row here, nothing else.
//
// Rules (a refused value leaves the knob unchanged):
//   any_int()           every value, stored as given
//   on_off()            every value, stored as value != 0
//   low_bits(m)         every value, stored as value & m
//   range(lo, hi)       lo <= value <= hi
//   at_least(lo)        value >= lo
//   one_of({a, b, ..})  exactly these values
//
// "Default" in a comment below means the value in the row; where a default was chosen by a measurement, the measurement is here.
// Knobs marked "results invalid" are timing experiments: they leave work out, so the outputs are wrong on purpose.
//
// No #pragma once, on purpose: every include expands the rows with the CFEN_KNOB in force (repeated declarations are legal).  CFEN_KNOB and
// CFEN_GEMM_TILE_IDS belong to this file: nothing else may define them, except cfen_tune.cpp around its own includes of the table.
#ifndef CFEN_KNOB
#define CFEN_KNOB(ident, key, shipped, rule) int& cfen_tune_##ident();
#define CFEN_KNOB_DECLARATIONS_ONLY
#endif
// k_gemm_dma tile ids: 2 = 96 x 128 (features x tokens), 3 = 96 x 96, 4 = 96 x 64, 5 = 96 x 32; +10 / +20 for 3 / 4 LDS stages instead of 2;
// 34 = tile 4 with 5 stages, 45 / 65 = tile 5 with 6 / 8 stages
#define CFEN_GEMM_TILE_IDS one_of({2, 3, 4, 5, 12, 13, 14, 15, 22, 23, 24, 25, 32, 34, 45, 65})

// ---- token GEMMs (k_gemm.hip) -----------------------------------------------------------------------------------------------------
// -1 (default) choose by shape, 0 register-staged k_gemm_nt, 1 k_gemm_skinny, 2 .. 5 LDS-DMA k_gemm_dma with that tile id (+10 per extra
// stage); 1 .. 5 need K * element size to be a multiple of 128 bytes
CFEN_KNOB(gemm_kernel, "gemm.kernel", -1, range(-1, 25))
// the tile the shape rule uses for problems with >= 1024 tiles of 96 x 64 (LViT): occupancy (4 workgroups a CU) wins
CFEN_KNOB(gemm_large, "gemm.large", 4, CFEN_GEMM_TILE_IDS)
// ... with at most 512 tiles of 96 x 32.  15 = 96 x 32 tiles, 3-stage ring: the few-token GViT GEMMs are latency bound (one K-step per
// memory round trip with 2 stages)
CFEN_KNOB(gemm_small, "gemm.small", 15, CFEN_GEMM_TILE_IDS)
// ... with more than 512 tiles of 96 x 32 and fewer than 1024 of 96 x 64 (the grouped GViT-2 decoder GEMMs, 3 x 512 tokens).
// Round 5, four forwards in flight, same box: 96 x 128 tiles (2) 2.059 / 2.060 ms per step, 96 x 64 (4) 2.094, 96 x 96 (3) 2.106, 96 x 32 on
// 2 / 3 stages (5 / 15: rounds 2-4) 2.075-2.078 / 2.136 (profiles/r05_ab_gvit2_decoder_gemm_tiles.txt): a quarter of the weight bytes
// through the DMA path
CFEN_KNOB(gemm_mid, "gemm.mid", 2, CFEN_GEMM_TILE_IDS)
// many-token GEMMs with N >= 768: 0 (default) off; 6: 192 x 128 tiles, 2-stage ring (80 KB of LDS, two workgroups a CU).  MEASURED
// (MI355X, B = 8, round 2): the LViT-3 / GViT-1 qkv, ffn1, head1 GEMMs are 5 - 25 % SLOWER on it (ln1_qkv x3 60 -> 76 us, ln2_ffn1 x3
// 75 -> 80 us; a 3-stage one-workgroup-a-CU variant 104 / 119 us): with K = 384 a tile is 6 dependent K-steps, the kernel is bound by the
// latency of that chain and what hides it is the number of workgroups a CU holds, not the bytes or LDS reads per flop.  Kept as a tested
// variant.
CFEN_KNOB(gemm_big, "gemm.big", 0, one_of({0, 6}))
// ... used when a launch has at least this many 192 x 128 tiles
CFEN_KNOB(gemm_big_min_tiles, "gemm.big_min_tiles", 256, at_least(1))
// experiment: problems of <= 128 tokens take this tile id (+10 per extra stage; 2 = 96 x 128: every weight byte is pulled by ONE
// workgroup); 0 = shape rule
CFEN_KNOB(gemm_m128, "gemm.m128", 0, one_of({0, 2, 32, 3, 4, 14, 34}))
// weight rows of k_gemm_dma by non-temporal LDS-DMA: 0 never, 1 few-token GEMMs (M <= 512: GViT levels 2 and 3), 2 always
CFEN_KNOB(gemm_nt, "gemm.nt", 0, any_int())
// k_gemm_dma: 1 = a K-step's refill behind its first fragment reads, 0 = right behind the barrier (rounds 2-5)
CFEN_KNOB(gemm_defer_refill, "gemm.defer_refill", 1, on_off())
// 1 = round 3's shape rule: K-heavy few-token GEMMs inside the net run split-K with the in-launch reduction (scratch from the workspace).
// 0 (default, round 4): with several forwards in flight the unsplit launches are faster (2.13 against 2.16 ms per step, and 2.80 with the
// release fence below: a split launch is more workgroups, and CU-time is what a forward costs there); bitwise right either way, DESIGN 4.4
CFEN_KNOB(gemm_splitk, "gemm.splitk", 0, on_off())
// extra ring stages of the 96 x 128 split-K tile: 0 (two stages) or 3 (five stages, 140 KB)
CFEN_KNOB(gemm_splitk_stages, "gemm.splitk_stages", 0, one_of({0, 3}))
// 1 (default): every K slice runs an agent-scope release fence before its arrival ticket -- the memory model's recipe;
// 0 = round 3's publish (write-through slab stores + a vmcnt drain, the guide's "measured, not an architectural guarantee" row): also
// right in every test here, 57.7 -> 22.0 us on a 1024-workgroup launch.  (Round 4 blamed this seam for wrong outputs with two forwards in
// flight; the cause was the counters' zeroing as a graph MEMSET node: "net.zero_memset".)  The persistent chain (k_gvit.hip) reads it too.
CFEN_KNOB(gemm_splitk_release, "gemm.splitk_release", 1, any_int())

// ---- convolutions (k_conv.hip, k_conv_tile.hip) ---------------------------------------------------------------------------------------
// tiles per workgroup of the 128-byte k_convT_tile variant
CFEN_KNOB(convT_tpw, "convT.tpw", 2, at_least(1))
// tiles per workgroup of the Toeplitz 7x7 kernel k_conv7_tz
CFEN_KNOB(conv7_tpw, "conv7.tpw", 4, at_least(1))
// gather convs stage their weight matrix in LDS: 0 never, 1 matrices up to 60 KB, 2 up to 150 KB
CFEN_KNOB(conv_wlds, "conv.wlds", 2, at_least(0))
// ... only for launches below 2^this pixels
CFEN_KNOB(conv_wlds_maxlog, "conv.wlds_maxlog", 40, at_least(0))

// ---- LViT front half (k_embed.hip) ------------------------------------------------------------------------------------------------
// bit 2: the LDS-DMA-ring front half k_embed_qkv2; else k_embed_qkv stages its weights through LDS for D = 96 (bit 0) / D = 192 (bit 1)
CFEN_KNOB(embed_lds, "embed.lds", 6, low_bits(7))
// LDS-DMA ring stages of k_embed_qkv2 at D = 192: 2 (rounds 2-4), 3, 4 (default, round 5), 5
CFEN_KNOB(embed_stages, "embed.stages", 4, range(2, 5))
// k_embed_qkv2: 1 = refill behind the chunk's first fragment reads, 0 = right behind the barrier (rounds 2-5)
CFEN_KNOB(embed_defer_refill, "embed.defer_refill", 1, on_off())

// ---- fused MLP blocks (k_mlp.hip, k_stream.hip) ---------------------------------------------------------------------------------------
// fused-MLP kernel variant at D = 96 / 192: 0 .. 4 the register-staged k_mlp tilings, >= 10 the LDS-DMA k_mlp2 (tens digit: D = 96 variant,
// ones digit: D = 192 variant; the list is at launch_mlp in k_mlp.hip)
CFEN_KNOB(mlp_small_tiles, "mlp.small_tiles", 10, any_int())
// k_mlp3 at D = 192 (LViT level 2): 22 (default, round 5) = 2 token tiles a wave at 256 registers on a three-slot ring, two 78 KB workgroups
// a CU; 24 = the same on four slots (one 102 KB workgroup a CU); 25 = 22 with the D = 384 kernel's refill placement (round-6 A/B); 28 = ONE
// 8-wave workgroup a CU sharing one three-slot ring; 4 / 3 / 2 token tiles a wave on the six-slot ring of one 150 KB workgroup a CU (512
// registers)
CFEN_KNOB(mlp3_tm192, "mlp3.tm192", 22, one_of({2, 3, 4, 22, 24, 25, 28}))
// the D = 384 block (projection + LayerNorm + both stages) on k_mlp3p (two waves per SIMD, the hidden dimension split over a wave pair):
// 0 = k_mlp3<24, ...> (one wave per SIMD; results equal to 1-2 fp16 ulp: the LayerNorm sums associate over the pair), 1 on (default,
// round 6: 134-150 us a launch against 152-172; +0.6-1.0 % on the headline step, level on the other two configurations), 2 = k_mlp3p's
// stamped timing build (prints to stderr, synchronises)
CFEN_KNOB(mlp3_pair, "mlp3.pair", 1, any_int())
// k_mlp3 timing experiments (results invalid): 1 no DMA refills, 2 no MFMAs; 64 .. 72 per-phase stamps (tools/dbg_mlp3_stamps.py)
CFEN_KNOB(mlp3_debug, "mlp3.debug", 0, any_int())
// k_front3 timing experiments: 1 no refills, 8 no qkv stores, 24 no stores (results invalid); | 64 = section stamps to stderr
CFEN_KNOB(front3_debug, "front3.debug", 0, any_int())

// ---- LViT level 1 window kernel, attention, deformable conv ---------------------------------------------------------------------------------
// k_lvit_window's workgroup shape / schedule.  2 (default): 16 waves x 1 token tile (four waves per SIMD, 128 registers, no spills:
// 2.858 -> 2.83 ms -- a wave issues a vector instruction every ~10 cycles and two thirds of this kernel are vector-instruction bound,
// DESIGN 4.3); 0: 8 waves x 2 token tiles; 1: 4 waves x 4 token tiles (one wave per SIMD, 512 registers); 3 denominator by MFMA; 4 / 5 the
// 16 x 1 / 8 x 2 shapes with hand-issued K / V fragment reads; 6 64-row front chunks (round 5: bitwise equal, not faster); 12 the refill right
// behind the barrier; 15 double MLP chunks over the dead K / V tiles (round 6); 8 / 9 timing experiments without the softmax (results invalid)
CFEN_KNOB(lvit_shape, "lvit.shape", 2, any_int())
// k_lvit_window: 64 = section stamps of workgroup 0 to stderr
CFEN_KNOB(lvit_debug, "lvit.debug", 0, any_int())
// head-major attention: 1: 256-token windows run on k_attention_hm_long<16, 16> (two query tiles per K / V fragment, 8 waves); 2: 1024-token
// windows on 8 waves instead of 16
CFEN_KNOB(attn_hm_pair, "attn.hm_pair", 0, any_int())
// deformable conv forward: 1 (default) k_dcn_lean where its shapes allow; 0: k_dcn_nhwc (round 2)
CFEN_KNOB(dcn_tile, "dcn.tile", 1, any_int())
// taps per K slice of k_dcn_lean at most this (0: as many as fit 60 KB of LDS)
CFEN_KNOB(dcn_tps, "dcn.tps", 0, any_int())

// ---- the generator's launch plan (cfen_net.cpp); read when a forward is enqueued or a graph is built ------------------------------------
// 1 (default): LN1 / LN2 of the blocks without a fused kernel (GViT, LViT level 3) ride on the qkv / ffn1 GEMM (cfen_gemm_ln); 0 separate
// LayerNorm launches
CFEN_KNOB(ln_fold, "net.ln_fold", 1, on_off())
// k_embed_qkv is used for LViT embedding dims <= this (0 = never)
CFEN_KNOB(fused_front_max_dim, "net.fused_front_max_dim", 192, any_int())
// 1 (default): the LViT embedding GEMM gathers its patch tokens from the map; 0: separate k_patchify launch
CFEN_KNOB(embed_gather, "net.embed_gather", 1, on_off())
// 1 (default): LViT level 1 runs as one k_lvit_window launch per instance group
CFEN_KNOB(lvit_window, "net.lvit_window", 1, on_off())
// 1 (default): the last GEMM of an unfused block (mlp_head.3) stores straight into the NHWC map (fold + Join2x2), no unpatchify launch
CFEN_KNOB(fold_in_gemm, "net.fold_in_gemm", 1, on_off())
// 1 (default): LViT levels with a fused front half hand qkv to attention per (window, head); 0 row-major [M][3D]
CFEN_KNOB(attn_head_major, "net.attn_head_major", 1, on_off())
// 1: the input layout pass and head.0.0 run as one k_head5 launch where it applies
CFEN_KNOB(head5, "net.head5", 1, on_off())
// 1: the head (conv5x5 + ResBlock) runs as one k_head_fused launch where it applies.  0 (default): three k_conv_tile launches.  MEASURED
// (MI355X, batch 8): k_head_fused moves 100 MB instead of 400 MB and is SLOWER, 131 us against 108: with 3 input channels padded to 8 and
// 5 taps to 8 its MFMA work is 5x the algorithmic flops (22 % MFMA-busy, profiles/r03_*), and the unfused kernels already run at the HBM
// rate of their own maps
CFEN_KNOB(head_fused, "net.head_fused", 0, on_off())
// 1: the head's ResBlock runs as one k_resblock_fused launch where it applies.  0 (default): MEASURED with three forwards in flight 2.44
// against 2.48 ms -- the fused kernel (5-wave workgroups, 58 KB of LDS, 154 registers) is 13 us shorter alone and costs more CU-time beside
// other forwards
CFEN_KNOB(resblock_fused, "net.resblock_fused", 0, on_off())
// k_front3 for the D = 384 LViT blocks: 0 never, 1 grouped decoder launches, 2 (default, round 4) always (with three forwards in flight the
// single encoder instance on the stream kernels is 0.03 ms better: one whole-CU launch of 64 workgroups instead of 8 GEMM launches)
CFEN_KNOB(stream_front, "net.stream_front", 2, range(0, 2))
// k_mlp3 (k_stream.hip) for the D = 384 LViT blocks: 0 never, 1 launches of >= 128 workgroups (at 512 x 512 the grouped decoder launch; a
// single instance has 64 workgroups of 128 tokens: a quarter of the chip), 2 (default, round 4) always
CFEN_KNOB(stream_mlp, "net.stream_mlp", 2, range(0, 2))
// LViT level 2 (D = 192) proj + MLP block: 1 (default, round 5) on k_mlp3 (fragment-stream weights, three-slot ring; mlp3.tm192 = 22: TWO
// 78 KB workgroups a CU at 256 registers -- k_mlp2's occupancy without its two-stage ring, whose chunk period is one LDS-DMA issue ->
// landed latency: encoder 79.7 -> 56.4 us, grouped decoder launch 168.4 -> 128.2 us (961 TF), 2.148 -> 2.121 ms per step with four
// forwards in flight, profiles/r05_ab_stream_mlp192_two_wgs_per_cu.txt); 0: k_mlp2.  (k_mlp3<12, 3> on one 150 KB workgroup a CU, rounds
// 3-4: equal to k_mlp2.)
CFEN_KNOB(stream_mlp192, "net.stream_mlp192", 1, on_off())
// GViT blocks of embedding dim 384 on the LViT-3 stream kernels (k_front3 / k_mlp3, 5 launches a block): 0 never, 1 in the serial launch
// plan only, 2 (default, round 5) on every plan: which KERNELS produce the outputs no longer depends on the lane plan or on profiling
// (two-lane, serial and profiled forwards are bitwise equal; the stream kernels cost one forward at a time 2.80 -> 2.85 ms -- 277 us of
// latency against 134 -- and gain 2.27 -> 2.24 with several in flight)
CFEN_KNOB(gvit_stream, "net.gvit_stream", 2, range(0, 2))
// GViT blocks run their GEMMs as persistent chains (k_gvit.hip): 0 off, 1 (default) every GViT block, 2 the grouped decoder launches only,
// 3 the encoder blocks only, 4 every GEMM of a block as its own one-phase launch of the chain kernel (never split over K: no grid barrier, no
// split-K seam), 5 as 4 with K split so that a launch has about a workgroup per CU (the in-launch split-K seam, no grid barrier).  Every other
// value is 0.  Only nets built with fragment-stream GViT weights (cfg.reserved bit 2) can use it.
CFEN_KNOB(gvit_chain, "net.gvit_chain", 1, any_int())
// the decoders' output tails (us_conv_d01* ConvTranspose, 3x3, reflect-pad 7x7 + tanh): 0 three launches, 1 ConvTranspose + 3x3 fused
// (k_up_conv3_fused, round 4) + the 7x7, 2 (default, round 5) the whole tail in one launch (k_tail_fused, both intermediate maps in LDS)
// -- bitwise equal
CFEN_KNOB(tail_fused, "net.tail_fused", 2, range(0, 2))
// 1: GViT's x4 bilinear runs inside the level's fuse conv (k_conv UP), no k_upsample4 launch.  Default 0: measured 6 launches and 0.35 GB of
// HBM traffic fewer per forward but 0.7 % SLOWER (the 9-tap interpolation per pixel on the vector pipe in front of a K = 48 .. 192 1x1
// costs more than the copy it saves: lgcat_conv_d01 72 -> 110 us for a 19 us launch)
CFEN_KNOB(up_fused, "net.up_fused", 0, on_off())
// 1: fused launches also store the stage maps they keep on chip (us_conv_d01*), for parity tests
CFEN_KNOB(keep_stages, "net.keep_stages", 0, on_off())
// Zeroing of synchronisation words (split-K arrival counters, the chains' barrier words) in front of the launches that use them: 0
// (default) a kernel, 1 a memset.  MEASURED (round 4, MI355X, ROCm 7.2): as a hipGraph MEMSET node -- dependencies recorded like every
// kernel node's -- the zeroing is NOT ordered against its neighbouring kernel nodes once several instantiated graphs are in flight on
// different streams: counters were cleared in the middle of a launch that was counting arrivals (outputs off by 0.07 .. 0.2, no wait gave
// up), one graph at a time it is fine.  As a kernel node it is ordered.  1 is the old form, kept for the A/B
// (tests/test_hip_net.py::test_three_forwards_in_flight...; profiles/r04_ab_zero_memset.txt).
CFEN_KNOB(zero_memset, "net.zero_memset", 0, on_off())

// what-if probes for re-tuning the launch plan (timing only, results invalid)
// bit mask of kernel classes the net does NOT launch (marginal-cost timing)
CFEN_KNOB(skip_classes, "net.skip_classes", 0, any_int())
// the launches number skip_from .. skip_to of a forward are not launched
CFEN_KNOB(skip_from, "net.skip_from", -1, any_int())
CFEN_KNOB(skip_to, "net.skip_to", -1, any_int())
// that many one-workgroup 1 us launches in front of every ViT block (what a launch costs a chain)
CFEN_KNOB(extra_launches, "net.extra_launches", 0, any_int())
// GViT blocks are replaced by a launch that holds `wgs` x groups CUs for `us` microseconds (cfen_occupy_impl) ...
CFEN_KNOB(gvit_dummy_wgs, "net.gvit_dummy_wgs", 0, any_int())
CFEN_KNOB(gvit_dummy_us, "net.gvit_dummy_us", 100, any_int())
// ... and streams memory meanwhile
CFEN_KNOB(gvit_dummy_stream, "net.gvit_dummy_stream", 0, any_int())
// 1: the probe replaces only the blocks that run as a launch per GEMM (levels 2-3)
CFEN_KNOB(gvit_dummy_levels, "net.gvit_dummy_levels", 0, any_int())

// ---- persistent GViT chain (k_gvit.hip) ---------------------------------------------------------------------------------------------
// workgroups (= CUs) per GViT block of the persistent chain (three blocks share the chip)
CFEN_KNOB(gvit_team, "gvit.team", 48, range(1, 85))
// forwards of the chain plan that may be in flight at once.  A grid barrier needs its whole team resident; with several forwards of the
// chain plan in flight (replica plans on their own streams) two launches asking for more CUs than the chip has can each end up partially
// resident and spin on each other until GV_SPIN_LIMIT.  The host caps team x groups x this at 256 CUs (cfen_net.cpp) and hipnet refuses a
// replica beyond it.
CFEN_KNOB(gvit_max_concurrent, "gvit.max_concurrent", 1, range(1, 8))
// timing experiments on the chain kernel (results invalid): 1 no weight DMAs, 2 no token DMAs, 4 no fragment reads / MFMAs
CFEN_KNOB(gvit_debug, "gvit.debug", 0, any_int())

// ---- the one-launch output tail (k_tail.hip) ------------------------------------------------------------------------------------------
// work split between k_tail_fused's wave groups: bit 0 = the 7x7's scale / tanh / store of all eight rows on the ConvTranspose waves.
// In-kernel stamps (tools/dbg_tail_stamps.py): per band the ConvTranspose waves are busy 3.05 us, the 3x3 waves 4.2, the 7x7 waves 3.45 ->
// with bit 0 3.3 / 3.8 / 3.45 and the launch 8 % shorter alone (265 against 287 us), but no faster with four forwards in flight
// (2.090-2.109 against 2.084-2.092 ms)
CFEN_KNOB(tail_balance, "tail.balance", 0, any_int())
// timing experiments (results invalid): 1 no ConvTranspose MFMAs, 2 no 3x3 MFMAs, 4 no 7x7 MFMAs, 8 no tanh, 16 no output stores, 32 no
// input fetch
CFEN_KNOB(tail_debug, "tail.debug", 0, any_int())
// vertical segments a 64-column strip of k_tail_fused is cut into: more workgroups against 5 fill / drain steps per segment.  Measured,
// batch 8: alone 4 segments are fastest (202 us against 235 for 2); with four forwards in flight fewer are: 2.043-2.048 ms per step on 4,
// 2.022-2.046 on 2, 2.023-2.035 on 1
CFEN_KNOB(tail_segments, "tail.segments", 1, range(1, 64))

#undef CFEN_GEMM_TILE_IDS
#ifdef CFEN_KNOB_DECLARATIONS_ONLY
#undef CFEN_KNOB_DECLARATIONS_ONLY
#undef CFEN_KNOB
#endif
