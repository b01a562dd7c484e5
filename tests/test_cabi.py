"""The C-ABI library loads and exports every symbol include/cfen_hip.h declares (no compute calls: runs
without a GPU), and the ctypes signature table covers exactly that set."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "cfen_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cfen_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    from cfen_vit_dehazing_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    syms = declared_symbols()
    assert len(syms) >= 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), "libcfen_hip.so does not export %s" % s
    assert sorted(_lib.SIGNATURES) == syms
    assert _lib.load().cfen_abi_version() == 1


def test_every_header_has_its_own_table_and_the_tables_are_apart():
    """the ledger of _lib.HEADERS: every header under include/ that declares a function has a table, every table holds exactly what its header
    declares, no two tables share a name, and the core is the frozen one.  A new header fails here until it has a table of its own."""
    import glob
    import itertools
    import cabi_ledger
    _lib = cabi_ledger.library()
    declared = {os.path.basename(p): cabi_ledger.header_functions(os.path.basename(p)) for p in glob.glob(os.path.join(ROOT, "include", "cfen_*.h"))}
    assert {h for h, fns in declared.items() if fns} == set(_lib.HEADERS)
    for (h1, t1), (h2, t2) in itertools.combinations(_lib.HEADERS.items(), 2):
        assert not set(t1) & set(t2), (h1, h2)
    for header, table in _lib.HEADERS.items():
        assert sorted(declared[header]) == sorted(table), header
    assert _lib.SIGNATURES is _lib.HEADERS["cfen_hip.h"] and len(_lib.SIGNATURES) == 68 and sorted(_lib.SIGNATURES) == declared_symbols()
    assert _lib.load().cfen_abi_version() == 1


def test_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    cfg = _lib.NetConfigC(batch=1, n_feats=24, hidden_dim_ratio=4, patch_size=32, load_size=250, num_heads=4, dtype=1, reserved=0)
    h = ctypes.c_void_p()
    assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cfg)) == -1          # loadSize != 8*patch_size
    assert b"loadSize" in lib.cfen_last_error()
    cfg.load_size = 256
    assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
    assert lib.cfen_net_workspace_bytes(h) > 0
    assert abs(lib.cfen_net_flops_per_image(h) / 1e9 - 120.85) < 0.01           # SURVEY 8d closed form
    assert lib.cfen_net_set_param(h, b"no.such.param", ctypes.c_void_p(16), 4) == -1
    buf = ctypes.create_string_buffer(1 << 16)
    assert lib.cfen_net_missing_params(h, buf, 1 << 16) == 690   # (+ 1: head.0.0.w5, the 8-byte-pixel layout of k_head5; + 4 level-1 GViT blocks x 5 fragment-stream layouts, round 4) (+ 4 level-3 LViT blocks x 5 and 4 level-2 blocks x 3 fragment-stream layouts, round 3; the window kernel's three layouts became one stream) 24 transformer blocks x 21 + 15 conv layers x 3 ... + 8 LViT blocks with the extra fused-front layouts (2 each) + 4 level-1 LViT blocks x 1 window-kernel weight stream + 16 unfused blocks (GViT, LViT-3) x 6 LayerNorm-folded entries
    lib.cfen_net_destroy(h)
    for hdr, gf in ((2, 85.07),):
        cfg.hidden_dim_ratio = hdr
        assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
        assert abs(lib.cfen_net_flops_per_image(h) / 1e9 - gf) < 0.01
        lib.cfen_net_destroy(h)
    cfg.hidden_dim_ratio, cfg.patch_size, cfg.load_size = 4, 64, 512
    assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cfg)) == 0
    assert abs(lib.cfen_net_flops_per_image(h) / 1e9 - 624.21) < 0.01
    lib.cfen_net_destroy(h)


def test_tuning_knobs_validate_without_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    assert lib.cfen_tune(b"no.such.knob", 1) == -1 and b"unknown key" in lib.cfen_last_error()
    assert lib.cfen_tune(b"gemm.kernel", 99) == -1
    assert lib.cfen_tune(b"gemm.large", 1) == -1            # tile ids are 2..5 (+10 / +20 for deeper rings)
    assert lib.cfen_tune(b"net.tail_fused", 3) == -1 and lib.cfen_tune(b"tail.segments", 0) == -1 and lib.cfen_tune(b"gemm.mid", 7) == -1
    for key, val in ((b"gemm.kernel", -1), (b"gemm.large", 4), (b"gemm.small", 15), (b"gemm.mid", 2), (b"gemm.splitk", 0), (b"mlp.small_tiles", 10),
                     (b"net.attn_head_major", 1), (b"net.embed_gather", 1), (b"net.fused_front_max_dim", 192), (b"net.skip_classes", 0),
                     (b"net.tail_fused", 2), (b"tail.segments", 1), (b"tail.balance", 0), (b"tail.debug", 0), (b"net.skip_from", -1), (b"net.skip_to", -1),
                     (b"net.extra_launches", 0), (b"net.gvit_dummy_levels", 0)):
        assert lib.cfen_tune(key, val) == 0, key       # (the shipped defaults: the knobs are process-wide)



# The 61 knobs of the table (csrc/cfen_tune_knobs.hpp), as the strcmp ladder of cfen_tune() spelled them before the table existed.
KNOB_KEYS = """gemm.kernel gemm.large gemm.small gemm.mid gemm.big convT.tpw conv7.tpw conv.wlds conv.wlds_maxlog gemm.big_min_tiles embed.lds embed.stages
    mlp3.tm192 embed.defer_refill gemm.defer_refill lvit.debug front3.debug mlp3.pair mlp3.debug gemm.m128 gemm.splitk_stages gemm.splitk_release gemm.splitk
    net.ln_fold net.fused_front_max_dim net.skip_classes mlp.small_tiles lvit.shape net.lvit_window net.fold_in_gemm net.attn_head_major dcn.tps gemm.nt dcn.tile
    attn.hm_pair net.head_fused net.stream_front net.stream_mlp192 net.stream_mlp net.gvit_dummy_wgs net.gvit_dummy_us net.skip_from net.skip_to
    net.extra_launches net.gvit_dummy_levels net.gvit_dummy_stream gvit.team net.gvit_stream gvit.max_concurrent net.tail_fused tail.balance tail.debug
    tail.segments net.up_fused net.zero_memset net.keep_stages net.resblock_fused net.head5 gvit.debug net.gvit_chain net.embed_gather""".split()
# The defaults the GPU tests spelled out in their `finally:` blocks for six rounds (they restore through ops.tuning now and know none): pinned here so
# the table cannot drift silently from them.  "net.resblock_fused" is the one those tests had wrong (they restored 1; the library ships 0).
PINNED_DEFAULTS = {"gemm.splitk": 0, "gemm.splitk_release": 1, "gemm.kernel": -1, "gemm.big": 0, "gemm.big_min_tiles": 256, "attn.hm_pair": 0, "embed.lds": 6,
                   "embed.stages": 4, "conv.wlds": 2, "conv7.tpw": 4, "convT.tpw": 2, "mlp3.tm192": 22, "mlp3.pair": 1, "lvit.shape": 2, "net.head_fused": 0,
                   "net.head5": 1, "net.tail_fused": 2, "net.keep_stages": 0, "tail.segments": 1, "net.up_fused": 0, "net.gvit_stream": 2,
                   "gvit.max_concurrent": 1, "dcn.tile": 1, "net.resblock_fused": 0}


def _query(lib, key):
    value, shipped = ctypes.c_int(-12345), ctypes.c_int(-12345)
    assert lib.cfen_tune_query(key.encode(), ctypes.byref(value), ctypes.byref(shipped)) == 0, key
    return value.value, shipped.value


def test_knob_enumeration_is_the_61_keys():
    from cfen_vit_dehazing_amd import _lib, ops
    lib = _lib.load()
    keys = ops.tune_keys()
    assert len(keys) == 61 and len(set(keys)) == 61
    assert sorted(keys) == sorted(KNOB_KEYS)
    assert lib.cfen_tune_key(61) is None and lib.cfen_tune_key(-1) is None and lib.cfen_tune_key(1 << 30) is None
    assert lib.cfen_tune_query(b"no.such.knob", None, None) == -1 and b"unknown key" in lib.cfen_last_error()
    assert lib.cfen_tune_query(b"gemm.kernel", None, None) == 0            # either pointer may be NULL


def test_every_knob_is_swept_or_excused():
    """the ledger of tests/test_hip_variants.py: every key of the library's table is either swept by that module's GPU tests (SWEPT: key -> the values they
    run, each accepted by the knob's rule, at least one of them not the shipped default) or excused in EXCLUDED with a reason.  A new knob row fails here until someone
    tests or excuses it."""
    from cfen_vit_dehazing_amd import _lib, ops
    import test_hip_variants as tv
    lib = _lib.load()
    keys = ops.tune_keys()
    assert sorted(keys) == sorted(KNOB_KEYS)
    missing = [k for k in keys if k not in tv.SWEPT and k not in tv.EXCLUDED]
    assert not missing, "knobs neither swept by tests/test_hip_variants.py nor excused in its EXCLUDED: %r" % missing
    assert not set(tv.SWEPT) & set(tv.EXCLUDED) and not (set(tv.SWEPT) | set(tv.EXCLUDED)) - set(keys)
    assert all(isinstance(r, str) and len(r) > 10 and "\n" not in r for r in tv.EXCLUDED.values())
    assert "gemm.splitk_stages" in tv.EXCLUDED and "no launcher" in tv.EXCLUDED["gemm.splitk_stages"]
    for key, values in tv.SWEPT.items():
        before, shipped = _query(lib, key)
        assert any(v != shipped for v in values), key
        for v in values:                        # (validation only: nothing launches)
            assert lib.cfen_tune(key.encode(), v) == 0, (key, v, lib.cfen_last_error())
        assert lib.cfen_tune(key.encode(), before) == 0
    # what the GPU tests iterate is what the ledger shows: every value of SWEPT comes from the operator sweeps or the launch-plan sweeps, and every launch-plan
    # case (key, value, kind of net) is run by one of the two parametrised tests -- by name, or among the settings that keep the kernel names (NET_DEAD)
    for key, values in tv.SWEPT.items():
        assert set(values) == set(tv.OP_SWEPT.get(key, ())) | set(tv.NET_SWEPT.get(key, ())), key
    assert set(tv.OP_SWEPT) | set(tv.NET_SWEPT) == set(tv.SWEPT)
    for key, values in tv.NET_SWEPT.items():
        for v in values:
            assert [c for c in tv.NET_CASES if c[:2] == (key, v)], "launch-plan setting %s = %d has no case" % (key, v)
    for case, (needs, reason) in tv.NET_DEAD.items():
        assert case in tv.NET_CASES, "NET_DEAD names a case that is not swept: %r" % (case,)
        assert (needs is None or needs.startswith("k_")) and isinstance(reason, str) and len(reason) > 10, case


# functions of the header that launch nothing on the device: queries, set-up and host-side settings
HOST_ONLY = """cfen_abi_version cfen_last_error cfen_tune cfen_tune_query cfen_tune_key cfen_net_create cfen_net_destroy cfen_net_workspace_bytes
    cfen_net_set_param cfen_net_actnorm_pending cfen_net_actnorm_pending_count cfen_net_set_input_u8 cfen_net_set_output_u8 cfen_net_set_output_f16
    cfen_net_missing_params cfen_net_profile_entry cfen_net_profile_entry_kernel cfen_net_stage cfen_net_chain_error_words cfen_net_flops_per_image
    cfen_image_metrics_bytes cfen_image_msssim_bytes cfen_png_workspace_bytes cfen_stats_workspace cfen_deform_conv_columns_bytes
    cfen_deform_conv_backward_bytes cfen_deform_conv_backward_set_lds""".split()


def test_every_kernel_launching_entry_point_is_guard_band_tested_or_excused():
    """the ledger of tests/test_hip_bounds.py: every function of include/cfen_hip.h that launches a kernel is run between guard bands by a test of that
    module (COVERED: entry point -> test) or excused in its NOT_COVERED with a reason.  A new entry point fails here until someone does one or the other."""
    import test_hip_bounds as tb
    syms = declared_symbols()
    assert not set(HOST_ONLY) - set(syms), "HOST_ONLY names functions the header does not declare: %r" % sorted(set(HOST_ONLY) - set(syms))
    launching = set(syms) - set(HOST_ONLY)
    missing = sorted(launching - set(tb.COVERED) - set(tb.NOT_COVERED))
    assert not missing, "entry points neither run by tests/test_hip_bounds.py nor excused in its NOT_COVERED: %r" % missing
    assert not set(tb.COVERED) & set(tb.NOT_COVERED) and not (set(tb.COVERED) | set(tb.NOT_COVERED)) - launching
    assert all(isinstance(r, str) and len(r) > 10 and "\n" not in r for r in tb.NOT_COVERED.values())
    # the test a COVERED entry names is the one that makes the call: by the ops wrapper of that name, or through the C ABI
    how = {"cfen_embed_qkv_stream": ("stream_weights=True",), "cfen_instnorm_relu": ("ops.instnorm_relu_(",)}
    for sym, test in tb.COVERED.items():
        fn = getattr(tb, test, None)
        assert callable(fn) and test.startswith("test_"), (sym, test)
        body = inspect.getsource(fn)
        calls = how.get(sym, ("ops.%s(" % sym[len("cfen_"):], "lib.%s(" % sym))
        assert any(c in body for c in calls), "%s of tests/test_hip_bounds.py does not call %s" % (test, sym)


def test_a_caller_placed_output_is_validated():
    """ops._out, behind every wrapper's out=: a fresh tensor by default (zeroed where the wrapper always handed its kernel a zeroed one), the caller's tensor
    if it fits, ValueError naming the operator for a wrong shape, dtype or device, a non-contiguous tensor and something that is no tensor"""
    import torch
    from cfen_vit_dehazing_amd import ops
    cpu = torch.device("cpu")
    fresh = ops._out(None, (3, 5), torch.float16, cpu, "op")
    assert fresh.shape == (3, 5) and fresh.dtype == torch.float16 and fresh.device == cpu and fresh.is_contiguous()
    assert not ops._out(None, (3, 5), torch.float32, cpu, "op", zero=True).any()
    mine = torch.empty(3, 5, dtype=torch.float16)
    assert ops._out(mine, (3, 5), torch.float16, cpu, "op") is mine
    assert ops._out(mine, torch.Size([3, 5]), torch.float16, cpu, "op") is mine
    bad = {"shape": torch.empty(3, 6, dtype=torch.float16), "rank": torch.empty(15, dtype=torch.float16), "dtype": torch.empty(3, 5, dtype=torch.float32),
           "device": torch.empty(3, 5, dtype=torch.float16, device="meta"), "strides": torch.empty(5, 3, dtype=torch.float16).t(),
           "no tensor": [[0.0] * 5] * 3}
    assert bad["strides"].shape == (3, 5) and not bad["strides"].is_contiguous()
    for what, t in bad.items():
        with pytest.raises(ValueError, match="some_op: out must be a contiguous torch.float16 tensor of shape"):
            ops._out(t, (3, 5), torch.float16, cpu, "some_op")


def test_knobs_of_a_fresh_process_are_at_their_shipped_defaults():
    """in an interpreter of its own, so that no test that ran before in this process can matter"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from cfen_vit_dehazing_amd import ops\n"
            "keys = ops.tune_keys()\n"
            "assert len(keys) == 61 and not ops.tune_not_shipped(), ops.tune_not_shipped()\n"
            "print('fresh ok', len(keys))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fresh ok 61" in r.stdout, r.stdout + r.stderr


def test_every_knob_takes_its_own_default_and_pinned_defaults_hold():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    before = {k: _query(lib, k) for k in KNOB_KEYS}
    for k, (_, shipped) in before.items():
        assert lib.cfen_tune(k.encode(), shipped) == 0, (k, shipped, lib.cfen_last_error())
        assert _query(lib, k) == (shipped, shipped), k
    for k, (value, _) in before.items():          # (put back whatever an earlier test of this process left: this test changes nothing for good)
        assert lib.cfen_tune(k.encode(), value) == 0
    assert {k: _query(lib, k) for k in KNOB_KEYS} == before
    assert {k: before[k][1] for k in PINNED_DEFAULTS} == PINNED_DEFAULTS


def test_knob_values_are_normalised_and_a_refused_value_changes_nothing():
    from cfen_vit_dehazing_amd import _lib, ops
    lib = _lib.load()
    with ops.tuning({"net.head5": 7, "embed.lds": 15, "net.keep_stages": -3}):
        assert ops.tuned("net.head5") == 1 and ops.tuned("embed.lds") == 7 and ops.tuned("net.keep_stages") == 1
    for key, refused in (("gemm.kernel", 26), ("gemm.kernel", -2), ("gemm.mid", 7), ("gemm.big", 1), ("gemm.m128", 5), ("gemm.splitk_stages", 1), ("mlp3.tm192", 23),
                         ("embed.stages", 6), ("net.stream_front", 3), ("net.gvit_stream", -1), ("tail.segments", 65), ("gvit.team", 86), ("gvit.max_concurrent", 9),
                         ("convT.tpw", 0), ("conv7.tpw", 0), ("gemm.big_min_tiles", 0), ("conv.wlds", -1), ("conv.wlds_maxlog", -1)):
        before = ops.tuned(key)
        assert lib.cfen_tune(key.encode(), refused) == -1, (key, refused)
        assert key.encode() in lib.cfen_last_error() and ops.tuned(key) == before, key


def test_tuning_context_restores_previous_values():
    from cfen_vit_dehazing_amd import ops
    from cfen_vit_dehazing_amd._lib import CfenError
    start = {k: ops.tuned(k) for k in KNOB_KEYS}
    with ops.tuning({"tail.segments": 4}):
        with ops.tuning({"tail.segments": 8, "net.tail_fused": 0}):          # nests: the inner block gives back the OUTER block's value, not the default
            assert (ops.tuned("tail.segments"), ops.tuned("net.tail_fused")) == (8, 0)
        assert (ops.tuned("tail.segments"), ops.tuned("net.tail_fused")) == (4, start["net.tail_fused"])
        with pytest.raises(ZeroDivisionError):                                 # an exception in the body
            with ops.tuning({"tail.segments": 2, "conv.wlds": 0}):
                1 / 0
        assert (ops.tuned("tail.segments"), ops.tuned("conv.wlds")) == (4, start["conv.wlds"])
        with pytest.raises(CfenError, match="gemm.big"):                       # a refused key: the sets already made are undone, the body never runs
            with ops.tuning({"tail.segments": 16, "gemm.big": 1, "conv.wlds": 0}):
                raise AssertionError("the body must not run")
        assert (ops.tuned("tail.segments"), ops.tuned("conv.wlds")) == (4, start["conv.wlds"])
    assert {k: ops.tuned(k) for k in KNOB_KEYS} == start


def _pack_and_register(cfg, dtype, wtile):
    import torch
    from cfen_vit_dehazing_amd import _lib
    from cfen_vit_dehazing_amd.hipnet import _VARIANT_CODE
    from cfen_vit_dehazing_amd.manifest import generate_state_dict
    from cfen_vit_dehazing_amd.packing import pack_state_dict
    lib = _lib.load()
    td = torch.float16 if dtype == "fp16" else torch.float32
    packed = pack_state_dict(generate_state_dict(cfg, seed=0, with_dead=False), cfg, td, wtile=wtile)
    cc = _lib.NetConfigC(batch=2, n_feats=cfg.n_feats, hidden_dim_ratio=cfg.hidden_dim_ratio, patch_size=cfg.patch_size, load_size=cfg.load_size,
                         num_heads=cfg.num_heads, dtype=_lib.dtype_code(td), reserved=(_VARIANT_CODE[cfg.variant] << 8) | (2 if wtile else 0))
    h = ctypes.c_void_p()
    assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cc)) == 0, lib.cfen_last_error()
    keep = {}
    for name, t in packed.items():
        if isinstance(t, str):
            t = packed[t[1:]]
        keep[name] = t = t.contiguous()
        assert lib.cfen_net_set_param(h, name.encode(), ctypes.c_void_p(t.data_ptr()), t.numel() * t.element_size()) == 0, lib.cfen_last_error()
    buf = ctypes.create_string_buffer(1 << 16)
    assert lib.cfen_net_missing_params(h, buf, 1 << 16) == 0, buf.value[:400]
    lib.cfen_net_destroy(h)


@pytest.mark.parametrize("variant,wtile", [("v3", False), ("v3", True), ("cfs", False), ("crs", False), ("v5", False), ("v5", True)])
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_packed_parameters_are_exactly_what_the_launch_plan_asks_for(variant, wtile, dtype):
    """packing.pack_state_dict (host) and cfen_net::build (csrc/cfen_net.cpp) must agree on every packed name and byte size, for each of
    the four generators; set_param only records the pointer, so this runs without a GPU"""
    from cfen_vit_dehazing_amd.config import NetConfig
    _pack_and_register(NetConfig(24, 4, patch_size=8, load_size=64, variant=variant), dtype, wtile)


@pytest.mark.parametrize("n_feats,hdr,patch,dtype", [(24, 3, 32, "fp16"), (24, 1, 32, "fp16"), (8, 4, 8, "fp16"), (8, 4, 8, "fp32"), (16, 3, 8, "fp16"),
                                                    (32, 2, 8, "fp16")])
def test_packed_parameters_match_the_plan_where_the_fused_kernels_do_not_apply(n_feats, hdr, patch, dtype):
    """the host predicates (packing.window_fusable / mlp_is_fused / front_is_fused / mlp_is_streamed, the LayerNorm fold's 128-byte rule)
    mirror cfen_net::build also off the benchmarked shape: odd hidden_dim_ratio at the window kernel's geometry (hidden % 64 != 0),
    embedding dims whose rows are not whole 128-byte K steps (n_feats 8: D = 32, 128), and the D = 384 fragment-stream blocks"""
    from cfen_vit_dehazing_amd.config import NetConfig
    _pack_and_register(NetConfig(n_feats, hdr, patch_size=patch, load_size=8 * patch), dtype, True)


@pytest.mark.parametrize("n_feats,num_heads,dtype,flag", [(40, 4, "fp16", b"n_feats"), (40, 4, "fp32", b"n_feats"),
                                                          (24, 8, "fp16", b"--num_heads 8"), (16, 16, "fp16", b"--num_heads 16"),
                                                          (32, 2, "fp16", b"--num_heads 2"), (32, 2, "fp32", b"--num_heads 2")])
def test_configurations_the_kernels_cannot_run_are_refused_at_create(n_feats, num_heads, dtype, flag):
    """refused by cfen_net_create (host-side plan build, no launch), with a message that names the flag: n_feats 40 (token rows over 128
    elements), head dims the attention kernels do not take -- 12 (n_feats 24, 8 heads) and 4 (n_feats 16, 16 heads) are not multiples of the
    fp16 fragment width of 8, GViT-1 of n_feats 32 at 2 heads has a head dim of 256 > 128"""
    import torch
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    cc = _lib.NetConfigC(batch=1, n_feats=n_feats, hidden_dim_ratio=4, patch_size=8, load_size=64, num_heads=num_heads,
                         dtype=_lib.dtype_code(torch.float16 if dtype == "fp16" else torch.float32), reserved=0)
    h = ctypes.c_void_p()
    assert lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cc)) == -1
    assert flag in lib.cfen_last_error(), lib.cfen_last_error()


@pytest.mark.parametrize("n_feats,num_heads,dtype,flag", [(40, 4, "fp32", "n_feats"), (24, 8, "fp16", "--num_heads 8"), (16, 16, "fp16", "--num_heads 16"),
                                                          (32, 2, "fp32", "--num_heads 2")])
def test_dec_ipt_refuses_them_when_it_is_built(n_feats, num_heads, dtype, flag):
    """dec_ipt(cfg, compute_dtype=...) checks the launch plan on construction, before any weights move to the device or any kernel launches"""
    from cfen_vit_dehazing_amd._lib import CfenError
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    with pytest.raises(CfenError, match=flag):
        dec_ipt(NetConfig(n_feats, 4, patch_size=8, load_size=64, num_heads=num_heads), compute_dtype=dtype)


def test_switching_to_a_dtype_the_heads_do_not_fit_is_refused():
    """n_feats 24 at 8 heads: LViT head dim 12 runs in fp32 (fragment width 4), not in fp16 (8); the switch is refused, the net stays fp32"""
    import torch
    from cfen_vit_dehazing_amd._lib import CfenError
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    net = dec_ipt(NetConfig(24, 4, patch_size=8, load_size=64, num_heads=8), compute_dtype="fp32")
    with pytest.raises(CfenError, match="--num_heads 8"):
        net.set_compute_dtype("fp16")
    assert net.compute_dtype == torch.float32


@pytest.mark.parametrize("n_feats,hdr,num_heads,dtype", [(32, 6, 4, "fp16"), (32, 6, 4, "fp32"), (32, 6, 8, "fp16"), (16, 3, 4, "fp16"),
                                                         (8, 4, 4, "fp16"), (8, 1, 4, "fp32"), (16, 4, 16, "fp32")])
def test_configurations_the_kernels_run_are_accepted(n_feats, hdr, num_heads, dtype):
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    dec_ipt(NetConfig(n_feats, hdr, patch_size=8, load_size=64, num_heads=num_heads), compute_dtype=dtype)
