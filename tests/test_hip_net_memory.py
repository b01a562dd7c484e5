"""The launch plan's use of memory: a forward must not depend on what its workspace, its output slab or a tile arena held before, must
not write outside them, and must not carry anything over from the forward before.

All on NetConfig(24, 4, patch_size=8, load_size=64) (T = 128, fixture tiny_nf24_hdr4): its 12-channel maps sit in a channel stride of 16, so
padding lanes exist in both dtypes.  The workspace is a guarded buffer (tests/guarded.py) of exactly cfen_net_workspace_bytes(), handed to the
net before its first forward: a fresh workspace has arbitrary contents and the first call primes its synchronisation words, so every fill is a
legal use of the ABI.

Why the non-zero fills cannot hang: the only wait on a workspace word in csrc/ is the grid barrier of k_gvit.hip, which polls the primed
barrier word and gives up after GV_SPIN_LIMIT polls; the split-K reduction of k_gemm.hip takes a ticket on a primed counter and never waits
("nobody waits for anybody").  prime_workspace (csrc/cfen_net.cpp) zeroes both regions when a net handle first sees a workspace, and every
fill below runs on a net handle of its own (net._free_nets()).

What this cannot see: an access further outside a buffer than its 64 KiB band, and an over-read whose value reaches no result."""
import ctypes
import os

import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, tiled
from cfen_vit_dehazing_amd._lib import check
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.manifest import synthetic_input
from guarded import check_bands, guarded_copy, guarded_empty
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from helpers import load_net_fixture
from test_hip_net import check_fp16_fixture, check_fp32_fixture, make_net

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FIXTURE = "tiny_nf24_hdr4"
CFG = NetConfig(24, 4, patch_size=8, load_size=64)
B = 2
FILLS = ("zero", "ff", "random")          # zero first: it is the one held against the fixture


def _fixture():
    cfg, batch, z = load_net_fixture(FIXTURE)
    assert repr(cfg) == repr(CFG) and batch == B
    return z


def stage_names(z):
    return [n for n in (str(s) for s in z["stage_names"]) if not n.startswith("tail_")]          # the tails are the outputs


def raw_stage(net, name):
    """the bytes of a stage map of the last forward as they lie in the workspace: every pixel's whole channel stride, padding lanes included"""
    h, ws, key = net._last.handle, net._last.ws, net._last.key
    p = ctypes.c_void_p()
    C, cs, H, W = (ctypes.c_int32() for _ in range(4))
    check(_lib.load().cfen_net_stage(h, name.encode(), ctypes.byref(p), ctypes.byref(C), ctypes.byref(cs), ctypes.byref(H), ctypes.byref(W)), "cfen_net_stage")
    esz = 2 if key.dtype == torch.float16 else 4
    off = p.value - ws.data_ptr()
    n = key.batch * H.value * W.value * cs.value * esz
    assert 0 <= off and off + n <= ws.numel(), "stage %s lies outside the workspace" % name
    return ws[off:off + n].clone(), C.value, cs.value


def padding_is_zero(net, name):
    raw, C, cs = raw_stage(net, name)
    if cs > C:
        lanes = raw.view(net._last.key.dtype).view(-1, cs)[:, C:]
        assert float(lanes.float().abs().max()) == 0.0, "stage %s: padding lanes %d..%d are not exact zeros" % (name, C, cs)
    return cs > C


def guard_workspace(net, x, fill):
    """replace the workspace of the net that will run `x` -- before its first forward -- by a guarded buffer of exactly the bytes the library asks for"""
    rec = net._net_for(x.shape[0], x.device, x.dtype == torch.uint8)
    nbytes = _lib.load().cfen_net_workspace_bytes(rec.handle)
    assert nbytes == rec.ws.numel()
    g = guarded_empty((nbytes,), torch.uint8, x.device, fill, name="workspace (%s)" % fill, align=256)
    rec.ws = g
    return g


def run(net, x, graph):
    if graph:
        gid, outs = net.capture(x)
        for o in outs:
            o.fill_(float("nan")) if o.dtype.is_floating_point else o.fill_(255)
        net.replay(gid)
    else:
        outs = net(x)
    torch.cuda.synchronize()
    return outs


def snapshot(net, outs, names):
    return [o.clone() for o in outs], {n: raw_stage(net, n)[0] for n in names}


def same(a, b, what):
    for k, (p, q) in enumerate(zip(a[0], b[0])):
        assert torch.equal(p, q), "%s: output %d differs" % (what, k)
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), "%s: stage %s differs (padding lanes included)" % (what, n)


def fills_agree(dtype, serial, graph, knobs=None, chain=False):
    z = _fixture()
    names = stage_names(z)
    if chain:
        os.environ["CFEN_GVIT_CHAIN"] = "1"          # read when the net is built (hipnet.dec_ipt)
    try:
        net = make_net(CFG, dtype)
    finally:
        os.environ.pop("CFEN_GVIT_CHAIN", None)
    assert net.gvit_chain == chain
    net.serial_plan = serial
    x = synthetic_input(B, CFG).to(DEV)
    settings = {"net.keep_stages": 1}
    settings.update(knobs or {})
    first = None
    with ops.tuning(settings):
        for fill in FILLS:
            net._free_nets()            # a net handle of its own per fill (it primes its workspace on first use), as a caller with a fresh workspace has
            g = guard_workspace(net, x, fill)
            outs = run(net, x, graph)
            check_bands(g)
            if chain:
                assert net.chain_errors() == [0, 0, 0]
            for o in outs:
                assert bool(torch.isfinite(o).all())
            snap = snapshot(net, outs, names)
            if fill == "zero":
                if dtype == "fp32":
                    check_fp32_fixture(FIXTURE, net, z, outs)
                else:
                    check_fp16_fixture(z, outs)
                assert any([padding_is_zero(net, n) for n in names]), "no stage of this fixture has padding lanes: the test would be blind"
                first = snap
            else:
                same(snap, first, "workspace prefilled %r against 'zero'" % fill)
    return net


@pytest.mark.parametrize("plan", ["two_lane", "serial", "graph"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_workspace_contents_do_not_matter(dtype, plan):
    """outputs and every stage map, padding lanes included, are bitwise the same whether the workspace held zeros, 0xff bytes (NaN in every float
    type) or random bytes; the zero-fill run holds the fixture's bars; nothing is written outside cfen_net_workspace_bytes()"""
    fills_agree(dtype, serial=plan == "serial", graph=plan == "graph")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_workspace_contents_do_not_matter_with_in_launch_split_k(dtype):
    fills_agree(dtype, serial=True, graph=False, knobs={"gemm.splitk": 1})


@pytest.mark.parametrize("gvit_chain", [None, 0, 4])
def test_workspace_contents_do_not_matter_on_the_chain_plan(gvit_chain):
    """CFEN_GVIT_CHAIN=1 (fp16): the persistent chains' barrier, error words and split-K slabs live in the workspace; "net.gvit_chain" 0 / 4 run the
    same weights without the grid barrier (one launch per GEMM)"""
    fills_agree("fp16", serial=True, graph=False, knobs=None if gvit_chain is None else {"net.gvit_chain": gvit_chain}, chain=True)


# ---- stale state -----------------------------------------------------------------------------------------------------------------------------
def _inputs():
    return synthetic_input(B, CFG).to(DEV), synthetic_input(B, CFG, seed0=5).to(DEV)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["fp32", "fp16", "fp16_output_u8", "fp16_output_f16"])
def test_a_forward_leaves_nothing_behind_for_the_next(kind, graph):
    """forward(A) then forward(B) on one net equals forward(B) on a fresh net, bitwise: outputs, and stage maps where the plan keeps them
    (output_u8 / output_f16 run the fused tail, which "net.keep_stages" would replace: outputs only there).  On a captured graph the input
    tensor is overwritten in place between the replays."""
    z = _fixture()
    dtype = kind.split("_")[0]
    plain = kind == dtype
    names = stage_names(z) if plain else []
    xa, xb = _inputs()

    def make():
        net = make_net(CFG, dtype)
        net.output_u8, net.output_f16 = kind.endswith("output_u8"), kind.endswith("output_f16")
        return net

    with ops.tuning({"net.keep_stages": 1} if plain else {}):
        fresh = make()
        want = snapshot(fresh, run(fresh, xb.clone(), False), names)
        used = make()
        if graph:
            x = xa.clone()
            gid, outs = used.capture(x)
            used.replay(gid)
            torch.cuda.synchronize()
            x.copy_(xb)
            used.replay(gid)
            torch.cuda.synchronize()
        else:
            run(used, xa, False)
            outs = run(used, xb.clone(), False)
        same(snapshot(used, outs, names), want, "forward(B) after forward(A) against a fresh net's forward(B) (%s)" % kind)
    if kind == "fp16_output_u8":
        assert used.writes_u8_natively() and all(o.dtype == torch.uint8 for o in outs)
    if kind == "fp16_output_f16":
        assert all(o.dtype == torch.float16 for o in outs)


# ---- outputs and inputs stay inside their tensors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_outputs_stay_inside_their_slab_and_inputs_are_not_over_read(dtype):
    net = make_net(CFG, dtype)
    x = synthetic_input(B, CFG).to(DEV)
    n = CFG.image_size
    want = [o.clone() for o in net(x)]
    slab = guarded_empty((7 * B * n * n,), torch.float32, DEV, "ff", name="output slab")
    outs = net(x, out=slab)
    torch.cuda.synchronize()
    check_bands(slab)
    assert bool(torch.isfinite(slab).all()), "an element of the output slab was never written"
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    # the input in a guarded tensor whose bands are NaN: fp32 NCHW, and uint8 HWC (bands of 255)
    gx = guarded_copy(x, name="input fp32 NCHW")
    outs = net(gx)
    torch.cuda.synchronize()
    check_bands(gx)
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    img = torch.randint(0, 256, (B, n, n, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    want8 = [o.clone() for o in net(img)]
    g8 = guarded_copy(img, name="input uint8 HWC")
    slab.fill_(float("nan"))
    outs = net(g8, out=slab)
    torch.cuda.synchronize()
    check_bands(g8, slab)
    assert bool(torch.isfinite(slab).all())
    for a, b in zip(outs, want8):
        assert torch.equal(a, b)


# ---- tile and ensemble arenas ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_ensemble", [False, True], ids=["plain", "self_ensemble"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_tile_arena_contents_do_not_matter(dtype, self_ensemble):
    """forward_tiled of a 70 x 45 uint8 image (tile_batch 4) through an arena prefilled with 0xff bytes and one prefilled with zeros: bitwise equal, float
    and uint8 outputs, nothing written outside the arena"""
    net = make_net(CFG, dtype)
    net(synthetic_input(B, CFG).to(DEV))
    H, W, T = 70, 45, CFG.image_size
    img = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(DEV)
    ys, xs = tiled.tile_grid(H, W, T, tiled.default_overlap(T))
    ntiles = len(ys) * len(xs)
    Bt = min(4, ntiles)
    numel = -(-ntiles // Bt) * 7 * Bt * T * T
    res = {}
    for fill in ("ff", "zero"):
        arena = guarded_empty((numel,), torch.float32, DEV, fill, name="tile arena (%s)" % fill)
        res[fill] = [t.clone() for u8 in (False, True)
                     for t in net.forward_tiled(img, tile_batch=4, output_u8=u8, self_ensemble=self_ensemble, arena=arena)]
        torch.cuda.synchronize()
        check_bands(arena)
        assert bool(torch.isfinite(arena).all()), "an element of the arena was never written"
    for a, b in zip(res["ff"], res["zero"]):
        assert torch.equal(a, b)
    plain = net.forward_tiled(img, tile_batch=4, self_ensemble=self_ensemble)
    for a, b in zip(res["ff"][:3], plain):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="arena"):
        net.forward_tiled(img, tile_batch=4, arena=torch.empty(numel - 1, device=DEV))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_ensemble_arena_contents_do_not_matter(dtype):
    """forward_x8 of one uint8 image (eight forwards into the arena, one merge out of it) through an arena prefilled with 0xff bytes and one prefilled
    with zeros: bitwise equal, float and uint8 outputs, and equal to the call that allocates its own arena; nothing written outside the arena, every
    element of it written"""
    net = make_net(CFG, dtype)
    net(synthetic_input(B, CFG).to(DEV))                   # (initialises the ActNorm layers: forward_x8 refuses a net that has not run)
    T = CFG.image_size
    img = torch.randint(0, 256, (1, T, T, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).to(DEV)
    numel = 56 * T * T
    res = {}
    for fill in ("ff", "zero"):
        arena = guarded_empty((numel,), torch.float32, DEV, fill, name="ensemble arena (%s)" % fill)
        res[fill] = [t.clone() for u8 in (False, True) for t in net.forward_x8(img, output_u8=u8, arena=arena)]
        torch.cuda.synchronize()
        check_bands(arena)
        assert bool(torch.isfinite(arena).all()), "an element of the arena was never written"
    for a, b in zip(res["ff"], res["zero"]):
        assert torch.equal(a, b)
    for a, b in zip(res["ff"][:3], net.forward_x8(img)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="arena"):
        net.forward_x8(img, arena=torch.empty(numel - 1, device=DEV))
