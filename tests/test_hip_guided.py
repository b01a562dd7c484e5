"""Guided upsampling on the device (cfen_guided_coef_u8, cfen_guided_apply_u8; ops.guided_coef_u8, ops.guided_apply_u8, ops.guided_upsample_u8),
fit-to-size inference with refine="guided" on top of it (dec_ipt.forward_fit, test.py --fit --fit_refine guided), and the second half of the
ledger of include/cfen_guided.h.  The reference is the float64 restatement tests/guided_ref.py; the tolerance TAU (levels) is measured on the CPU in
tests/test_guided_host.py, never against the kernels; the composition tests have no tolerance."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from cfen_vit_dehazing_amd import _lib, ops
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import cabi_ledger
import guarded
import guided_ref as ref
import test_hip_resample as fitref                      # TINY (T = 128), make_net, net_input, plain_u8, _run_cli
from test_guided_host import TAU

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = fitref.T


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared reference arrays are read-only


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", ref.EPS)
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("name", list(ref.COEF_CASES))
def test_coefficients_against_float64(name, kind, eps):
    B, h, w, r = ref.COEF_CASES[name]
    I, P, a64, b64 = ref.coef_case(name, kind, eps)
    coef = ops.guided_coef_u8(dev(I), dev(P), r, eps)
    assert coef.shape == (B, h, w, 6) and coef.dtype == torch.float32
    c = coef.cpu().numpy().astype(np.float64)
    err = np.abs(c[..., :3] - a64) * 255 + np.abs(c[..., 3:] - b64)
    print("%s %s eps %g: max |da| 255 + |db| = %.3e (TAU %.3e)" % (name, kind, eps, err.max(), TAU))
    assert np.isfinite(c).all() and err.max() <= TAU


# ---- apply and the composed call ----------------------------------------------------------------------------------------------------------------
def assert_bytes(got, v64, what):
    """a byte may differ from the reference's, by exactly 1, only where the reference's v lies within TAU of k + 0.5"""
    want = ref.to_bytes(v64)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = got.astype(np.int64) - want
    dist = np.abs((v64 - 0.5) - np.round(v64 - 0.5))             # distance of v to the nearest k + 0.5
    print("%s: %d of %d bytes differ, %d lie within TAU of a rounding boundary" % (what, (diff != 0).sum(), diff.size, (dist <= TAU).sum()))
    assert np.abs(diff).max() <= 1, what
    assert (dist[diff != 0] <= TAU).all(), (what, float(dist[diff != 0].max()))


def test_paths_the_cases_claim():
    """row pitches and pointer alignment that send a case to the 16-byte or the byte path, and the coefficient-column counts that send a workgroup
    to the staged (<= 1024 columns) or the global-memory path"""
    pitch = {n: 3 * c[1][1] for n, c in ref.APPLY_CASES.items()}
    vec = sorted(n for n, p in pitch.items() if p % 16 == 0)
    assert vec == ["20x24_30x400", "33x40_16x16", "4x1500_2x1376", "4x30_2x1376"] and pitch["5x7_37x53"] == 159 and pitch["20x24_30x400"] == 1200
    assert sorted(n for n, p in pitch.items() if p > 4096) == ["40x30_3x1400", "4x1500_2x1376", "4x30_2x1376", "6x2100_3x1400"]

    def columns(w, W, first, last):
        x0, x1, _ = ref.axis_coords(w, W)
        return int(x1[min(last, W - 1)] - x0[first] + 1)
    assert columns(2100, 1400, 0, 1365) > 1024 and columns(1500, 1376, 0, 1365) > 1024 and columns(2100, 1400, 1365, 1399) <= 1024
    assert columns(30, 1400, 0, 1365) <= 1024 and columns(512, 3840, 0, 1365) == 183
    G, _, _, v = ref.apply_case("12x14_20x31_binary")
    assert set(np.unique(G)) == {0, 255} and v.min() < -100 and v.max() > 355              # the clamp works on both sides


@pytest.mark.parametrize("name", list(ref.APPLY_CASES))
def test_guided_upsample_against_float64(name):
    (h, w), (H, W), r, kind = ref.APPLY_CASES[name]
    G, I, P, v64 = ref.apply_case(name)
    tG, tI, tP = dev(G), dev(I), dev(P)
    got = ops.guided_upsample_u8(tG, tI, tP, r, 1e-4)
    assert got.shape == (1, H, W, 3) and got.dtype == torch.uint8
    assert_bytes(got.cpu().numpy(), v64, name)
    two = ops.guided_apply_u8(ops.guided_coef_u8(tI, tP, r, 1e-4), tG)                       # the composed call is the two halves
    assert torch.equal(two, got)


@pytest.mark.parametrize("c", [0, 1, 128, 255])
def test_constant_output_is_exact(c):
    G = dev(ref.hires("random", 2, 37, 53, c))
    I = dev(ref.lowres("random", 2, 17, 20, c)[0])
    P = torch.full((2, 17, 20, 3), c, dtype=torch.uint8, device=DEV)
    for r, eps in ((1, 1e-4), (2, 1e-4), (16, 1e-2)):
        coef = ops.guided_coef_u8(I, P, r, eps)
        assert bool((coef[..., :3] == 0).all()) and bool((coef[..., 3:] == c).all())
        assert bool((ops.guided_apply_u8(coef, G) == c).all())


def test_constant_guide_gives_zero_slope():
    P = dev(ref.lowres("random", 1, 17, 20, 3)[1])
    for g in (0, 7, 255):
        coef = ops.guided_coef_u8(torch.full((1, 17, 20, 3), g, dtype=torch.uint8, device=DEV), P, 2, 1e-4)
        assert bool((coef[..., :3] == 0).all()) and bool(torch.isfinite(coef).all())


def test_python_argument_errors():
    G, (I, P) = dev(ref.hires("random", 1, 9, 9, 0)), (dev(x) for x in ref.lowres("random", 1, 4, 4, 0))
    with pytest.raises(ValueError, match="guided_coef_u8 needs"):
        ops.guided_coef_u8(I.float(), P)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.guided_coef_u8(I, P[:, :3].contiguous())
    for bad in ({"radius": 0}, {"radius": 17}, {"eps": 0.0}, {"eps": float("nan")}, {"eps": float("inf")}):
        with pytest.raises(ValueError, match="guided_coef_u8: (radius|eps)"):
            ops.guided_coef_u8(I, P, **bad)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.guided_coef_u8(I, I)
    coef = ops.guided_coef_u8(I, P)
    with pytest.raises(ValueError, match="guided_apply_u8 needs coef"):
        ops.guided_apply_u8(coef[..., :3].contiguous(), G)
    with pytest.raises(ValueError, match="guided_apply_u8: out must be"):
        ops.guided_apply_u8(coef, G, out=torch.empty(1, 9, 9, 3, device=DEV))
    with pytest.raises(ValueError, match="differ in batch"):
        ops.guided_upsample_u8(torch.cat([G, G]), I, P)


# ---- determinism ------------------------------------------------------------------------------------------------------------------------------------
def _raw(tG, tI, tP, r, eps, tmp, coef, dst, stream=None):
    """the two C entry points with caller-placed tmp, coef and dst"""
    B, h, w, _ = tI.shape
    H, W = tG.shape[1:3]
    lib = _lib.load()
    s = stream if stream is not None else _lib.current_stream()
    _lib.check(lib.cfen_guided_coef_u8(_lib.ptr(tI), _lib.ptr(tP), B, h, w, r, eps * 255.0 * 255.0, _lib.ptr(tmp), _lib.ptr(coef), s), "guided_coef_u8")
    _lib.check(lib.cfen_guided_apply_u8(_lib.ptr(coef), B, h, w, _lib.ptr(tG), H, W, _lib.ptr(dst), s), "guided_apply_u8")


def test_determinism():
    B, h, w, H, W, r = 3, 17, 70, 37, 53, 2                                # rows of 159 bytes, images of 5883: lane 1 of dst at an odd address
    I, P = ref.lowres("model", B, h, w, 77)
    tG, tI, tP = dev(ref.hires("random", B, H, W, 77)), dev(I), dev(P)
    whole = ops.guided_upsample_u8(tG, tI, tP, r)
    coefs = ops.guided_coef_u8(tI, tP, r)
    for b in range(B):                                                     # B = 3 equals three B = 1 calls
        assert torch.equal(ops.guided_upsample_u8(tG[b:b + 1], tI[b:b + 1], tP[b:b + 1], r), whole[b:b + 1])
        assert torch.equal(ops.guided_coef_u8(tI[b:b + 1], tP[b:b + 1], r), coefs[b:b + 1])
    for _ in range(3):                                                     # repeated calls
        assert torch.equal(ops.guided_upsample_u8(tG, tI, tP, r), whole)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.guided_upsample_u8(tG, tI, tP, r)
    side.synchronize()
    assert torch.equal(on_side, whole)
    for fill in (0x00, 0xff):                                              # what tmp, coef and dst held before does not matter
        tmp = torch.full((B * h * w * 24,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(B, h, w, 6)
        coef = torch.full((B * h * w * 24,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(B, h, w, 6)
        dst = torch.full((B, H, W, 3), fill, dtype=torch.uint8, device=DEV)
        _raw(tG, tI, tP, r, 1e-4, tmp, coef, dst)
        assert torch.equal(dst, whole) and torch.equal(coef, coefs)
        a, b = ref.coefficients(I[1], P[1], r, 1e-4)                       # tmp holds the unsmoothed a, b
        t = tmp[1].cpu().numpy().astype(np.float64)
        assert (np.abs(t[..., :3] - a) * 255 + np.abs(t[..., 3:] - b)).max() <= TAU


@pytest.mark.parametrize("size", [(37, 53), (16, 16)])
def test_dst_as_a_lane_of_a_slab(size):
    """out = lane 1 of a (3, H, W, 3) slab: at 37 x 53 the lane starts at an odd address (the byte path), at 16 x 16 on a 16-byte boundary (the
    vector path); the neighbouring lanes keep their bytes"""
    I, P = ref.lowres("model", 1, 33, 40, 5)
    G = ref.hires("random", 1, size[0], size[1], 5)
    slab = dev(np.random.RandomState(6).randint(0, 256, (3,) + size + (3,), dtype=np.uint8))
    before = slab.clone()
    out = ops.guided_upsample_u8(dev(G), dev(I), dev(P), out=slab[1:2])
    assert out.data_ptr() == slab[1].data_ptr() and (out.data_ptr() % 2 == 1) == (size == (37, 53)) and (out.data_ptr() % 16 == 0) == (size == (16, 16))
    assert_bytes(slab[1:2].cpu().numpy(), ref.guided_v(G[0], I[0], P[0], 2, 1e-4)[None], "lane 1 of the slab")
    assert torch.equal(slab[1:2], ops.guided_upsample_u8(dev(G), dev(I), dev(P)))
    assert torch.equal(slab[0], before[0]) and torch.equal(slab[2], before[2])


# ---- guard bands and the header's ledger ------------------------------------------------------------------------------------------------------------
def test_guard_bands_guided():
    """every input between 0xff bands, tmp, coef and dst prefilled 0xff between random bands, for both entry points: no band changes, the results
    are the unguarded call's, and a zero prefill gives the same"""
    lib = _lib.load()
    B, h, w, r = 2, 33, 40, 4
    I, P = ref.lowres("model", B, h, w, 21)
    tI, tP = guarded.guarded_copy(dev(I)), guarded.guarded_copy(dev(P))
    tmp = guarded.guarded_empty((B, h, w, 6), torch.float32, DEV, fill="ff")
    coef = guarded.guarded_empty((B, h, w, 6), torch.float32, DEV, fill="ff")
    want_coef = ops.guided_coef_u8(dev(I), dev(P), r)
    for H, W in ((37, 53), (20, 1376)):                                    # byte path; vector path with two workgroups per row
        G = ref.hires("random", B, H, W, 22)
        tG = guarded.guarded_copy(dev(G))
        dst = guarded.guarded_empty((B, H, W, 3), torch.uint8, DEV, fill="ff")
        want = ops.guided_upsample_u8(dev(G), dev(I), dev(P), r)
        for fill in ("ff", "zero"):
            for t in (tmp, coef, dst):
                guarded.refill(t, fill)
            _lib.check(lib.cfen_guided_coef_u8(_lib.ptr(tI), _lib.ptr(tP), B, h, w, r, 1e-4 * 255.0 * 255.0, _lib.ptr(tmp), _lib.ptr(coef),
                                               _lib.current_stream()), "guided_coef_u8")
            _lib.check(lib.cfen_guided_apply_u8(_lib.ptr(coef), B, h, w, _lib.ptr(tG), H, W, _lib.ptr(dst), _lib.current_stream()), "guided_apply_u8")
            torch.cuda.synchronize()
            guarded.check_bands(tI, tP, tmp, coef, tG, dst)
            assert bool(torch.isfinite(tmp).all()) and torch.equal(coef, want_coef) and torch.equal(dst, want), (H, W, fill)
        assert_bytes(dst.cpu().numpy(), np.stack([ref.guided_v(G[b], I[b], P[b], r, 1e-4) for b in range(B)]), "guarded %d x %d" % (H, W))


def test_every_function_of_the_guided_header_is_guard_band_tested():
    """what tests/test_cabi.py checks for include/cfen_hip.h, for include/cfen_guided.h: every function it declares is called through lib. inside
    the guard-band test above"""
    fns = cabi_ledger.header_functions("cfen_guided.h")
    assert sorted(fns) == sorted(_lib.HEADERS["cfen_guided.h"])
    cabi_ledger.check_guard_band_test_calls("test_hip_guided.py", "test_guard_bands_guided", fns)


# ---- forward_fit(refine="guided") ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8_input", [True, False], ids=["u8_input", "float_input"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_forward_fit_guided(dtype, u8_input):
    net = fitref.make_net(dtype)
    big, tbig = fitref.images(2, 200, 300, 41)
    mid, tmid = fitref.images(1, 90, 128, 42)
    same, tsame = fitref.images(1, T, T, 43)
    # (2, 200, 300, 3): resample -> plain forward with uint8 outputs -> xr, xs resampled, xd guided, by hand
    small = ops.resample_u8(tbig, (T, T))
    lo = [dev(o) for o in fitref.plain_u8(net, fitref.net_input(small.cpu().numpy(), u8_input))]
    plain = net.forward_fit(tbig, u8_input=u8_input)
    got = net.forward_fit(tbig, u8_input=u8_input, refine="guided")
    assert all(g.shape == (2, 200, 300, 3) and g.dtype == torch.uint8 for g in got)
    assert torch.equal(got[2], ops.guided_upsample_u8(tbig, small, lo[2])) and not torch.equal(got[2], plain[2])
    assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])                   # xr and xs keep the plain resample
    assert torch.equal(got[0], ops.resample_u8(lo[0], (200, 300))) and torch.equal(got[1], ops.resample_u8(lo[1], (200, 300)))
    # radius and eps reach the kernels
    got = net.forward_fit(tbig, u8_input=u8_input, refine="guided", radius=5, eps=1e-2)
    assert torch.equal(got[2], ops.guided_upsample_u8(tbig, small, lo[2], 5, 1e-2))
    # refine=None is the call without the argument, which is resample_u8 of the three outputs
    none = net.forward_fit(tbig, u8_input=u8_input, refine=None)
    assert all(torch.equal(a, b) and torch.equal(a, ops.resample_u8(o, (200, 300))) for a, b, o in zip(none, plain, lo))
    # the list form: one batch-3 forward; the T x T image is the plain forward bitwise
    x = torch.cat([small[:1], ops.resample_u8(tmid, (T, T)), tsame])
    lo = [dev(o) for o in fitref.plain_u8(net, fitref.net_input(x.cpu().numpy(), u8_input))]
    imgs = [tbig[0], tmid[0], tsame[0]]
    plain = net.forward_fit(imgs, u8_input=u8_input)
    got = net.forward_fit(imgs, u8_input=u8_input, refine="guided")
    assert len(got) == 3 and all(len(g) == 3 for g in got)
    for i, t in enumerate(imgs[:2]):
        assert got[2][i].shape == t.shape and torch.equal(got[2][i], ops.guided_upsample_u8(t[None], x[i:i + 1], lo[2][i:i + 1])[0]), i
    assert torch.equal(got[2][2], lo[2][2])
    for k in (0, 1):
        assert all(torch.equal(a, b) for a, b in zip(got[k], plain[k]))
    # self-ensemble composes: forward_x8 of the resampled image, xd guided
    lo = [dev(o) for o in fitref.plain_u8(net, fitref.net_input(small[:1].cpu().numpy(), u8_input), x8=True)]
    got = net.forward_fit(tbig[:1], self_ensemble=True, u8_input=u8_input, refine="guided")
    assert torch.equal(got[2], ops.guided_upsample_u8(tbig[:1], small[:1], lo[2])) and torch.equal(got[0], ops.resample_u8(lo[0], (200, 300)))
    with pytest.raises(ValueError, match="forward_fit: refine"):
        net.forward_fit(tbig, refine="bilateral")
    with pytest.raises(ValueError, match="forward_fit: radius"):
        net.forward_fit(tbig, refine="guided", radius=17)
    assert net.output_u8 is False


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_fit_refine_guided(tmp_path):
    """test.py --fit --fit_refine guided in a fresh child process writes the PNGs of the library path, with --eval rows; a second child process with
    an explicit --fit_refine none writes the bytes of --fit alone, which are the library path without refine (that test.py --fit with the flag ABSENT
    writes those is tests/test_hip_resample.py::test_cli_fit_writes_input_sized_pngs, unchanged)."""
    name = "iid_hlgvit_crs_gd4_cfs_v3_fit"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(fitref.TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    rs = np.random.RandomState(0)
    imgs = {"big": rs.randint(0, 256, (200, 300, 3), dtype=np.uint8), "small": rs.randint(0, 256, (T, T, 3), dtype=np.uint8)}
    os.makedirs(tmp_path / "data" / "hazy")
    os.makedirs(tmp_path / "data" / "clear")
    for stem, a in imgs.items():
        Image.fromarray(a).save(tmp_path / "data" / "hazy" / (stem + ".png"))
        Image.fromarray(rs.randint(0, 256, a.shape, dtype=np.uint8)).save(tmp_path / "data" / "clear" / (stem + ".png"))
    net = fitref.make_net("fp32")                                          # --precision single is the default
    res = tmp_path / "res_data" / name / "test_32"
    written = {}
    for flag, refine in (("guided", "guided"), ("none", None)):
        r = fitref._run_cli(tmp_path, tmp_path / "data", name, ["--out_all", "--fit", "--fit_refine", flag, "--eval"])
        assert r.returncode == 0, r.stdout[-3000:]
        assert ("fit_refine: guided" in r.stdout and "fit_radius: 2" in r.stdout) if refine else "fit_refine:" not in r.stdout
        assert sorted(os.listdir(res / "images")) == ["big_fake_A.png", "small_fake_A.png"]
        for stem, a in imgs.items():
            got = np.asarray(Image.open(res / "images" / (stem + "_fake_A.png"))).copy()
            want = net.forward_fit(dev(a)[None], u8_input=False, refine=refine)[2][0].cpu().numpy()
            assert got.shape == a.shape and np.array_equal(got, want), (stem, flag)
            written[stem, flag] = got
        lines = open(res / "metrics.csv").read().splitlines()
        assert lines[0] == "image,psnr,ssim" and [l.split(",")[0] for l in lines[1:]] == ["big.png", "small.png"]
    assert not np.array_equal(written["big", "guided"], written["big", "none"]) and np.array_equal(written["small", "guided"], written["small", "none"])
