"""Python handles on the individual HIP operators of libcfen_hip.so (tensors in, tensors out).

Used by the parity tests and by anyone who wants one fused block instead of the whole generator.
Every function launches on torch's current CUDA(=HIP) stream and raises CfenError on failure; there
is no PyTorch fallback.
"""
import contextlib
import ctypes
import functools
import math

import torch

from . import _lib
from ._lib import ptr, check, dtype_code, current_stream, ConvArgsC, MlpArgsC
from .packing import round_up


def _cuda(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise ValueError("HIP operators need contiguous CUDA tensors")


def _out(out, shape, dtype, device, what, zero=False):
    """the operator's output: `out` if the caller places it (ValueError unless it is a contiguous `dtype` tensor of `shape` on `device`), else a
    fresh tensor as before (`zero`: the wrappers that have always handed their kernel a zeroed one)"""
    shape = tuple(int(s) for s in shape)
    if out is None:
        return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s tensor of shape %s on %s" % (what, dtype, shape, device))
    return out


def _tensor_arg(what, name, t, shape, dtype, like=None):
    """argument `name` of operator `what`: ValueError unless `t` is a contiguous CUDA tensor of `dtype` whose sizes are `shape` (None: any size >= 1,
    written B, H, W in the message), on the device of the tensor `like` if one is given"""
    if not isinstance(t, torch.Tensor) or t.dim() != len(shape) or t.dtype != dtype or (like is not None and t.device != like.device) or \
            any(n < 1 if s is None else n != s for n, s in zip(t.shape, shape)):
        free = iter("BHW"[3 - sum(s is None for s in shape):])        # the free sizes in order: (B,H,W,3), (H,W,3), (B,3,H,W)
        want = ",".join(next(free) if s is None else str(s) for s in shape)
        raise ValueError("%s needs %s as a contiguous (%s) %s tensor%s, got %s" % (
            what, name, want, str(dtype)[len("torch."):], "" if like is None else " on %s" % like.device,
            "%s %s on %s" % (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__))
    _cuda(t)


def _rgb_batch(what, **images):
    """each of `images` (name=tensor) is a contiguous (B,H,W,3) uint8 CUDA tensor"""
    for name, t in images.items():
        _tensor_arg(what, name, t, (None, None, None, 3), torch.uint8)


def _rgb_pair(what, **images):
    """the two images of a comparison: _rgb_batch, and of one shape on one device"""
    _rgb_batch(what, **images)
    (na, a), (nb, b) = images.items()
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("%s: %s %s and %s %s differ in shape or device" % (what, na, tuple(a.shape), nb, tuple(b.shape)))


def _int_arg(what, name, v, lo, hi, choices=None):
    """`v` (a Python or numpy scalar, a 0-d tensor) as an int, if it is a whole number in lo .. hi -- or one of `choices`, if given"""
    try:
        i = int(v)
    except (TypeError, ValueError, OverflowError):
        i = None
    if i is None or i != v or not (lo <= i <= hi if choices is None else i in choices):
        rule = "an integer in %d .. %d" % (lo, hi) if choices is None else "%s or %d" % (", ".join(str(c) for c in choices[:-1]), choices[-1])
        raise ValueError("%s: %s must be %s, got %r" % (what, name, rule, v))
    return i


def _float_arg(what, name, v, test, rule):
    """`v` as a float, if test(float(v)) holds; `rule` says in the message what `test` asks for"""
    try:
        f = float(v)
    except (TypeError, ValueError, OverflowError):
        f = None
    if f is None or not test(f):
        raise ValueError("%s: %s must be %s, got %r" % (what, name, rule, v))
    return f


def _scratch_for(what, bytes_fn, dims, device, limits=None):
    """a kernel's scratch of doubles, of the size the library's bytes_fn(*dims) asks for (it goes back to torch's allocator on the stream it was used
    on).  The library answers 0 for sizes its entry point refuses: ValueError with `limits`, or without it left to the entry point's own message"""
    nbytes = bytes_fn(*dims)
    if nbytes == 0 and limits is not None:
        raise ValueError("%s: sizes %s are outside the limits (%s)" % (what, tuple(dims), limits))
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def tune(key, value):
    """process-wide kernel-variant knob (cfen_tune; the table of knobs is csrc/cfen_tune_knobs.hpp); for benchmarks"""
    check(_lib.load().cfen_tune(key.encode(), int(value)), "tune")


def _tune_query(key):
    value, shipped = ctypes.c_int(), ctypes.c_int()
    check(_lib.load().cfen_tune_query(key.encode(), ctypes.byref(value), ctypes.byref(shipped)), "tune_query")
    return value.value, shipped.value


def tuned(key):
    """the value of a knob now, read from the library (so a knob set through the C ABI directly is seen too)"""
    return _tune_query(key)[0]


def tune_keys():
    """every knob's key, in the order of the library's table"""
    lib = _lib.load()
    keys = []
    while True:
        k = lib.cfen_tune_key(len(keys))
        if k is None:
            return keys
        keys.append(k.decode())


def tune_not_shipped():
    """{key: (value, shipped default)} of the knobs that are not at their shipped default"""
    return {k: vs for k, vs in ((k, _tune_query(k)) for k in tune_keys()) if vs[0] != vs[1]}


@contextlib.contextmanager
def tuning(knobs):
    """with ops.tuning({key: value, ...}): sets the knobs in order, and puts the values they had back in reverse order on the way out
    (also when the body raises, and for the knobs already set when a later one is refused)"""
    undo = []
    try:
        for key, value in knobs.items():
            before = tuned(key)
            tune(key, value)
            undo.append((key, before))
        yield
    finally:
        for key, before in reversed(undo):
            tune(key, before)


def gemm_nt(x, w, bias=None, residual=None, pos=None, relu=False, out=None):
    """act(x @ w.T + bias) + residual + pos[row % len(pos)]   (x: [M,K], w: [N,K])"""
    _cuda(x, w, bias, residual, pos, out)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=x.dtype, device=x.device)
    lib = _lib.load()
    check(lib.cfen_gemm_nt(dtype_code(x.dtype), ptr(x), K, ptr(w), K, ptr(bias), ptr(residual), N, ptr(pos),
                           pos.shape[0] if pos is not None else 0, ptr(out), N, M, N, K, int(relu), current_stream()), "gemm_nt")
    return out


def gemm_ln(x, wl, s, bias=None, relu=False, eps=1e-5, out=None):
    """act(LayerNorm-statistics(x) applied to x @ wl.T: rstd (x wl^T - mean s) + bias); wl / s / bias from packing.ln_folded"""
    _cuda(x, wl, s, bias)
    M, K = x.shape
    N = wl.shape[0]
    out = _out(out, (M, N), x.dtype, x.device, "gemm_ln")
    check(_lib.load().cfen_gemm_ln(dtype_code(x.dtype), ptr(x), K, ptr(wl), K, ptr(s), ptr(bias), ptr(out), N, M, N, K, int(relu), eps,
                                   current_stream()), "gemm_ln")
    return out


def gemm_splitk(x, w, nsplit, bias=None, residual=None, relu=False, lnf_s=None, scratch=None, out=None):
    """cfen_gemm_splitk: act(x @ w.T + bias) + residual (or the LayerNorm-folded form when lnf_s is given) with K cut into nsplit slices and
    the in-launch reduction; `scratch` (zeroed uint8 buffer) can be passed to check that calls leave its counters zero"""
    _cuda(x, w, bias, residual, lnf_s, scratch)
    M, K = x.shape
    N = w.shape[0]
    out = _out(out, (M, N), x.dtype, x.device, "gemm_splitk")
    tiles = ((N + 95) // 96) * ((M + 31) // 32)
    if scratch is None:
        scratch = torch.zeros(4096 + tiles * nsplit * 14336, dtype=torch.uint8, device=x.device)
    check(_lib.load().cfen_gemm_splitk(dtype_code(x.dtype), ptr(x), K, ptr(w), K, ptr(lnf_s), ptr(bias), ptr(residual), N, ptr(out), N, M, N, K,
                                       int(relu), nsplit, ptr(scratch), scratch.numel(), current_stream()), "gemm_splitk")
    return out


def head_conv5(x, w, bias, act=0, out=None):
    """cfen_head_conv5: conv5x5 (pad 2) of the network input -- (B,3,H,W) fp32 NCHW or (B,H,W,3) uint8 -- to a (B,H,W,16) fp16 NHWC map;
    w: (Cout <= 16, 3, 5, 5), bias: (Cout,)"""
    from .packing import pack_head5
    _cuda(x, w, bias)
    u8 = x.dtype == torch.uint8
    B, H, W = (x.shape[0], x.shape[1], x.shape[2]) if u8 else (x.shape[0], x.shape[2], x.shape[3])
    w5 = pack_head5(w, torch.float16)
    scale = torch.ones(16, dtype=torch.float32, device=x.device)
    shift = torch.zeros(16, dtype=torch.float32, device=x.device)
    shift[:bias.numel()] = bias.float()
    out = _out(out, (B, H, W, 16), torch.float16, x.device, "head_conv5")
    check(_lib.load().cfen_head_conv5(1, int(u8), ptr(x), ptr(w5), ptr(scale), ptr(shift), ptr(out), B, H, W, 16, act, current_stream()), "head_conv5")
    return out


def gemm_chain(phases, M, team=48, fold=None, sync=None):
    """cfen_gemm_chain: a list of dependent GEMM phases in one persistent launch.  Every phase is a dict with x [M,K], w [N,K] (row-major; packed
    to a fragment stream here) or w_stream, y (preallocated output, [M,N] or the NHWC map when fold), and optionally bias, lnf_s, residual, pos,
    relu, nsplit, fold.  fold = (H, W, cs, C, p) of the map.  Returns the error word (0 = fine)."""
    from .packing import pack_stream_tiles
    from ._lib import ChainArgsC
    a = ChainArgsC()
    keep = []
    a.nphases, a.M = len(phases), M
    maxslab = 0
    for i, ph in enumerate(phases):
        x, y = ph["x"], ph["y"]
        ws = ph.get("w_stream")
        if ws is None:
            ws = pack_stream_tiles(ph["w"].contiguous())
        keep.append(ws)
        N, K = (ph["w"].shape if "w" in ph else (ph["N"], ph["K"]))
        _cuda(x, ws, y, ph.get("bias"), ph.get("lnf_s"), ph.get("residual"), ph.get("pos"))
        q = a.phase[i]
        q.x, q.w_stream, q.bias, q.lnf_s, q.residual, q.pos, q.y = (ptr(x).value, ptr(ws).value, ptr(ph.get("bias")).value, ptr(ph.get("lnf_s")).value,
                                                                  ptr(ph.get("residual")).value, ptr(ph.get("pos")).value, ptr(y).value)
        q.ldx, q.ldr, q.ldy = x.shape[1], N, N
        q.period = ph["pos"].shape[0] if ph.get("pos") is not None else 0
        q.N, q.K, q.relu, q.nsplit, q.fold = N, K, int(ph.get("relu", False)), int(ph.get("nsplit", 1)), int(ph.get("fold", False))
        maxslab = max(maxslab, (N // 128) * q.nsplit)
    if fold is not None:
        a.fold_H, a.fold_W, a.fold_cs, a.fold_C, a.fold_p = fold
    own = sync is None
    if own:
        sync = torch.zeros(8192 + ((M + 127) // 128) * maxslab * 65536, dtype=torch.uint8, device=phases[0]["x"].device)
    a.sync_ws, a.sync_ws_bytes = ptr(sync).value, sync.numel()
    check(_lib.load().cfen_gemm_chain(dtype_code(phases[0]["x"].dtype), ctypes.byref(a), team, current_stream()), "gemm_chain")
    return int(sync[:8].view(torch.int32)[1].item()) if own else None     # with a caller-owned `sync` buffer: no read-back (word 1 of it = error)


def layernorm(x, gamma, beta, eps=1e-5, out=None, padded=None):
    """LayerNorm over the rows of x (M, D).  padded = (cs, C): cfen_layernorm_padded of include/cfen_padnorm.h -- a row is D / cs pixels of cs
    slots of which the first C are real; statistics over the real slots, the others come out as beta"""
    _cuda(x, gamma, beta)
    out = _out(out, x.shape, x.dtype, x.device, "layernorm")
    if padded is not None:
        cs, C = padded
        check(_lib.load().cfen_layernorm_padded(dtype_code(x.dtype), ptr(x), ptr(out), ptr(gamma), ptr(beta), x.shape[0], x.shape[1], int(cs), int(C),
                                                eps, current_stream()), "layernorm_padded")
        return out
    check(_lib.load().cfen_layernorm(dtype_code(x.dtype), ptr(x), ptr(out), ptr(gamma), ptr(beta), x.shape[0], x.shape[1], eps,
                                     current_stream()), "layernorm")
    return out


def attention(qkv, nseq, S, heads, out=None):
    """qkv: [nseq*S, 3*D] -> [nseq*S, D]"""
    _cuda(qkv)
    D = qkv.shape[1] // 3
    out = _out(out, (qkv.shape[0], D), qkv.dtype, qkv.device, "attention")
    check(_lib.load().cfen_attention(dtype_code(qkv.dtype), ptr(qkv), ptr(out), nseq, S, heads, D // heads, current_stream()), "attention")
    return out


def attention_head_major(qkv, nseq, S, heads, out=None):
    """qkv in the head-major layout of embed_qkv(head_major_heads=heads) -> [nseq*S, D] row-major"""
    _cuda(qkv)
    D = qkv.numel() // (3 * nseq * S)
    out = _out(out, (nseq * S, D), qkv.dtype, qkv.device, "attention_head_major")
    check(_lib.load().cfen_attention_head_major(dtype_code(qkv.dtype), ptr(qkv), ptr(out), nseq, S, heads, D // heads, current_stream()),
          "attention_head_major")
    return out


def mlp_block(x, w1a, b1a, w2a, b2a, ln=None, second=None, fold=None, proj=None, out=None):
    """Fused y1 = x + W2a relu(W1a LN(x)+b1a) + b2a [; y2 = y1 + W2b relu(W1b y1 + b1b) + b2b].
    Weights must already carry packing.kperm32 on their k axis for fp16.  fold = (B, H, W, C, cs, ws, p) writes
    the result into a fresh NHWC map instead of a token matrix.  proj = (att, w_proj): x is first replaced by x + att @ w_proj.T."""
    _cuda(x, w1a, b1a, w2a, b2a)
    M, D = x.shape
    a = MlpArgsC(x=x.data_ptr(), w1a=w1a.data_ptr(), b1a=b1a.data_ptr(), w2a=w2a.data_ptr(), b2a=b2a.data_ptr(), M=M, D=D,
                 H=w1a.shape[0], eps=1e-5)
    if proj is not None:
        _cuda(*proj)
        a.att, a.w_proj = proj[0].data_ptr(), proj[1].data_ptr()
    if ln is not None:
        _cuda(*ln)
        a.ln_gamma, a.ln_beta = ln[0].data_ptr(), ln[1].data_ptr()
    if second is not None:
        _cuda(*second)
        a.w1b, a.b1b, a.w2b, a.b2b = (t.data_ptr() for t in second)
    if fold is None:
        out = _out(out, x.shape, x.dtype, x.device, "mlp_block")
        a.y = out.data_ptr()
    else:
        B, H, W, C, cs, ws, p = fold
        out = _out(out, (B, H, W, cs), x.dtype, x.device, "mlp_block(fold=)", zero=True)
        a.fmap, a.mapH, a.mapW, a.C, a.cs, a.ws, a.p = out.data_ptr(), H, W, C, cs, ws, p
    check(_lib.load().cfen_mlp_block(dtype_code(x.dtype), ctypes.byref(a), current_stream()), "mlp_block")
    return out


def mlp_stream_block(x, wa, b1a, b2a, hidden, ln=None, second=None, fold=None, proj=None, out=None):
    """cfen_mlp_stream_block (csrc/k_stream.hip): mlp_block with the matrices as fragment streams.  wa = packing.pack_stream_pair(W1k, W2k);
    second = (wb, b1b, b2b); proj = (att, packing.pack_stream_sq(Wp)); fold = (B, H, W, C, cs, ws, p)."""
    from ._lib import MlpStreamArgsC
    _cuda(x, wa, b1a, b2a)
    M, D = x.shape
    a = MlpStreamArgsC(x=x.data_ptr(), wa_stream=wa.data_ptr(), b1a=b1a.data_ptr(), b2a=b2a.data_ptr(), M=M, D=D, H=hidden, eps=1e-5)
    if proj is not None:
        _cuda(*proj)
        a.att, a.wp_stream = proj[0].data_ptr(), proj[1].data_ptr()
    if ln is not None:
        _cuda(*ln)
        a.ln_gamma, a.ln_beta = ln[0].data_ptr(), ln[1].data_ptr()
    if second is not None:
        _cuda(*second)
        a.wb_stream, a.b1b, a.b2b = (t.data_ptr() for t in second)
    if fold is None:
        out = _out(out, x.shape, x.dtype, x.device, "mlp_stream_block")
        a.y = out.data_ptr()
    else:
        B, H, W, C, cs, ws, p = fold
        out = _out(out, (B, H, W, cs), x.dtype, x.device, "mlp_stream_block(fold=)", zero=True)
        a.fmap, a.mapH, a.mapW, a.C, a.cs, a.ws, a.p = out.data_ptr(), H, W, C, cs, ws, p
    check(_lib.load().cfen_mlp_stream_block(dtype_code(x.dtype), ctypes.byref(a), current_stream()), "mlp_stream_block")
    return out


def lvit_window(fmap, C, ws, p, packed, name, hidden, cs_out=None, eps=1e-5, out=None):
    """whole LViT block (C = 24, p = 2, ws = 32) map -> map in one launch; `packed` = packing.pack_vit entries of `name` + packing.pack_lvit_window's fragment stream (`hidden` = the stream's hidden width)"""
    from ._lib import LvitArgsC
    _cuda(fmap)
    B, H, W, cs = fmap.shape
    cs_out = cs if cs_out is None else cs_out
    out = _out(out, (B, H, W, cs_out), fmap.dtype, fmap.device, "lvit_window", zero=True)
    g = lambda k: packed[name + k].data_ptr()
    a = LvitArgsC(fmap=fmap.data_ptr(), out=out.data_ptr(), B=B, H=H, W=W, C=C, cs_in=cs, cs_out=cs_out, ws=ws, p=p,
                  w_stream=g(".lw.ws"), be=g(".embed.b"), pos=g(".pos"), ln1_gamma=g(".ln1.g"), ln1_beta=g(".ln1.b"),
                  ln2_gamma=g(".ln2.g"), ln2_beta=g(".ln2.b"), b1a=g(".ffn1.b"), b2a=g(".ffn2.b"), b1b=g(".head1.b"), b2b=g(".head2.b"),
                  hidden=hidden, eps=eps)
    check(_lib.load().cfen_lvit_window(dtype_code(fmap.dtype), ctypes.byref(a), current_stream()), "lvit_window")
    return out


def patchify(fmap, C, ws, p, pool=1, out=None):
    """fmap: NHWC [B,Hf,Wf,cs] -> tokens [B*nwin*S, p*p*C] in (i,j,c) feature order."""
    _cuda(fmap)
    B, Hf, Wf, cs = fmap.shape
    H, W = Hf // pool, Wf // pool
    tok = _out(out, (B * H * W // (p * p), p * p * C), fmap.dtype, fmap.device, "patchify")
    check(_lib.load().cfen_patchify(dtype_code(fmap.dtype), ptr(fmap), ptr(tok), B, H, W, C, cs, ws, p, pool, current_stream()), "patchify")
    return tok


def embed_gather(fmap, C, ws, p, w, bias, pos, out=None):
    """tokens = patchify(fmap) gathered inside the GEMM:  tok @ w.T + bias + tok + pos[row % len(pos)]  -> [M, p*p*C]"""
    _cuda(fmap, w, bias, pos)
    B, H, W, cs = fmap.shape
    D = p * p * C
    out = _out(out, (B * H * W // (p * p), D), fmap.dtype, fmap.device, "embed_gather")
    check(_lib.load().cfen_embed_gather(dtype_code(fmap.dtype), ptr(fmap), B, H, W, C, cs, ws, p, ptr(w), w.shape[1], ptr(bias), ptr(pos),
                                        pos.shape[0] if pos is not None else 0, ptr(out), D, current_stream()), "embed_gather")
    return out


def embed_qkv(fmap, C, ws, p, we, be, pos, ln_g, ln_b, wqkv, eps=1e-5, head_major_heads=0, stream_weights=False, out=None):
    """fused LViT front half (D = p*p*C in {96,192}); we / wqkv with the k axis in packing.kperm32 order for fp16.
    Returns (x1 [M,D], qkv [M,3D]); out = (x1, qkv) places them."""
    from ._lib import EmbedQkvArgsC
    _cuda(fmap, we, be, pos, ln_g, ln_b, wqkv)
    B, H, W, cs = fmap.shape
    D = p * p * C
    M = B * H * W // (p * p)
    x1 = _out(out[0] if out is not None else None, (M, D), fmap.dtype, fmap.device, "embed_qkv (x1)")
    qkv = _out(out[1] if out is not None else None, (M, 3 * D), fmap.dtype, fmap.device, "embed_qkv (qkv)")
    a = EmbedQkvArgsC(fmap=fmap.data_ptr(), B=B, H=H, W=W, C=C, cs=cs, ws=ws, p=p, we=we.data_ptr(), be=be.data_ptr(), pos=pos.data_ptr(),
                      ln_gamma=ln_g.data_ptr(), ln_beta=ln_b.data_ptr(), wqkv=wqkv.data_ptr(), x1=x1.data_ptr(), qkv=qkv.data_ptr(), eps=eps,
                      head_major_heads=head_major_heads)
    fn = _lib.load().cfen_embed_qkv_stream if stream_weights else _lib.load().cfen_embed_qkv   # stream_weights: we / wqkv = packing.pack_stream_rows (D = 384)
    check(fn(dtype_code(fmap.dtype), ctypes.byref(a), current_stream()), "embed_qkv")
    return x1, qkv


def unpatchify(tok, B, H, W, C, cs, ws, p, out=None):
    _cuda(tok)
    fmap = _out(out, (B, H, W, cs), tok.dtype, tok.device, "unpatchify", zero=True)
    check(_lib.load().cfen_unpatchify(dtype_code(tok.dtype), ptr(tok), ptr(fmap), B, H, W, C, cs, ws, p, current_stream()), "unpatchify")
    return fmap


def upsample4(small, cs_out=None, out=None):
    _cuda(small)
    B, h, w, cs_in = small.shape
    cs_out = cs_out or cs_in
    out = _out(out, (B, 4 * h, 4 * w, cs_out), small.dtype, small.device, "upsample4", zero=True)
    check(_lib.load().cfen_upsample4(dtype_code(small.dtype), ptr(small), ptr(out), B, h, w, cs_in, cs_in, cs_out, current_stream()), "upsample4")
    return out


def nchw_to_nhwc(x, cs, dtype, out=None):
    _cuda(x)
    B, C, H, W = x.shape
    out = _out(out, (B, H, W, cs), dtype, x.device, "nchw_to_nhwc")
    check(_lib.load().cfen_nchw_to_nhwc(dtype_code(dtype), ptr(x), ptr(out), B, C, H, W, cs, current_stream()), "nchw_to_nhwc")
    return out


def conv2d(src0, weight, scale, shift, cin, cout, k=3, stride=1, pad=1, reflect=False, src1=None, transpose=False, act=0,
           res0=None, res1=None, cs_out=None, nchw_f32=False, rows_layout=False, toeplitz=False, src2=None, out=None):
    """src*: NHWC [B,H,W,cs]; weight/scale/shift packed by packing.pack_conv*_weight / affine.
    rows_layout: weight from packing.pack_conv_weight_rows -> the LDS-tiled stride-1 kernel."""
    _cuda(src0, src1, src2, weight, scale, shift, res0, res1)
    B, Hin, Win, cs_in = src0.shape
    cout_pad = round_up(cout, 16)
    if transpose:
        Hout, Wout = 2 * Hin, 2 * Win
    else:
        Hout, Wout = (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1
    if nchw_f32:
        out = _out(out, (B, cout, Hout, Wout), torch.float32, src0.device, "conv2d")
        cs_out = cout_pad
    else:
        cs_out = cs_out or round_up(cout, 8)
        out = _out(out, (B, Hout, Wout, cs_out), src0.dtype, src0.device, "conv2d", zero=True)
    a = ConvArgsC(kind=1 if transpose else 0, k=k, stride=stride, pad=pad, reflect=int(reflect), nsrc=3 if src2 is not None else 2 if src1 is not None else 1,
                  B=B, Hin=Hin, Win=Win, Cin=cin, cs_in=cs_in, Cout=cout, Cout_pad=cout_pad, Kpad=weight.shape[-1], cs_out=cs_out,
                  act=act, out_nchw_f32=int(nchw_f32), cs_res=cs_out, wlayout=2 if toeplitz else int(rows_layout),
                  src0=src0.data_ptr(), src1=src1.data_ptr() if src1 is not None else None, weight=weight.data_ptr(),
                  scale=scale.data_ptr(), shift=shift.data_ptr(), res0=res0.data_ptr() if res0 is not None else None,
                  res1=res1.data_ptr() if res1 is not None else None, out=out.data_ptr(),
                  src2=src2.data_ptr() if src2 is not None else None)
    check(_lib.load().cfen_conv2d(dtype_code(src0.dtype), ctypes.byref(a), current_stream()), "conv2d")
    return out


def _stats_ws(B, device, ws=None):
    n = _lib.load().cfen_stats_workspace(B, 128)
    return _out(ws, (n // 4,), torch.float32, device, "stats workspace")


def instnorm_relu_(x, C, eps=1e-5, stats_ws=None):
    """in place on NHWC [B,H,W,cs]; stats_ws: the caller's float32 workspace of cfen_stats_workspace(B, 128) bytes (contents irrelevant)"""
    _cuda(x)
    B, H, W, cs = x.shape
    ws = _stats_ws(B, x.device, stats_ws)
    check(_lib.load().cfen_instnorm_relu(dtype_code(x.dtype), ptr(x), ptr(ws), B, H * W, C, cs, eps, current_stream()), "instnorm_relu")
    return x


def cfsm2g(x0, x1, x2, w, C, out=None, stats_ws=None):
    _cuda(x0, x1, x2, w)
    B, H, W, cs = x0.shape
    out = _out(out, x0.shape, x0.dtype, x0.device, "cfsm2g", zero=True)
    ws = _stats_ws(B, x0.device, stats_ws)
    check(_lib.load().cfen_cfsm2g(dtype_code(x0.dtype), ptr(x0), ptr(x1), ptr(x2), ptr(out), ptr(w), ptr(ws), B, H * W, C, cs,
                                  current_stream()), "cfsm2g")
    return out


def tensor2im_u8(x, out=None):
    """(1|3,H,W) fp32 CUDA tensor in [-1,1] -> (H,W,3) uint8 CUDA tensor; util.tensor2im on the device"""
    _cuda(x)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("tensor2im_u8 needs a contiguous (C,H,W) float32 tensor")
    C, H, W = x.shape
    out = _out(out, (H, W, 3), torch.uint8, x.device, "tensor2im_u8")
    check(_lib.load().cfen_tensor2im_u8(ptr(x), ptr(out), C, H, W, current_stream()), "tensor2im_u8")
    return out


def tile_gather(img, T, ny, nx, t0, B, out=None):
    """cfen_tile_gather: tiles [t0, t0 + B) of the ny x nx tile plan (tiled.tile_grid) of `img` -- (H,W,3) uint8 or (3,H,W) fp32 CUDA tensor -- into
    the network's input slab: (B,T,T,3) uint8 or (B,3,T,T) fp32 (`out`, else allocated).  Tile indices past ny*nx repeat the last tile."""
    _cuda(img, out)
    u8 = img.dtype == torch.uint8
    if img.dim() != 3 or (u8 and img.shape[2] != 3) or (not u8 and (img.dtype != torch.float32 or img.shape[0] != 3)):
        raise ValueError("tile_gather needs a contiguous (H,W,3) uint8 or (3,H,W) float32 image, got %s %s" % (tuple(img.shape), img.dtype))
    H, W = (img.shape[0], img.shape[1]) if u8 else (img.shape[1], img.shape[2])
    shape = (B, T, T, 3) if u8 else (B, 3, T, T)
    if out is None:
        out = torch.empty(shape, dtype=img.dtype, device=img.device)
    elif tuple(out.shape) != shape or out.dtype != img.dtype:
        raise ValueError("tile_gather: out must be a %s tensor of shape %s" % (img.dtype, shape))
    check(_lib.load().cfen_tile_gather(int(u8), ptr(img), ptr(out), H, W, T, ny, nx, t0, B, current_stream()), "tile_gather")
    return out


def tile_blend(arena, B, T, H, W, ny, nx, overlap, output_u8=False, out=None, lane0=0):
    """cfen_tile_blend: the tile outputs in `arena` -- the forwards' [xr | xs | xd] output slabs of B tiles each, back to back, float32 or float16 --
    blended into the H x W image: [xr (3,H,W), xs (1,H,W), xd (3,H,W)] float32, or with output_u8 three (H,W,3) uint8 images (util.tensor2im's bytes);
    out = the three tensors, placed by the caller.  lane0: the lane of the image's tile 0 in the slab `arena` starts at, when the image shares its
    slabs with other images (tiled.pack_plan): tile t is read from global slot lane0 + t, so the arena holds ceil((lane0 + ny*nx) / B) slabs"""
    _cuda(arena)
    if not isinstance(lane0, int) or isinstance(lane0, bool) or not 0 <= lane0 < B:
        raise ValueError("tile_blend: lane0 = %r must be an int in 0 .. B - 1 = %d" % (lane0, B - 1))
    need = -(-(lane0 + ny * nx) // B) * 7 * B * T * T
    if arena.dtype not in (torch.float32, torch.float16) or arena.numel() < need:
        raise ValueError("tile_blend: the arena must hold %d float32 / float16 elements (%d slabs of 7*%d*%d*%d), got %d %s"
                         % (need, need // (7 * B * T * T), B, T, T, arena.numel(), arena.dtype))
    dev = arena.device
    if out is not None and len(out) != 3:
        raise ValueError("tile_blend: out must be the three output tensors [xr, xs, xd]")
    given = out if out is not None else (None, None, None)
    if output_u8:
        outs = [_out(o, (H, W, 3), torch.uint8, dev, "tile_blend") for o in given]
    else:
        outs = [_out(o, (c, H, W), torch.float32, dev, "tile_blend") for o, c in zip(given, (3, 1, 3))]
    # the dtype argument carries two fields (include/cfen_hip.h): bits 0..7 the element type, bits 8..23 lane0
    check(_lib.load().cfen_tile_blend(dtype_code(arena.dtype) | (lane0 << 8), ptr(arena), B, T, H, W, ny, nx, overlap, int(output_u8), ptr(outs[0]),
                                      ptr(outs[1]), ptr(outs[2]), current_stream()), "tile_blend")
    return outs


def x8_expand(images, m=0, out=None):
    """cfen_x8_expand: the eight flips / transposes of image `m` of `images` -- (M,T,T,3) uint8 or (M,3,T,T) fp32 CUDA tensor -- as the network's
    batch-8 input slab, (8,T,T,3) uint8 or (8,3,T,T) fp32 (`out`, else allocated), in the variant order of ensemble.py"""
    _cuda(images, out)
    u8 = images.dtype == torch.uint8
    if images.dim() != 4 or not images.is_contiguous() or (u8 and images.shape[3] != 3) or \
            (not u8 and (images.dtype != torch.float32 or images.shape[1] != 3)) or images.shape[1 if u8 else 2] != images.shape[2 if u8 else 3]:
        raise ValueError("x8_expand needs contiguous (M,T,T,3) uint8 or (M,3,T,T) float32 square images, got %s %s" % (tuple(images.shape), images.dtype))
    M, T = images.shape[0], images.shape[2]
    shape = (8, T, T, 3) if u8 else (8, 3, T, T)
    if out is None:
        out = torch.empty(shape, dtype=images.dtype, device=images.device)
    elif tuple(out.shape) != shape or out.dtype != images.dtype or not out.is_contiguous():
        raise ValueError("x8_expand: out must be a contiguous %s tensor of shape %s" % (images.dtype, shape))
    check(_lib.load().cfen_x8_expand(int(u8), ptr(images), ptr(out), M, int(m), T, current_stream()), "x8_expand")
    return out


def x8_merge(arena, M, T, output_u8=False, out=None):
    """cfen_x8_merge: `arena` holds M forward output slabs back to back, float32 or float16, slab m = [xr (8,3,T,T) | xs (8,1,T,T) | xd (8,3,T,T)] of
    the eight variants of image m; returns the ensemble [xr (M,3,T,T), xs (M,1,T,T), xd (M,3,T,T)] float32 -- each variant mapped back, summed in
    fp32 in variant order, times 1/8 -- or with output_u8 three (M,T,T,3) uint8 images (util.tensor2im's bytes of those values).  `out`: optional flat
    float32 buffer of 7*M*T*T elements that receives [xr | xs | xd] back to back, as forward(x, out=) lays them out; the results are views of it"""
    _cuda(arena, out)
    need = M * 56 * T * T
    if arena.dtype not in (torch.float32, torch.float16) or arena.dim() != 1 or not arena.is_contiguous() or arena.numel() < need:
        raise ValueError("x8_merge: the arena must be a flat tensor of %d float32 / float16 elements (%d slabs of 7*8*%d*%d), got %s %s"
                         % (need, M, T, T, tuple(arena.shape), arena.dtype))
    dev = arena.device
    px = M * T * T
    if output_u8:
        if out is not None:
            raise ValueError("x8_merge: output_u8 allocates its own (M,T,T,3) uint8 outputs: no `out` buffer")
        outs = [torch.empty(M, T, T, 3, dtype=torch.uint8, device=dev) for _ in range(3)]
    elif out is not None:
        if out.dtype != torch.float32 or out.dim() != 1 or out.numel() != 7 * px or not out.is_contiguous() or out.device != dev:
            raise ValueError("x8_merge: out must be a flat contiguous float32 buffer of 7*M*T*T = %d elements on the arena's device" % (7 * px))
        outs = [out[:3 * px].view(M, 3, T, T), out[3 * px:4 * px].view(M, 1, T, T), out[4 * px:].view(M, 3, T, T)]
    else:
        outs = [torch.empty(M, c, T, T, dtype=torch.float32, device=dev) for c in (3, 1, 3)]
    check(_lib.load().cfen_x8_merge(dtype_code(arena.dtype), ptr(arena), M, T, int(output_u8), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                    current_stream()), "x8_merge")
    return outs


def resample_u8(images_u8, size, filter="bicubic", out=None):
    """cfen_resample_u8 (include/cfen_resample.h): PIL's Image.resize((W2, H2), filter) of contiguous (B,H,W,3) uint8 CUDA images, byte for byte:
    (B,H2,W2,3) uint8 for size = (H2, W2).  The integer tables come from resample.coefficients (uploaded once per axis pair, filter and device); the
    horizontal pass runs if W2 != W into a uint8 intermediate, the vertical pass if H2 != H; with neither the result is a copy.  out: the caller's
    (B,H2,W2,3) uint8 tensor, which may be a lane of a larger slab (no alignment is assumed)."""
    from . import resample
    _rgb_batch("resample_u8", images_u8=images_u8)
    B, H, W, _ = images_u8.shape
    H2, W2 = (int(s) for s in size)
    if min(H2, W2) < 1:
        raise ValueError("resample_u8: empty image or target, %s -> %s" % (tuple(images_u8.shape), (H2, W2)))
    dev = images_u8.device
    out = _out(out, (B, H2, W2, 3), torch.uint8, dev, "resample_u8")
    xb, xc = resample.device_tables(W, W2, filter, dev) if W2 != W else (None, None)
    yb, yc = resample.device_tables(H, H2, filter, dev) if H2 != H else (None, None)
    tmp = torch.empty(B * H * W2 * 3, dtype=torch.uint8, device=dev) if xb is not None and yb is not None else None
    check(_lib.load().cfen_resample_u8(ptr(images_u8), B, H, W, ptr(xb), ptr(xc), xc.shape[1] if xc is not None else 0, W2,
                                       ptr(yb), ptr(yc), yc.shape[1] if yc is not None else 0, H2, ptr(tmp), ptr(out), current_stream()), "resample_u8")
    return out      # (tmp goes back to torch's allocator on the stream it was used on)


def _guided_params(what, radius, eps):
    radius = _int_arg(what, "radius", radius, 1, 16)
    eps = _float_arg(what, "eps", eps, lambda e: math.isfinite(e) and e > 0, "finite and > 0")
    return radius, eps * 255.0 * 255.0          # eps is in squared units of the [0, 1] scale; the kernels work on bytes


def _field(what, name, t, guide_hi):
    """the coefficient (or delta) field an apply kernel upsamples to the size of guide_hi"""
    _tensor_arg(what, name, t, (guide_hi.shape[0], None, None, 6), torch.float32, like=guide_hi)


def guided_coef_u8(guide_lo, src_lo, radius=2, eps=1e-4, out=None):
    """cfen_guided_coef_u8 (include/cfen_guided.h): the smoothed coefficients of the local linear model src_lo ~ a * guide_lo + b, fitted per pixel
    and channel over a (2 radius + 1)^2 window: (B,h,w,6) float32 = [abar_R, abar_G, abar_B, bbar_R, bbar_G, bbar_B] on the 0..255 scale.
    guide_lo, src_lo: contiguous (B,h,w,3) uint8 CUDA tensors; eps regularises the variance, in squared units of the [0, 1] scale.  out: the
    caller's (B,h,w,6) float32 tensor."""
    _rgb_pair("guided_coef_u8", guide_lo=guide_lo, src_lo=src_lo)
    radius, eps255 = _guided_params("guided_coef_u8", radius, eps)
    B, h, w, _ = guide_lo.shape
    dev = guide_lo.device
    out = _out(out, (B, h, w, 6), torch.float32, dev, "guided_coef_u8")
    tmp = torch.empty(B, h, w, 6, dtype=torch.float32, device=dev)
    check(_lib.load().cfen_guided_coef_u8(ptr(guide_lo), ptr(src_lo), B, h, w, radius, eps255, ptr(tmp), ptr(out), current_stream()), "guided_coef_u8")
    return out      # (tmp goes back to torch's allocator on the stream it was used on)


def guided_apply_u8(coef, guide_hi, out=None):
    """cfen_guided_apply_u8 (include/cfen_guided.h): coef (B,h,w,6) float32 of guided_coef_u8, upsampled bilinearly (half-pixel centres, edge clamp)
    to the size of guide_hi (B,H,W,3) uint8 and applied to it: (B,H,W,3) uint8 = clamp(floor(Abar * guide_hi + Bbar + 0.5), 0, 255).  out: the
    caller's (B,H,W,3) uint8 tensor, which may be a lane of a larger slab (no alignment is assumed)."""
    _rgb_batch("guided_apply_u8", guide_hi=guide_hi)
    _field("guided_apply_u8", "coef", coef, guide_hi)
    B, H, W, _ = guide_hi.shape
    out = _out(out, (B, H, W, 3), torch.uint8, guide_hi.device, "guided_apply_u8")
    check(_lib.load().cfen_guided_apply_u8(ptr(coef), B, coef.shape[1], coef.shape[2], ptr(guide_hi), H, W, ptr(out), current_stream()), "guided_apply_u8")
    return out


def guided_upsample_u8(guide_hi, guide_lo, src_lo, radius=2, eps=1e-4, out=None):
    """Guided upsampling (He & Sun, "Fast Guided Filter") of src_lo (B,h,w,3) uint8 to the size of guide_hi (B,H,W,3) uint8, where guide_lo
    (B,h,w,3) is the low-resolution guide src_lo was computed from: guided_apply_u8(guided_coef_u8(guide_lo, src_lo, radius, eps), guide_hi).
    Three launches."""
    _rgb_batch("guided_upsample_u8", guide_hi=guide_hi, guide_lo=guide_lo, src_lo=src_lo)
    if guide_hi.shape[0] != guide_lo.shape[0]:
        raise ValueError("guided_upsample_u8: guide_hi %s and guide_lo %s differ in batch" % (tuple(guide_hi.shape), tuple(guide_lo.shape)))
    return guided_apply_u8(guided_coef_u8(guide_lo, src_lo, radius, eps), guide_hi, out=out)


def temporal_blend(guide, prev_guide, coef, state, radius=2, motion=8.0, strength=0.8, have_state=True, out=None):
    """cfen_temporal_blend (include/cfen_temporal.h): the motion-gated recursion S_t = c_t + k (S_{t-1} - c_t) on the coefficient fields coef
    (B,h,w,6) float32 of the B consecutive working-resolution frames guide (B,h,w,3) uint8, in one launch: returns delta (B,h,w,6) float32 =
    S_t - c_t and updates state (h,w,6) float32 in place to S of the last frame.  prev_guide (h,w,3) uint8 is the frame before guide[0]; it is only
    read.  have_state False: guide[0] is the first frame of a stream, prev_guide (may be None) and what state holds are not looked at.  out: the
    caller's (B,h,w,6) float32 tensor."""
    _rgb_batch("temporal_blend", guide=guide)
    B, h, w, _ = guide.shape
    dev = guide.device
    _tensor_arg("temporal_blend", "coef", coef, (B, h, w, 6), torch.float32, like=guide)
    _tensor_arg("temporal_blend", "state", state, (h, w, 6), torch.float32, like=guide)
    have_state = bool(have_state)
    if have_state:
        _tensor_arg("temporal_blend with have_state", "prev_guide", prev_guide, (h, w, 3), torch.uint8, like=guide)
    radius = _int_arg("temporal_blend", "radius", radius, 1, 16)
    motion = _float_arg("temporal_blend", "motion", motion, lambda m: math.isfinite(m) and m > 0, "finite and > 0")
    strength = _float_arg("temporal_blend", "strength", strength, lambda s: 0 <= s < 1, "in [0, 1)")
    out = _out(out, (B, h, w, 6), torch.float32, dev, "temporal_blend")
    check(_lib.load().cfen_temporal_blend(ptr(guide), ptr(prev_guide if have_state else None), ptr(coef), B, h, w, radius, motion, strength,
                                          int(have_state), ptr(state), ptr(out), current_stream()), "temporal_blend")
    return out


def temporal_apply_u8(delta, guide_hi, src_hi, out=None):
    """cfen_temporal_apply_u8 (include/cfen_temporal.h): delta (B,h,w,6) float32 of temporal_blend, upsampled bilinearly as guided_apply_u8 upsamples
    to the size of guide_hi and src_hi (B,H,W,3) uint8 -- the hazy and the dehazed frames -- and applied as a correction of src_hi:
    (B,H,W,3) uint8 = clamp(floor(src_hi + DA * guide_hi + DB + 0.5), 0, 255).  out: the caller's (B,H,W,3) uint8 tensor, which may be a lane of a
    larger slab (no alignment is assumed)."""
    _rgb_pair("temporal_apply_u8", guide_hi=guide_hi, src_hi=src_hi)
    _field("temporal_apply_u8", "delta", delta, guide_hi)
    B, H, W, _ = guide_hi.shape
    out = _out(out, (B, H, W, 3), torch.uint8, guide_hi.device, "temporal_apply_u8")
    check(_lib.load().cfen_temporal_apply_u8(ptr(delta), B, delta.shape[1], delta.shape[2], ptr(guide_hi), ptr(src_hi), H, W, ptr(out), current_stream()),
          "temporal_apply_u8")
    return out


def _motion_block(what, block):
    return _int_arg(what, "block", block, 8, 32, choices=(8, 16, 32))


def _pair(out):
    if out is None:
        return None, None
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out must be a pair of tensors")
    return out


def motion_search_u8(guide, prev_guide, block, range, bias, out=None):
    """cfen_motion_search_u8 (include/cfen_motion.h): per block x block block of each of the B consecutive working-resolution frames guide (B,h,w,3)
    uint8, the displacement (dy, dx) within +-range at which the previous frame matches best (the smallest 16 SAD + bias (|dy| + |dx|) 3 n_b, ties
    to the shorter and then the lexicographically smaller vector), in one launch: returns (vec (B,bh,bw,2) int16, sad (B,bh,bw) int32, the
    winner's SAD).  prev_guide (h,w,3) uint8 is the frame before guide[0].  out: the caller's (vec, sad) pair."""
    _rgb_batch("motion_search_u8", guide=guide)
    B, h, w, _ = guide.shape
    dev = guide.device
    _tensor_arg("motion_search_u8", "prev_guide", prev_guide, (h, w, 3), torch.uint8, like=guide)
    block = _motion_block("motion_search_u8", block)
    r = _int_arg("motion_search_u8", "range", range, 1, 16)
    bi = _int_arg("motion_search_u8", "bias", bias, 0, 255)
    bh, bw = -(-h // block), -(-w // block)
    vec, sad = _pair(out)
    vec = _out(vec, (B, bh, bw, 2), torch.int16, dev, "motion_search_u8")
    sad = _out(sad, (B, bh, bw), torch.int32, dev, "motion_search_u8")
    check(_lib.load().cfen_motion_search_u8(ptr(guide), ptr(prev_guide), B, h, w, block, r, bi, ptr(vec), ptr(sad), current_stream()), "motion_search_u8")
    return vec, sad


def motion_warp(vec, prev_guide, state, block, out=None):
    """cfen_motion_warp (include/cfen_motion.h): the previous working-resolution frame prev_guide (h,w,3) uint8 and the recursion's state (h,w,6)
    float32 fetched, per pixel, from where its block's vector vec (bh,bw,2) int16 of motion_search_u8 points (coordinates clamped to the
    frame): returns (prev_out (h,w,3) uint8, state_out (h,w,6) float32).  A pure gather; inputs and outputs must not overlap.  out: the caller's
    (prev_out, state_out) pair."""
    _tensor_arg("motion_warp", "prev_guide", prev_guide, (None, None, 3), torch.uint8)
    h, w, _ = prev_guide.shape
    dev = prev_guide.device
    block = _motion_block("motion_warp", block)
    bh, bw = -(-h // block), -(-w // block)
    _tensor_arg("motion_warp", "vec", vec, (bh, bw, 2), torch.int16, like=prev_guide)
    _tensor_arg("motion_warp", "state", state, (h, w, 6), torch.float32, like=prev_guide)
    prev_out, state_out = _pair(out)
    prev_out = _out(prev_out, (h, w, 3), torch.uint8, dev, "motion_warp")
    state_out = _out(state_out, (h, w, 6), torch.float32, dev, "motion_warp")
    check(_lib.load().cfen_motion_warp(ptr(vec), ptr(prev_guide), ptr(state), h, w, block, ptr(prev_out), ptr(state_out), current_stream()), "motion_warp")
    return prev_out, state_out


def motion_refine_u8(guide, prev_guide, vec, block, subpel, bias, out=None):
    """cfen_motion_refine_u8 (include/cfen_subpel.h): the whole-pixel block vectors vec (B,bh,bw,2) int16 of motion_search_u8 on the same guide
    (B,h,w,3) uint8 and prev_guide (h,w,3) uint8, refined to 1 / subpel pixel (subpel 2 or 4) by an exhaustive search of the (2 subpel - 1)^2
    bilinearly sampled positions within +-3/4 pixel, in one launch: returns (vec4 (B,bh,bw,2) int16 in QUARTER pixels, sad4 (B,bh,bw) int32, the
    winner's SAD).  out: the caller's (vec4, sad4) pair."""
    _rgb_batch("motion_refine_u8", guide=guide)
    B, h, w, _ = guide.shape
    dev = guide.device
    _tensor_arg("motion_refine_u8", "prev_guide", prev_guide, (h, w, 3), torch.uint8, like=guide)
    block = _motion_block("motion_refine_u8", block)
    q = _int_arg("motion_refine_u8", "subpel", subpel, 2, 4, choices=(2, 4))
    bi = _int_arg("motion_refine_u8", "bias", bias, 0, 255)
    bh, bw = -(-h // block), -(-w // block)
    _tensor_arg("motion_refine_u8", "vec", vec, (B, bh, bw, 2), torch.int16, like=guide)
    vec4, sad4 = _pair(out)
    vec4 = _out(vec4, (B, bh, bw, 2), torch.int16, dev, "motion_refine_u8")
    sad4 = _out(sad4, (B, bh, bw), torch.int32, dev, "motion_refine_u8")
    check(_lib.load().cfen_motion_refine_u8(ptr(guide), ptr(prev_guide), ptr(vec), B, h, w, block, q, bi, ptr(vec4), ptr(sad4), current_stream()),
          "motion_refine_u8")
    return vec4, sad4


def motion_warp_subpel(vec4, prev_guide, state, block, out=None):
    """cfen_motion_warp_subpel (include/cfen_subpel.h): motion_warp for vectors in quarter pixels: the previous frame prev_guide (h,w,3) uint8
    sampled bilinearly in integers, and the recursion's state (h,w,6) float32 lerped in fp32, where each pixel's block vector vec4 (bh,bw,2) int16
    of motion_refine_u8 points (tap coordinates clamped to the frame): returns (prev_out (h,w,3) uint8, state_out (h,w,6) float32).  Multiples of 4
    give motion_warp with vec4 / 4.  Inputs and outputs must not overlap.  out: the caller's (prev_out, state_out) pair."""
    _tensor_arg("motion_warp_subpel", "prev_guide", prev_guide, (None, None, 3), torch.uint8)
    h, w, _ = prev_guide.shape
    dev = prev_guide.device
    block = _motion_block("motion_warp_subpel", block)
    bh, bw = -(-h // block), -(-w // block)
    _tensor_arg("motion_warp_subpel", "vec4", vec4, (bh, bw, 2), torch.int16, like=prev_guide)
    _tensor_arg("motion_warp_subpel", "state", state, (h, w, 6), torch.float32, like=prev_guide)
    prev_out, state_out = _pair(out)
    prev_out = _out(prev_out, (h, w, 3), torch.uint8, dev, "motion_warp_subpel")
    state_out = _out(state_out, (h, w, 6), torch.float32, dev, "motion_warp_subpel")
    check(_lib.load().cfen_motion_warp_subpel(ptr(vec4), ptr(prev_guide), ptr(state), h, w, block, ptr(prev_out), ptr(state_out), current_stream()),
          "motion_warp_subpel")
    return prev_out, state_out


def _image_pair(what, a, b):
    """the two images of a full-reference score as a batch: (a, b, u8, B, C, H, W)"""
    _cuda(a, b)
    if a.dim() == 3:
        a, b = a[None], b[None]
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        raise ValueError("%s: the two images differ in shape, dtype or device: %s %s against %s %s" % (what, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
    u8 = a.dtype == torch.uint8
    if a.dim() != 4 or (u8 and a.shape[3] != 3) or (not u8 and (a.dtype != torch.float32 or a.shape[1] not in (1, 3))):
        raise ValueError("%s needs (B,H,W,3) uint8 or (B,1|3,H,W) float32 images, got %s %s" % (what, tuple(a.shape), a.dtype))
    B, C, H, W = (a.shape[0], 3, a.shape[1], a.shape[2]) if u8 else tuple(a.shape)
    return a, b, u8, B, C, H, W


def _image_pair_scores(what, ncol, a, b, value_range, out):
    """cfen_<what> on the pair (a, b): the (B, ncol) float64 tensor of its results"""
    a, b, u8, B, C, H, W = _image_pair(what, a, b)
    lib = _lib.load()
    scratch = _scratch_for(what, getattr(lib, "cfen_%s_bytes" % what), (B, C, H, W), a.device)      # sizes it refuses: cfen_<what>'s own error
    if out is None:
        out = torch.empty(B, ncol, dtype=torch.float64, device=a.device)
    elif tuple(out.shape) != (B, ncol) or out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous (%d, %d) float64 CUDA tensor" % (what, B, ncol))
    lo, hi = value_range
    check(getattr(lib, "cfen_" + what)(int(u8), ptr(a), ptr(b), B, C, H, W, float(lo), float(hi), ptr(scratch), ptr(out), current_stream()), what)
    return out


def flicker_u8(guide, prev_guide, tgt, prev_tgt, vec, block, tol, out=None):
    """cfen_flicker_u8 (include/cfen_flicker.h): the integer sums behind the flicker along the motion of B consecutive working-resolution frames.
    guide, tgt (B,h,w,3) uint8: the hazy frames and the frames scored; prev_guide, prev_tgt (h,w,3) uint8: the frames before guide[0] and tgt[0];
    vec None (the zero field) or (B,bh,bw,2) int16 as ops.motion_search_u8 writes it; block 8, 16 or 32; tol 0 .. 255.  tgt may be guide and
    prev_tgt prev_guide.  Returns (B,8) int64: n_cov, n_match, sum_matched dI, sum_matched dF, sum_matched eF, sum_covered dF, sum_covered dI, 0;
    flicker.scores_from_sums turns them into scores.  Two launches; the same bits at every batch size and on every stream.  out: the caller's
    (B,8) int64 tensor."""
    _rgb_pair("flicker_u8", guide=guide, tgt=tgt)
    B, h, w, _ = guide.shape
    dev = guide.device
    _tensor_arg("flicker_u8", "prev_guide", prev_guide, (h, w, 3), torch.uint8, like=guide)
    _tensor_arg("flicker_u8", "prev_tgt", prev_tgt, (h, w, 3), torch.uint8, like=guide)
    block = _motion_block("flicker_u8", block)
    tl = _int_arg("flicker_u8", "tol", tol, 0, 255)
    bh, bw = -(-h // block), -(-w // block)
    if vec is not None:
        _tensor_arg("flicker_u8", "vec", vec, (B, bh, bw, 2), torch.int16, like=guide)
    lib = _lib.load()
    scratch = _scratch_for("flicker_u8", lib.cfen_flicker_bytes, (B, h, w), dev, "B <= 65536, h, w <= 16384, at most 2^31 - 1 tiles of 64 x 64")
    out = _out(out, (B, 8), torch.int64, dev, "flicker_u8")
    check(lib.cfen_flicker_u8(ptr(guide), ptr(prev_guide), ptr(tgt), ptr(prev_tgt), ptr(vec), B, h, w, block, tl, ptr(scratch), ptr(out),
                              current_stream()), "flicker_u8")
    return out


def plane_metrics(a, b, H, W, chroma, depth=8, prev=None):
    """cfen_plane_metrics (include/cfen_planes.h): B frames of a YCbCr stream against B frames of a ground-truth stream, plane by plane on the
    samples as stored.  a, b: (B, frame_bytes) uint8 CUDA tensors, the FRAME payloads of a .y4m stream as they are (rows any number >=
    frame_bytes of bytes apart; at depth 9 .. 16 little-endian 16-bit samples at even addresses); chroma: one of yuv.CHROMA; prev: None, or
    (a_prev, b_prev), the frame pair before frame 0 as two (frame_bytes,) tensors.  Returns (sse, dt, ssim, count), each (B, 3) over the planes
    Y, Cb, Cr: sse, dt and count int64, ssim float64 (NaN for a plane under 11 samples on a side or absent).  Two launches; the same bits at
    every batch size, stride, alignment and stream."""
    from . import yuv
    code = yuv.chroma_code(chroma)
    depth = _int_arg("plane_metrics", "depth", depth, 8, yuv.MAX_DEPTH)
    H, W = _int_arg("plane_metrics", "H", H, 1, yuv.MAX_EDGE), _int_arg("plane_metrics", "W", W, 1, yuv.MAX_EDGE)
    nbytes = yuv.frame_bytes(H, W, chroma, depth)
    sa, sb = _yuv_frames("plane_metrics (a)", a, nbytes), _yuv_frames("plane_metrics (b)", b, nbytes)
    if a.shape[0] != b.shape[0] or a.device != b.device:
        raise ValueError("plane_metrics: a holds %d frames on %s and b %d on %s" % (a.shape[0], a.device, b.shape[0], b.device))
    B, dev = a.shape[0], a.device
    pa = pb = None
    if prev is not None:
        pa, pb = prev
        for name, t in (("prev[0]", pa), ("prev[1]", pb)):
            _tensor_arg("plane_metrics", name, t, (nbytes,), torch.uint8, like=a)
    lib = _lib.load()
    scratch = _scratch_for("plane_metrics", lib.cfen_plane_metrics_bytes, (B, H, W, code), dev, "B <= %d, H W <= 2^31" % yuv.MAX_BATCH)
    out = torch.empty(B, 3, 4, dtype=torch.int64, device=dev)
    check(lib.cfen_plane_metrics(ptr(a), sa, ptr(b), sb, ptr(pa), ptr(pb), B, H, W, code, depth, ptr(scratch), ptr(out), current_stream()),
          "plane_metrics")
    return out[:, :, 0], out[:, :, 1], out.view(torch.float64)[:, :, 2], out[:, :, 3]          # views of one tensor: no launch of their own


def image_metrics(a, b, value_range=(-1.0, 1.0), out=None):
    """cfen_image_metrics: per image pair (sse, ssim) as two float64 CUDA tensors of shape (B,), in one fused pass.

    a, b: (B,H,W,3) uint8, scored as v / 255, or (B,C,H,W) float32 with C 1 or 3, scored as (v - lo) / (hi - lo) for value_range = (lo, hi); an
    image without the batch dimension is taken as a batch of one.  ssim is the reference's pytorch_msssim.ssim(window_size=11, val_range=1): Gaussian
    window, valid convolution, mean over channels and window positions.  sse is the sum of squared differences on the 0..255 scale over all values
    (exact for uint8); metrics.psnr_from_sse turns it into PSNR.  H, W >= 11."""
    out = _image_pair_scores("image_metrics", 2, a, b, value_range, out)
    return out[:, 0], out[:, 1]


def image_msssim(a, b, value_range=(-1.0, 1.0), out=None):
    """cfen_image_msssim: per image pair (sse, levels): sse a float64 CUDA tensor of shape (B,), levels a (B,5,2) float64 CUDA tensor of
    (ssim_l, cs_l) over the five levels of the 2 x 2 mean pyramid -- the reference's pytorch_msssim.msssim(window_size=11, val_range=1,
    normalize=None) up to the final powers and product, which metrics.msssim_from_levels takes on the host in float64.

    a, b, value_range: as for image_metrics; min(H, W) >= 176.  sse and levels[:, 0, 0] are bitwise what image_metrics returns for the same input.
    out: a contiguous (B, 11) float64 CUDA tensor to write into (sse, then the ten level values); the results are views of it."""
    out = _image_pair_scores("image_msssim", 11, a, b, value_range, out)
    return out[:, 0], out[:, 1:].unflatten(1, (5, 2))


_srgb_tables = {}      # device -> the 256-entry sRGB-to-linear table of include/cfen_colordiff.h


def _srgb_table(device):
    if device not in _srgb_tables:
        from . import metrics
        _srgb_tables[device] = torch.from_numpy(metrics.srgb_linear_table()).to(device)
    return _srgb_tables[device]


def image_ciede2000(a, b, map=None, out=None):
    """cfen_ciede2000_u8 (include/cfen_colordiff.h): per image pair the mean CIEDE2000 colour difference as a float64 CUDA tensor of shape (B,).

    a, b: (B,H,W,3) uint8 CUDA tensors read as sRGB (a is colour 1); an image without the batch dimension is taken as a batch of one.  map: None,
    True (a fresh (B,H,W) float32 tensor) or the caller's contiguous (B,H,W) float32 CUDA tensor for the per-pixel values; with a map the result is
    (means, map).  out: the caller's contiguous (B,) float64 CUDA tensor.  The means are the same bits with and without a map, at every batch size
    and on every stream."""
    if a.dim() == 3:
        a, b = a[None], b[None]
    _rgb_pair("image_ciede2000", a=a, b=b)
    B, H, W, _ = a.shape
    lib = _lib.load()
    scratch = _scratch_for("image_ciede2000", lib.cfen_ciede2000_bytes, (B, H, W), a.device, "B <= 65535, H, W <= 65536")
    if map is True:
        map = torch.empty(B, H, W, dtype=torch.float32, device=a.device)
    elif map is not None:
        map = _out(map, (B, H, W), torch.float32, a.device, "image_ciede2000 (map)")
    out = _out(out, (B,), torch.float64, a.device, "image_ciede2000")
    check(lib.cfen_ciede2000_u8(ptr(a), ptr(b), B, H, W, ptr(_srgb_table(a.device)), ptr(scratch), ptr(map), ptr(out), current_stream()), "image_ciede2000")
    return out if map is None else (out, map)


NOREF_TILE_W, NOREF_TILE_H = 64, 64      # CFEN_NOREF_TILE_W / _H of include/cfen_noref.h: one workgroup, one scratch record, per tile
NOREF_RECORD_BYTES = 2080                 # CFEN_NOREF_RECORD_BYTES
NOREF_MAX_RADIUS = 16                     # CFEN_NOREF_MAX_RADIUS


def _noref(what, hazy, out, radius, map_hazy, map_out):
    """cfen_noref_u8 on the pairs (hazy, out): (counts, grad, dark_hazy, dark_out), a map that was not asked for None"""
    _rgb_pair(what, hazy=hazy, out=out)
    B, H, W, _ = hazy.shape
    dev = hazy.device
    lib = _lib.load()
    scratch = _scratch_for(what, lib.cfen_noref_bytes, (B, H, W, int(radius)), dev, "B <= 65535, H, W <= 65536, radius 0 .. %d" % NOREF_MAX_RADIUS)
    counts = torch.empty(B, 2, 259, dtype=torch.int64, device=dev)
    grad = torch.empty(B, 2, dtype=torch.float64, device=dev)
    d0 = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if map_hazy else None
    d1 = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if map_out else None
    check(lib.cfen_noref_u8(ptr(hazy), ptr(out), B, H, W, int(radius), ptr(scratch), ptr(counts), ptr(grad), ptr(d0), ptr(d1), current_stream()), what)
    return counts, grad, d0, d1


def image_noref(hazy, out, radius=7, maps=False):
    """cfen_noref_u8 (include/cfen_noref.h): the raw no-reference statistics of B pairs (hazy input, dehazed output), as CUDA tensors.

    hazy, out: (B,H,W,3) uint8 CUDA tensors of equal shape; an image without the batch dimension is taken as a batch of one.  radius: the dark
    channel's window is (2 radius + 1)^2, 0 .. 16.  Returns (counts, grad): counts (B,2,259) int64 -- per side (0 hazy, 1 out) the 256 bins of
    the luma histogram, dark_sum, the saturation count (side 0: sat_in, side 1: sat_new) and a reserved 0 -- and grad (B,2) float64, the
    gradient sums.  With maps=True the result is (counts, grad, dark_hazy, dark_out), the two (B,H,W) uint8 dark-channel maps.  The same bits
    with and without maps, at every batch size and on every stream; metrics.noref_from_stats turns the statistics into scores."""
    if hazy.dim() == 3 and out.dim() == 3:
        hazy, out = hazy[None], out[None]
    counts, grad, d0, d1 = _noref("image_noref", hazy, out, radius, maps, maps)
    return (counts, grad, d0, d1) if maps else (counts, grad)


def dark_channel_u8(images, radius=7):
    """the dark channel (He, Sun and Tang 2009) of (B,H,W,3) uint8 CUDA images as a (B,H,W) uint8 CUDA tensor: per pixel the minimum of
    min(R, G, B) over the (2 radius + 1)^2 window clipped to the image (cfen_noref_u8 with the same images on both sides; an (H,W,3) image
    gives an (H,W) map)"""
    single = images.dim() == 3
    if single:
        images = images[None]
    dark = _noref("dark_channel_u8", images, images, radius, True, False)[2]
    return dark[0] if single else dark


def yuv_table(coef, oy):
    """a cfen_yuv_table (include/cfen_yuv.h) from a (3,3) integer table of yuv.tables and its luma offset: passed to the kernels by value"""
    t = _lib.YuvTableC()
    flat = [int(v) for row in coef for v in row]
    if len(flat) != 9:
        raise ValueError("yuv_table needs a 3 x 3 table, got %d entries" % len(flat))
    for k, v in enumerate(flat):
        t.coef[k] = v
    t.luma_offset = int(oy)
    return t


@functools.lru_cache(maxsize=None)
def _yuv_table_for(matrix, full_range, inverse):
    """the forward or inverse table of yuv.tables as a cfen_yuv_table, built once per (matrix, range, direction)"""
    from . import yuv
    fwd, inv, oy = yuv.tables(matrix, full_range)
    return yuv_table(inv if inverse else fwd, oy)


def _yuv_frames(what, frames, nbytes):
    """a batch of frames as the kernels take it: (B, frame_bytes) uint8 on the device, rows `stride(0)` >= frame_bytes bytes apart, bytes of a row adjacent"""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8 or frames.dim() != 2 or frames.shape[0] < 1 or \
            frames.shape[1] != nbytes or (frames.stride(1) != 1 and nbytes > 1) or (frames.shape[0] > 1 and frames.stride(0) < nbytes):
        raise ValueError("%s: frames must be a (B, %d) uint8 CUDA tensor whose rows are whole frames (unit stride inside a frame, frames at least "
                         "a frame apart), got %s" % (what, nbytes, (tuple(frames.shape), frames.stride(), frames.dtype) if isinstance(frames, torch.Tensor)
                                                     else type(frames)))
    return max(int(frames.stride(0)), nbytes) if frames.shape[0] > 1 else nbytes


def yuv_to_rgb_u8(frames, H, W, chroma, matrix="bt601", full_range=False, out=None):
    """cfen_yuv_to_rgb_u8 (include/cfen_yuv.h): B planar YCbCr frames -- the FRAME payloads of a .y4m stream as they are, (B, frame_bytes) uint8,
    rows any number >= frame_bytes of bytes apart, at any byte offset -- to (B,H,W,3) uint8 RGB.  A 1-D tensor is one frame and gives (H,W,3).
    chroma: one of yuv.CHROMA ("420jpeg", "420mpeg2", "422", "444", "mono"); matrix, full_range: the integer table of yuv.tables.  One launch,
    integer arithmetic, the same bits at every batch size, stride, alignment and stream."""
    from . import yuv
    code = yuv.chroma_code(chroma)
    single = isinstance(frames, torch.Tensor) and frames.dim() == 1
    if single:
        frames = frames[None]
    lib = _lib.load()
    nbytes = lib.cfen_yuv_frame_bytes(int(H), int(W), code)
    if nbytes == 0:
        raise ValueError("yuv_to_rgb_u8: frames of %s x %s are outside the limits (H, W in 1 .. %d)" % (H, W, yuv.MAX_EDGE))
    stride = _yuv_frames("yuv_to_rgb_u8", frames, nbytes)
    B = frames.shape[0]
    if out is not None and single:
        out = out[None]
    out = _out(out, (B, H, W, 3), torch.uint8, frames.device, "yuv_to_rgb_u8")
    check(lib.cfen_yuv_to_rgb_u8(ptr(frames), stride, B, int(H), int(W), code, _yuv_table_for(matrix, bool(full_range), True), ptr(out), current_stream()),
          "yuv_to_rgb_u8")
    return out[0] if single else out


def rgb_to_yuv_u8(rgb, chroma, matrix="bt601", full_range=False, out=None):
    """cfen_rgb_to_yuv_u8: (B,H,W,3) uint8 CUDA images to B planar YCbCr frames, (B, frame_bytes) uint8 (an (H,W,3) image gives a 1-D frame).
    out: the caller's (B, frame_bytes) tensor, rows at least a frame apart (a view into a larger buffer: the bytes between two frames are not
    written).  The counterpart of yuv_to_rgb_u8 with the forward table of yuv.tables; chroma planes are filtered from the converted bytes."""
    from . import yuv
    code = yuv.chroma_code(chroma)
    single = rgb.dim() == 3
    if single:
        rgb = rgb[None]
    _rgb_batch("rgb_to_yuv_u8", rgb=rgb)
    B, H, W, _ = rgb.shape
    lib = _lib.load()
    nbytes = lib.cfen_yuv_frame_bytes(H, W, code)
    if nbytes == 0:
        raise ValueError("rgb_to_yuv_u8: images of %d x %d are outside the limits (H, W in 1 .. %d)" % (H, W, yuv.MAX_EDGE))
    if out is None:
        out = torch.empty(B, nbytes, dtype=torch.uint8, device=rgb.device)
    elif single and out.dim() == 1:
        out = out[None]
    stride = _yuv_frames("rgb_to_yuv_u8 (out)", out, nbytes)
    if out.shape[0] != B or out.device != rgb.device:
        raise ValueError("rgb_to_yuv_u8: out holds %d frames on %s for %d images on %s" % (out.shape[0], out.device, B, rgb.device))
    check(lib.cfen_rgb_to_yuv_u8(ptr(rgb), B, H, W, code, _yuv_table_for(matrix, bool(full_range), False), ptr(out), stride, current_stream()), "rgb_to_yuv_u8")
    return out[0] if single else out


def yuv16_table(coef, oy, peak, depth):
    """a cfen_yuv16_table (include/cfen_yuv16.h) from a (3,3) integer table of yuv.tables(shift=20) and yuv.levels(depth): passed by value"""
    t = _lib.Yuv16TableC()
    flat = [int(v) for row in coef for v in row]
    if len(flat) != 9:
        raise ValueError("yuv16_table needs a 3 x 3 table, got %d entries" % len(flat))
    for k, v in enumerate(flat):
        t.coef[k] = v
    t.luma_offset, t.peak, t.depth = int(oy), int(peak), int(depth)
    return t


@functools.lru_cache(maxsize=None)
def _yuv16_table_for(matrix, full_range, depth, inverse):
    """the forward or inverse 2^-20 table of yuv.tables as a cfen_yuv16_table, built once per (matrix, range, depth, direction)"""
    from . import yuv
    fwd, inv, _ = yuv.tables(matrix, full_range, shift=yuv.DEEP_SHIFT)
    oy, peak, _ = yuv.levels(depth, full_range)
    return yuv16_table(inv if inverse else fwd, oy, peak, depth)


def _yuv16_depth(what, depth):
    from . import yuv
    return _int_arg(what, "depth", depth, yuv.MIN_DEPTH, yuv.MAX_DEPTH)


def yuv16_to_rgb_f32(frames, H, W, chroma, depth, matrix="bt601", full_range=False, out=None):
    """cfen_yuv16_to_rgb_f32 (include/cfen_yuv16.h): B planar YCbCr frames of `depth` (9 .. 16) bits per sample -- the FRAME payloads of a deep
    .y4m stream as they are, (B, frame_bytes) uint8 holding little-endian 16-bit samples, rows any even number >= frame_bytes of bytes apart, at
    an even address -- to (B,3,H,W) float32 RGB in [-1, 1], the layout the generator takes.  A 1-D tensor is one frame and gives (3,H,W).  One
    launch, 64-bit integer arithmetic and one IEEE division per value: the same bits at every batch size, stride, alignment and stream."""
    from . import yuv
    code = yuv.chroma_code(chroma)
    depth = _yuv16_depth("yuv16_to_rgb_f32", depth)
    single = isinstance(frames, torch.Tensor) and frames.dim() == 1
    if single:
        frames = frames[None]
    lib = _lib.load()
    nbytes = lib.cfen_yuv16_frame_bytes(int(H), int(W), code)
    if nbytes == 0:
        raise ValueError("yuv16_to_rgb_f32: frames of %s x %s are outside the limits (H, W in 1 .. %d)" % (H, W, yuv.MAX_EDGE))
    stride = _yuv_frames("yuv16_to_rgb_f32", frames, nbytes)
    B = frames.shape[0]
    if out is not None and single:
        out = out[None]
    out = _out(out, (B, 3, H, W), torch.float32, frames.device, "yuv16_to_rgb_f32")
    check(lib.cfen_yuv16_to_rgb_f32(ptr(frames), stride, B, int(H), int(W), code, _yuv16_table_for(matrix, bool(full_range), depth, True), ptr(out),
                                    current_stream()), "yuv16_to_rgb_f32")
    return out[0] if single else out


def rgb_f32_to_yuv16(rgb, chroma, depth, matrix="bt601", full_range=False, out=None):
    """cfen_rgb_f32_to_yuv16: (B,3,H,W) float32 CUDA images in [-1, 1] (float16 images are converted with .float(); values outside clamp, NaN is
    black) to B planar YCbCr frames of `depth` bits per sample, (B, frame_bytes) uint8 (a (3,H,W) image gives a 1-D frame).  out: the caller's
    (B, frame_bytes) tensor, rows at least a frame apart (the bytes between two frames are not written).  The floats are rounded to nearest, half
    to even; chroma planes are filtered from the converted values."""
    from . import yuv
    code = yuv.chroma_code(chroma)
    depth = _yuv16_depth("rgb_f32_to_yuv16", depth)
    single = isinstance(rgb, torch.Tensor) and rgb.dim() == 3
    if single:
        rgb = rgb[None]
    if isinstance(rgb, torch.Tensor) and rgb.dtype == torch.float16:
        rgb = rgb.float()
    _tensor_arg("rgb_f32_to_yuv16", "rgb", rgb, (None, 3, None, None), torch.float32)
    B, _, H, W = rgb.shape
    lib = _lib.load()
    nbytes = lib.cfen_yuv16_frame_bytes(H, W, code)
    if nbytes == 0:
        raise ValueError("rgb_f32_to_yuv16: images of %d x %d are outside the limits (H, W in 1 .. %d)" % (H, W, yuv.MAX_EDGE))
    if out is None:
        out = torch.empty(B, nbytes, dtype=torch.uint8, device=rgb.device)
    elif single and out.dim() == 1:
        out = out[None]
    stride = _yuv_frames("rgb_f32_to_yuv16 (out)", out, nbytes)
    if out.shape[0] != B or out.device != rgb.device:
        raise ValueError("rgb_f32_to_yuv16: out holds %d frames on %s for %d images on %s" % (out.shape[0], out.device, B, rgb.device))
    check(lib.cfen_rgb_f32_to_yuv16(ptr(rgb), B, H, W, code, _yuv16_table_for(matrix, bool(full_range), depth, False), ptr(out), stride,
                                    current_stream()), "rgb_f32_to_yuv16")
    return out[0] if single else out


def png_deflate(images, out=None, out_lengths=None, workspace=None):
    """cfen_png_deflate: contiguous (B,H,W,3) uint8 CUDA images -> (slab, lengths): slab (B, out_stride) uint8 holds image b's finished zlib
    stream (the IDAT payload of an 8-bit RGB PNG, png.assemble adds the container) in slab[b, :lengths[b]]; lengths (B,) int32.  The candidate
    Huffman tables (png.py) are uploaded once per device.  workspace: the caller's uint8 scratch of cfen_png_workspace_bytes(B, H, W) bytes (at least
    16; contents irrelevant), else allocated.  CfenError for an image wider than the encoder's strip (png.geometry)."""
    from . import png
    _cuda(images, out, out_lengths)
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8 or not images.is_contiguous():
        raise ValueError("png_deflate needs a contiguous (B,H,W,3) uint8 tensor, got %s %s" % (tuple(images.shape), images.dtype))
    B, H, W, _ = images.shape
    lib = _lib.load()
    strip, stride = ctypes.c_size_t(0), ctypes.c_size_t(0)
    nbytes = lib.cfen_png_workspace_bytes(B, H, W, ctypes.byref(strip), ctypes.byref(stride))
    tables = png.device_tables(images.device)
    workspace = _out(workspace, (max(nbytes, 16),), torch.uint8, images.device, "png_deflate (workspace)")
    if out is None:
        out = torch.empty(B, max(stride.value, 16), dtype=torch.uint8, device=images.device)
    elif nbytes and (tuple(out.shape) != (B, stride.value) or out.dtype != torch.uint8 or not out.is_contiguous()):
        raise ValueError("png_deflate: out must be a contiguous (%d, %d) uint8 CUDA tensor" % (B, stride.value))
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=torch.int32, device=images.device)
    elif tuple(out_lengths.shape) != (B,) or out_lengths.dtype != torch.int32 or not out_lengths.is_contiguous():
        raise ValueError("png_deflate: out_lengths must be a contiguous (%d,) int32 CUDA tensor" % B)
    check(lib.cfen_png_deflate(ptr(images), B, H, W, ptr(tables), tables.shape[0], ptr(workspace), ptr(out), ptr(out_lengths), current_stream()),
          "png_deflate")
    return out, out_lengths      # (workspace goes back to torch's allocator on the stream it was used on)


def u8hwc_to_nhwc(img, cs, dtype, out=None):
    """(B,H,W,3) uint8 CUDA tensor -> normalised NHWC [B,H,W,cs] of `dtype` (ToTensor + Normalize(0.5, 0.5) + layout)"""
    _cuda(img)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8 or not img.is_contiguous():
        raise ValueError("u8hwc_to_nhwc needs a contiguous (B,H,W,3) uint8 tensor")
    B, H, W, _ = img.shape
    out = _out(out, (B, H, W, cs), dtype, img.device, "u8hwc_to_nhwc")
    check(_lib.load().cfen_u8hwc_to_nhwc(dtype_code(dtype), ptr(img), ptr(out), B, H, W, cs, current_stream()), "u8hwc_to_nhwc")
    return out


def to_nhwc(x, cs=None, dtype=None):
    """NCHW torch tensor -> zero-padded NHWC (test helper; plain torch, not on the product path)."""
    B, C, H, W = x.shape
    cs = cs or round_up(C, 8)
    out = torch.zeros(B, H, W, cs, dtype=dtype or x.dtype, device=x.device)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def from_nhwc(x, C):
    return x[..., :C].permute(0, 3, 1, 2).contiguous()
