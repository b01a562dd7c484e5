"""numpy float64 restatement of the geometric self-ensemble (cfen_vit_dehazing_amd/ensemble.py; the reference's Model.forward_x8,
models/vit_model.py:102-147), for the tests.

Per (..., T, T) plane, with v = flip W, h = flip H, t = swap H and W:
    variant i = b0 + 2 b1 + 4 b2:  x_i = t^b2(h^b1(v^b0(x)))      (v applied first)
    mapped back:                   z_i = v^b0(h^b1(t^b2(y_i)))
    result:                        (z_0 + z_1 + ... + z_7) / 8      summed in increasing i
"""
import numpy as np

OPS = {"v": lambda a: a[..., ::-1], "h": lambda a: a[..., ::-1, :], "t": lambda a: np.swapaxes(a, -1, -2)}


def bits(i):
    return i & 1, (i >> 1) & 1, (i >> 2) & 1


def variant(x, i):
    """x_i"""
    b0, b1, b2 = bits(i)
    for on, op in ((b0, "v"), (b1, "h"), (b2, "t")):
        if on:
            x = OPS[op](x)
    return np.ascontiguousarray(x)


def variants(x):
    return np.stack([variant(x, i) for i in range(8)])


def back(y, i):
    """z_i of y_i"""
    b0, b1, b2 = bits(i)
    for on, op in ((b2, "t"), (b1, "h"), (b0, "v")):
        if on:
            y = OPS[op](y)
    return np.ascontiguousarray(y)


def merge(ys):
    """ys: the eight outputs y_0 .. y_7 (any dtype) -> float64 ensemble"""
    acc = back(np.asarray(ys[0], dtype=np.float64), 0)
    for i in range(1, 8):
        acc = acc + back(np.asarray(ys[i], dtype=np.float64), i)
    return acc * 0.125


def merge_f32(ys):
    """the same sum carried in float32, as the device carries it"""
    acc = back(np.asarray(ys[0], dtype=np.float32), 0)
    for i in range(1, 8):
        acc = acc + back(np.asarray(ys[i], dtype=np.float32), i)
    return acc * np.float32(0.125)


def transform(x, g):
    """one of the 8 transforms applied to an image (the same group elements as the variants)"""
    return variant(x, g)


def position_function(seed, C, T):
    """a seeded function of a (1,C,T,T) float32 image that is NOT equivariant under the eight transforms (position-dependent weights, as the
    generator's positional tables are) and returns two outputs, (1,C,T,T) and (1,1,T,T), with values in [-1,1]; float32 numpy throughout"""
    rs = np.random.RandomState(seed)
    wa, wb, wc = (rs.uniform(-1, 1, (1, c, T, T)).astype(np.float32) for c in (C, C, 1))

    def fn(x):
        x = np.asarray(x, dtype=np.float32)
        a = np.float32(0.5) * x * wa + np.float32(0.4) * wb
        b = np.float32(0.6) * x.mean(axis=1, keepdims=True, dtype=np.float32) * wc + np.float32(0.3) * np.roll(wc, 1, axis=-1)
        return [a.astype(np.float32), b.astype(np.float32)]
    return fn


CASES = {"c3_t8": (11, 3, 8), "c3_t16": (12, 3, 16), "c1_t12": (13, 1, 12)}
