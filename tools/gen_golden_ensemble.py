#!/usr/bin/env python3
"""Writes tests/golden/ensemble_x8.npz: what the REFERENCE's Model.forward_x8 (models/vit_model.py:102-147) does to a few small images.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ensemble.py --reference <checkout of the reference project>

A generator script: it runs on the CPU, needs the reference checkout, and is not part of any test or GPU run.  forward_x8 is called unbound with a
stub `self` (precision 'single', device cpu) and a recording forward function that is not equivariant under the eight transforms and returns a
list of two outputs (tests/ensemble_ref.position_function).  Per case of ensemble_ref.CASES the fixture holds
    <case>_x            the input (1,C,T,T) float32
    <case>_variants     the eight inputs the reference handed to the forward function, in its order (8,1,C,T,T)
    <case>_ya / _yb     what the forward function returned for them (8,1,C,T,T) / (8,1,1,T,T)
    <case>_out_a / _b   the reference's float32 results
and `max_ref32_f64` = max |reference - float64 restatement| over all of them: the reference's own fp32 rounding distance."""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds models/vit_model.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ensemble_x8.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import torch
    from models.vit_model import Model
    import ensemble_ref as ref

    stub = types.SimpleNamespace(precision="single", device=torch.device("cpu"))
    data, worst = {}, 0.0
    for name, (seed, C, T) in ref.CASES.items():
        fn = ref.position_function(seed, C, T)
        x = np.random.RandomState(seed + 100).uniform(-1, 1, (1, C, T, T)).astype(np.float32)
        seen, ya, yb = [], [], []

        def recording(t):
            seen.append(t.numpy().copy())
            a, b = fn(seen[-1])
            ya.append(a)
            yb.append(b)
            return [torch.from_numpy(a), torch.from_numpy(b)]

        with torch.no_grad():
            out_a, out_b = Model.forward_x8(stub, torch.from_numpy(x), forward_function=recording)
        assert len(seen) == 8
        out_a, out_b = out_a.numpy(), out_b.numpy()
        d = max(float(np.abs(out_a - ref.merge(ya)).max()), float(np.abs(out_b - ref.merge(yb)).max()))
        order = all(np.array_equal(seen[i], ref.variant(x, i)) for i in range(8))
        print("%-8s variant order matches the restatement: %s   max |ref32 - f64| %.3e" % (name, order, d))
        worst = max(worst, d)
        data.update({name + "_x": x, name + "_variants": np.stack(seen), name + "_ya": np.stack(ya), name + "_yb": np.stack(yb),
                     name + "_out_a": out_a, name + "_out_b": out_b})
    print("max |ref32 - f64| = %.3e" % worst)
    np.savez(args.out, names=np.array(list(ref.CASES)), max_ref32_f64=np.float64(worst), **data)


if __name__ == "__main__":
    main()
