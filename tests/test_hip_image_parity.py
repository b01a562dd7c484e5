"""The image-side entry points against tests/golden/image_parity.npz, bit for bit and with no tolerance.  The fixture holds what the library gave
BEFORE the shared code of these kernels moved into csrc/cfen_image.hpp (tools/gen_golden_image_parity.py, which also defines the cases and runs
them here): the apply kernel of k_guided / k_temporal, the fixed-order fp64 reductions of the scores and the byte rounding are each written once
now, and a change there that moves a single bit of any kernel's result fails here.  The fixture is not regenerated from the code under test."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_golden_image_parity as parity  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(parity.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_exactly_the_cases(golden):
    assert {k.rsplit("/", 1)[0] for k in golden} == set(parity.CASES)


@pytest.mark.parametrize("name", list(parity.CASES))
def test_same_bits_as_before_the_shared_header(name, golden):
    got = parity.CASES[name]()
    assert {name + "/" + k for k in got} == {k for k in golden if k.rsplit("/", 1)[0] == name}
    for k, v in got.items():
        want = golden[name + "/" + k]
        assert parity.same_bits(parity.packed(v), want), "%s/%s: %s %s %s differs from the fixture (%s)" % (
            name, k, v.dtype, v.shape, "as SHA-256" if v.nbytes > parity.WHOLE_BYTES else v.ravel()[:8], want.ravel()[:8])
