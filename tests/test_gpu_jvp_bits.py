"""GPU: the analytic-derivative passes (siren_jvp_forward_ex / siren_jvp_backward_ex) give the bits recorded
in tests/golden/jvp_bits.json at the commit the file names: the SHA-256 of the forward result and, after
backward(cotangent), of x.grad and of every weight and bias gradient. Equality, not a tolerance: the
kernels have no atomics and sum their slabs in a fixed order, so a mismatch means that a launch's grid or
an argument moved. Every record runs twice with fresh tensors and both runs must match. Cases, orders,
settings and inputs: tests/golden/make_golden_jvp_bits.py."""
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_jvp_bits import BITS_CASES, ORDERS, load, names, rows_of, run  # noqa: E402
from make_golden_jvp_plan import CASES, SETTINGS  # noqa: E402

pytestmark = pytest.mark.gpu
BITS = load()  # (the file keeps each distinct digest once: make_golden_jvp_bits.unpack)


def test_fixture_covers_the_cases():
    assert BITS_CASES == ("a", "b", "c", "d", "e", "f", "h") and ORDERS == (1, 2, 3, 4)
    assert sorted(BITS["cases"]) == sorted(n for c in BITS_CASES for n in names(c))
    assert len(BITS["commit"]) == 40
    assert [rows_of(c) for c in BITS_CASES] == [1000, 128, 300, 300, 300, 300, 129]
    # every order but the Hessian of case d's four inputs, the four settings, fp32 with and without a primal
    for c in BITS_CASES:
        fp32 = CASES[c][0] == "fp32"
        assert len(names(c)) == (3 if c == "d" else 4) * len(SETTINGS) * (2 if fp32 else 1)
        assert any(n.endswith("|primal") for n in names(c)) == fp32


@pytest.mark.parametrize("case", BITS_CASES)
def test_jvp_bits(case):
    for name in names(case):
        want = BITS["cases"][name]
        assert run(name) == want, name
        assert run(name) == want, name + " (second run)"
