"""GPU: every loss that ends in the inter-workgroup hand-off of a deterministic sum (siren_common.h
block_sum_handoff / handoff_publish) gives the bits recorded in tests/golden/loss_bits.json — the loss
as float32 and the SHA-256 of the gradient (the fused forward losses: of dL/dy and DC(y)) — at the
commit the file names. A changed order of summation anywhere shows here. Each case runs twice in a row
with fresh output tensors and both runs must match: the second shows that the first re-armed the
hand-off's counter. Cases and inputs: tests/golden/make_golden_loss_bits.py."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_loss_bits import FUSED_CASES, cases, fused_grid  # noqa: E402

pytestmark = pytest.mark.gpu
BITS = json.load(open(os.path.join(GOLDEN, "loss_bits.json")))
CASES = cases()


def test_fixture_covers_the_cases():
    assert sorted(BITS["cases"]) == sorted(CASES)
    assert len(BITS["commit"]) == 40
    # the fused forwards' grids: a few workgroups, more than the register forward's 512 threads, more
    # than the per-layer output kernel's 256
    assert [fused_grid(n) for n in FUSED_CASES] == [2, 520, 300]


@pytest.mark.parametrize("name", sorted(CASES))
def test_loss_bits(name):
    want = BITS["cases"][name]
    first = CASES[name]()
    second = CASES[name]()
    print(f"\n[loss bits] {name}: want {want['loss']}, got {first['loss']} then {second['loss']}")
    assert first == want
    assert second == want
