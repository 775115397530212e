"""What the backward plan says, what the library launches and what the library launched before the
backward became a plan agree: per case of tests/golden/stack_plan.json, the launches of every kernel
class in one forward + backward (counted by _native.KernelTimer) are the recorded ones, and the
backward classes are the ones the plan text names."""
import json
import os
import sys

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_stack_plan import FORWARD_CLASSES, GPU_SETTINGS, GPU_VARIANTS, plan_class_counts, plan_text  # noqa: E402
from make_golden_stack_sizes import CASES, describe, setting  # noqa: E402
from siren_mri_amd import _native  # noqa: E402
from siren_mri_amd.ops import siren_mlp  # noqa: E402

pytestmark = pytest.mark.gpu
PLAN = json.load(open(os.path.join(GOLDEN, "stack_plan.json")))


def measured_class_counts(case, flags):
    """Launches per kernel class 1..14 of one forward + backward (flags as siren_mlp_backward_plan's;
    dy comes from autograd and is always aligned)."""
    dev = torch.device("cuda:0")
    prec, dims, sets, rows = CASES[case]
    g = torch.Generator().manual_seed(1)
    lead = (sets,) if sets else ()
    ws = [((torch.rand(lead + (dims[l + 1], dims[l]), generator=g) - 0.5) * 0.1).to(dev).requires_grad_(True)
          for l in range(len(dims) - 1)]
    bs = [((torch.rand(lead + (dims[l + 1],), generator=g) - 0.5) * 0.1).to(dev).requires_grad_(True)
          for l in range(len(dims) - 1)]
    n = max(sets, 1) * rows * dims[0]
    off = 0 if flags & 2 else 2  # x starts 8 bytes past a 16-byte boundary
    x = (torch.rand(n + 2, generator=g) * 2 - 1).to(dev)[off:off + n].view(lead + (rows, dims[0]))
    assert (x.data_ptr() % 16 == 0) == bool(flags & 2)
    x.requires_grad_(bool(flags & 1))
    counts = {}
    for k in range(1, 15):
        with _native.KernelTimer(k) as kt:
            siren_mlp(x, ws, bs, w0=30.0, precision=prec).sum().backward()
            torch.cuda.synchronize()
        if kt.launches:
            counts[str(k)] = int(kt.launches)
    return counts


@pytest.mark.parametrize("case,flags", [(c, f) for c in sorted(CASES) for f in GPU_VARIANTS[c]])
def test_launches_are_the_recorded_and_the_planned_ones(case, flags):
    assert flags & 4
    for s in GPU_SETTINGS:
        key = f"{case}|{s}|{flags}"
        with setting(s):
            got = measured_class_counts(case, flags)
            planned = plan_class_counts(plan_text(describe(case), flags))
        assert got == PLAN["class_counts"][key], key
        assert {k: v for k, v in got.items() if int(k) not in FORWARD_CLASSES} == planned, key
        assert planned == plan_class_counts(PLAN["plans"][key]), key
