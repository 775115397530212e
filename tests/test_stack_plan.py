"""The stack's buffer sizes and its backward launch plan over a grid of small shapes and option
settings, against the recorded ones (tests/golden/stack_sizes.json, stack_plan.json). CPU only: the
library sizes buffers and plans launches without a device."""
import ctypes
import json
import os
import re
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_stack_plan import (FORWARD_CLASSES, GPU_SETTINGS, GPU_VARIANTS, VARIANTS, plan_class_counts,  # noqa: E402
                                    plan_text)
from make_golden_stack_sizes import CASES, SETTINGS, describe, setting  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

SIZES = json.load(open(os.path.join(GOLDEN, "stack_sizes.json")))
PLAN = json.load(open(os.path.join(GOLDEN, "stack_plan.json")))


def test_golden_files_cover_the_grid():
    assert SIZES["cases"] == {k: {"precision": v[0], "dims": v[1], "weight_sets": v[2], "rows": v[3]}
                              for k, v in CASES.items()}
    assert SIZES["settings"] == list(SETTINGS) and len(SETTINGS) == 10
    assert PLAN["variants"] == VARIANTS
    assert set(PLAN["plans"]) == {f"{c}|{s}|{f}" for c in CASES for s in SETTINGS for f in VARIANTS[c]}


@pytest.mark.parametrize("case", sorted(CASES))
def test_buffer_sizes_are_the_recorded_ones(case):
    lib = _native.load_library()
    d = describe(case)
    for s in SETTINGS:
        with setting(s):
            got = [lib.siren_mlp_saved_bytes(ctypes.byref(d)), lib.siren_mlp_workspace_bytes(ctypes.byref(d))]
        assert got == SIZES["sizes"][case][s], (case, s)


@pytest.mark.parametrize("case", sorted(CASES))
def test_backward_plan_is_the_recorded_one(case):
    d = describe(case)
    for s in SETTINGS:
        with setting(s):
            for flags in VARIANTS[case]:
                assert plan_text(d, flags) == PLAN["plans"][f"{case}|{s}|{flags}"], (case, s, flags)


def test_recorded_plans_name_the_measured_launches():
    """The launches per backward kernel class that a recorded plan names are the ones counted on the
    GPU before the backward became a plan (forward classes are not part of a backward plan)."""
    assert set(PLAN["class_counts"]) == {f"{c}|{s}|{f}" for c in CASES for s in GPU_SETTINGS for f in GPU_VARIANTS[c]}
    for key, counts in PLAN["class_counts"].items():
        backward = {k: n for k, n in counts.items() if int(k) not in FORWARD_CLASSES}
        assert plan_class_counts(PLAN["plans"][key]) == backward, key


def test_plan_lines_are_well_formed_and_in_bounds():
    """Every line is a launch with a grid inside the device's limits, and a launch that writes slabs
    says where they are summed; the header counts the lines."""
    pat = re.compile(r"^(siren::\w+(<[\w, ]+>)?) class=(\d+) layer=(\d+) grid=\((\d+),(\d+),(\d+)\) block=(256|512)"
                     r"( slab=(part|part2|partL|partB)(\+(partL|partB))? nsplit=\d+(\+\d+)?)?( p_vec=[01])?"
                     r"( reduce=(own|next_pair|flush))?$")
    for key, text in PLAN["plans"].items():
        head, *lines = text.splitlines()
        m = re.match(r"^# out=(last_bwd|tiled|ring) first=(ring|tiled|mfma|valu) xcopy=([01]) launches=(\d+)$", head)
        assert m, (key, head)
        assert int(m.group(4)) == len(lines)
        for line in lines:
            if line.startswith("hipMemcpyAsync "):
                assert m.group(3) == "1" and line == "hipMemcpyAsync class=0 layer=0 grid=(0,0,0) block=0", (key, line)
                continue
            lm = pat.match(line)
            assert lm, (key, line)
            gx, gy, gz = (int(lm.group(i)) for i in (5, 6, 7))
            assert 1 <= gx < 2 ** 31 and 1 <= gy <= 65535 and 1 <= gz <= 65535, (key, line)
            writes = lm.group(9) is not None and "reduce_" not in lm.group(1)
            assert writes == (lm.group(15) is not None), (key, line)
            assert (lm.group(14) is not None) == ("tn_dw_kernel<" in line and ", true, false>" in line), (key, line)


def test_every_form_of_the_plan_occurs():
    """Each output-layer and first-layer form, slab buffer, reduction place and kind of launch is in
    at least one recorded plan."""
    text = "\n".join(PLAN["plans"].values())
    for word in ("out=last_bwd", "out=tiled", "out=ring", "first=ring", "first=tiled", "first=mfma", "first=valu",
                 "xcopy=1", "slab=part ", "slab=part2 ", "slab=part+partL", "slab=part+partB", "slab=partL ",
                 "p_vec=0", "p_vec=1", "reduce=own", "reduce=next_pair", "reduce=flush"):
        assert word in text, word
    for kernel in (r"hipMemcpyAsync", r"last_bwd_kernel<[01], 1, 2>", r"reduce_kernel", r"reduce_multi_kernel",
                   r"pair_ring_bf16_kernel<0, false, false, 0, 0>", r"pair_ring_bf16_kernel<0, false, false, [12], 0>",
                   r"pair_ring_bf16_kernel<2, (true|false), true, 0, 2>",
                   r"tn_dw_kernel<0, false, false>", r"tn_dw_kernel<1, false, false>", r"tn_dw_kernel<1, false, true>",
                   r"dw_ring_bf16_kernel<0, 0>", r"dw_ring_bf16_kernel<0, [12]>", r"dw_ring_bf16_kernel<2, 0>",
                   r"jvp_tn2_kernel<false>", r"tn_dw_kernel<1, true, false>",
                   r"nt_bf16_kernel<1, 256, false, false>", r"nt_bf16_kernel<1, 512, false, false>",
                   r"nt_bf16_kernel<1, 256, true, false>", r"nt_bf16_kernel<1, 256, false, true>", r"nt_f32_kernel<1, 256>",
                   r"dx_ring_bf16_kernel<0, false, false, 0>", r"dx_ring_bf16_kernel<0, false, false, [12]>",
                   r"dx_ring_bf16_kernel<2, true, true, 0>", r"dx_ring_bf16_kernel<2, false, false, 0>",
                   r"jvp_tan_kernel<0, 2, 2>", r"nt_bf16_kernel<3, 256, false, false>",
                   r"first_bwd_kernel<[01], [12], 4>", r"first_bwd_wide_mfma_kernel", r"first_dx_wide_kernel"):
        assert re.search(r"siren::" + kernel + " |^" + kernel + " ", text, re.M), kernel


def test_plan_entry_point_contract():
    lib = _native.load_library()
    d = describe("a")
    n = lib.siren_mlp_backward_plan(ctypes.byref(d), 7, None, 0)
    buf = ctypes.create_string_buffer(16)  # too small: truncated and terminated, the need is still returned
    assert lib.siren_mlp_backward_plan(ctypes.byref(d), 7, buf, 16) == n
    assert buf.raw[15] == 0 and plan_text(d, 7).startswith(buf.value.decode())
    bad = _native.describe_only([2, 100, 1], prec=_native.PREC_BF16, rows_per_batch=64)
    assert lib.siren_mlp_backward_plan(ctypes.byref(bad), 7, None, 0) == -1
    assert "hidden width" in _native.last_error()
