"""The analytic-derivative passes' buffer sizes and launch plans (siren_jvp_plan) over a grid of small
shapes, orders, flags and option settings, against the recorded ones (tests/golden/jvp_plan.json: the
sizes of the library, and the plans transcribed from its launch code, before the passes became a plan).
CPU only: the library sizes buffers and plans launches without a device."""
import ctypes
import os
import re
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_golden_jvp_plan import (BF16_PRIMAL, CASES, FLAGS, ORDERS, SETTINGS, Shape, admits, describe, keys, load,  # noqa: E402
                                  parent_layout, plan_text, sizes)
from make_golden_stack_sizes import setting  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

PLAN = load()  # (the file keeps each distinct line once: make_golden_jvp_plan.unpack)
LINE = re.compile(r"^(fwd|bwd) (siren::\w+(<[\w, ]+>)?) layer=(\d+) cur=([01]) grid=\((\d+),(\d+),(\d+)\) block=(256|512)"
                  r"( slab=part nsplit=(\d+))?$")


def test_golden_file_covers_the_grid():
    assert PLAN["cases"] == {k: {"precision": v[0], "dims": v[1], "weight_sets": v[2], "rows": v[3]}
                             for k, v in CASES.items()}
    assert sorted(CASES) == list("abcdefghij") and ORDERS == (1, 2, 3, 4)
    assert PLAN["settings"] == list(SETTINGS) == ["default", "jvp_adj=0", "jvp_tan=0", "jvp_tn2=0"]
    assert FLAGS == {"fp32": (0, 1, 2, 3), "bf16": (0, 1)}
    assert set(PLAN["sizes"]) == {f"{c}|{o}|{s}" for c in CASES for o in ORDERS for s in SETTINGS}
    assert set(PLAN["plans"]) | set(PLAN["refused"]) == set(keys())
    # refused: the Hessian of case d's four inputs, and the one bf16 entry with a primal buffer
    assert set(PLAN["refused"]) == {k for k in keys() if k.startswith("d|4|")} | {BF16_PRIMAL}
    assert all(PLAN["sizes"][f"d|4|{s}"] == [-1, -1] for s in SETTINGS)


@pytest.mark.parametrize("case", sorted(CASES))
def test_sizes_and_plans_are_the_recorded_ones(case):
    d = describe(case)
    for key in (k for k in keys() if k.startswith(case + "|")):
        _, order, s, flags = key.split("|")
        with setting(s):
            assert sizes(d, int(order)) == PLAN["sizes"][f"{case}|{order}|{s}"], key
            text = plan_text(d, int(order), int(flags))
            if key in PLAN["refused"]:
                assert text is None and _native.last_error() == PLAN["refused"][key], key
            else:
                assert text == PLAN["plans"][key], key


def test_plan_lines_are_well_formed_and_in_bounds():
    """Every line is a launch with a grid inside the device's limits, the header counts the lines of
    each pass, and the slabs a launch writes (or a reduce launch sums) fit the workspace's slab region."""
    for key, text in PLAN["plans"].items():
        case, order, s, flags = key.split("|")
        head, *lines = text.splitlines()
        g = Shape(case, int(order))
        m = re.match(r"^# order=([1-4]) prec=(fp32|bf16) flags=([0-3]) streams=(\d+) fwd=(\d+) bwd=(\d+)$", head)
        assert m, (key, head)
        assert (m.group(1), m.group(2), m.group(3), int(m.group(4))) == (order, g.prec, flags, g.S), (key, head)
        assert int(m.group(5)) == sum(ln.startswith("fwd ") for ln in lines), key
        assert int(m.group(6)) == sum(ln.startswith("bwd ") for ln in lines), key
        assert [ln[:3] for ln in lines] == ["fwd"] * int(m.group(5)) + ["bwd"] * int(m.group(6)), key
        # the slab region: from the transcription's offset of `part` to the end of the recorded workspace
        # (which is the workspace proper followed by room for the saved tensors)
        saved_bytes, ws_bytes = PLAN["sizes"][f"{case}|{order}|{s}"]
        region = ws_bytes - saved_bytes - parent_layout(case, int(order))["part_off"]
        for line in lines:
            lm = LINE.match(line)
            assert lm, (key, line)
            gx, gy, gz = (int(lm.group(i)) for i in (6, 7, 8))
            assert 1 <= gx < 2 ** 31 and 1 <= gy <= 65535 and 1 <= gz <= 65535, (key, line)
            assert int(lm.group(4)) < g.L
            if lm.group(10) is not None:
                assert lm.group(1) == "bwd"
                assert 4 * int(lm.group(11)) * g.split_stride(g.slab(int(lm.group(4)))) <= region, (key, line)


def test_every_kernel_form_occurs():
    """Each template form the planner's tables list is in at least one recorded plan."""
    text = "\n".join(PLAN["plans"].values())
    forms = [f"jvp_tan_kernel<0, {c}>" for c in (1, 2, 3, 4)]
    forms += ["jvp_tn2_kernel<true>", "jvp_tn2_kernel<false>"]
    for p in (0, 1):
        forms += [f"jvp_adj_kernel<{p}, {sl}>" for sl in ("2, false", "3, false", "3, true", "4, false", "4, true")]
        forms += [f"jvp_nt_kernel<{p}, JMODE_FWD{f}>" for f in ("", ", true", ", false, true")]
        forms += [f"jvp_nt_kernel<{p}, JMODE_BWD>"]
        forms += [f"jvp_tn_kernel<{p}{f}>" for f in ("", ", true", ", false, true")]
        forms += [f"jvp_last_kernel<{p}>"] + [f"jvp_last_hess_kernel<{p}, {c}>" for c in (1, 2, 3)]
        forms += [f"jvp_combine_kernel<{p}>", f"jvp_combine_jac_kernel<{p}>"]
        forms += [f"jvp_hess_combine_kernel<{p}, {c}, {t}>" for c in (1, 2, 3) for t in ("true", "false")]
        forms += [f"jvp_first_kernel<{p}>", f"jvp_first_bwd_kernel<{p}>", f"jvp_first_dx_kernel<{p}>"]
    missing = [f for f in forms if f" siren::{f} " not in text]
    assert not missing, missing
    assert " siren::reduce_kernel " in text
    # and no other: the library's tables list nothing that the grid does not reach
    assert set(re.findall(r" siren::(\w+(?:<[\w, ]+>)?) ", text)) == set(forms) | {"reduce_kernel"}


def test_plan_entry_point_contract():
    lib = _native.load_library()
    d = describe("a")
    n = lib.siren_jvp_plan(ctypes.byref(d), 1, 3, None, 0)
    assert n == len(PLAN["plans"]["a|1|default|3"]) + 1
    buf = ctypes.create_string_buffer(16)  # too small: truncated and terminated, the need is still returned
    assert lib.siren_jvp_plan(ctypes.byref(d), 1, 3, buf, 16) == n
    assert buf.raw[15] == 0 and len(buf.value) == 15 and plan_text(d, 1, 3).startswith(buf.value.decode())
    assert not admits("d", 4)
    assert lib.siren_jvp_plan(ctypes.byref(describe("d")), 4, 0, None, 0) == -1
    assert "in_features <= 3" in _native.last_error()
    assert lib.siren_jvp_plan(ctypes.byref(describe("e")), 1, 2, None, 0) == -1
    assert "jvp primal: fp32 mode only" in _native.last_error()
    sine_out = _native.describe_only([2, 64, 64, 1], prec=_native.PREC_F32, rows_per_batch=64, outermost_linear=False)
    assert lib.siren_jvp_plan(ctypes.byref(sine_out), 1, 2, None, 0) == -1
    assert "outermost_linear" in _native.last_error()
    assert lib.siren_jvp_plan(ctypes.byref(d), 5, 0, None, 0) == -1
    assert "derivative mode 5" in _native.last_error()
    bad = _native.describe_only([2, 100, 1], prec=_native.PREC_F32, rows_per_batch=64)
    assert lib.siren_jvp_plan(ctypes.byref(bad), 1, 0, None, 0) == -1
    assert "hidden width" in _native.last_error()
