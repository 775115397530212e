"""Buffer sizes of the SIREN stack over a grid of small shapes and option settings (CPU only: the
library sizes buffers without a device):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stack_sizes.py

  stack_sizes.json  "cases": the shapes (precision, dims, weight sets, rows per weight set); "settings":
                    the option settings, each one option moved off its default (or none); "sizes": per
                    case and setting, [siren_mlp_saved_bytes, siren_mlp_workspace_bytes].
The file pins what a rewrite of the launch code must not move (tests/test_stack_plan.py asserts
equality), so it is written by the commit BEFORE such a rewrite and committed unchanged.
tests/golden/stack_plan.json (the backward launch plans of the same grid) uses the same cases and
setting names.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from siren_mri_amd import _native  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

# name -> (precision, dims, weight sets (0: shared weights), rows per weight set)
CASES = {
    "a": ("bf16", [2, 256, 256, 256, 256, 1], 0, 4096),
    "b": ("bf16", [2, 256, 256, 1], 0, 1000),
    "c": ("bf16", [2, 256, 256, 256, 1], 0, 333),
    "d": ("bf16", [3, 128, 128, 128, 2], 0, 640),
    "e": ("bf16", [16, 256, 256, 256, 2], 3, 500),
    "f": ("bf16", [120, 256, 256, 256, 2], 2, 512),
    "g": ("bf16", [2, 256, 256, 256, 256, 2], 65, 64),
    "h": ("bf16", [2, 512, 512, 1], 0, 300),
    "i": ("fp32", [2, 256, 256, 256, 1], 0, 1000),
    "j": ("fp32", [2, 64, 64, 2], 0, 129),
}
SETTINGS = ("default", "pair_ring=0", "dx_ring=0", "dw_ring=0", "fused_backward=0", "fuse_output_layer=1",
            "ring_output_fusion=0", "pair_tail_reduce=0", "debug_keep_p0=1", "f32_rows=0")


def describe(case):
    prec, dims, sets, rows = CASES[case]
    return _native.describe_only(dims, prec=_native.PRECISIONS[prec], weights_batched=sets > 0, batch=max(sets, 1),
                                 rows_per_batch=rows)


class setting:
    """Context manager: one option moved off its default ("default": none)."""

    def __init__(self, name):
        self.key, self.value = (name.split("=") + [None])[:2] if name != "default" else (None, None)

    def __enter__(self):
        if self.key:
            self.old = _native.get_option(self.key)
            _native.set_option(self.key, int(self.value))

    def __exit__(self, *exc):
        if self.key:
            _native.set_option(self.key, self.old)
        return False


def main():
    lib = _native.load_library()
    sizes = {}
    for case in CASES:
        d = describe(case)
        sizes[case] = {}
        for s in SETTINGS:
            with setting(s):
                assert lib.siren_mlp_check(ctypes.byref(d)) == 0, (case, s, _native.last_error())
                sizes[case][s] = [int(lib.siren_mlp_saved_bytes(ctypes.byref(d))),
                                  int(lib.siren_mlp_workspace_bytes(ctypes.byref(d)))]
    doc = {"cases": {k: {"precision": v[0], "dims": v[1], "weight_sets": v[2], "rows": v[3]} for k, v in CASES.items()},
           "settings": list(SETTINGS), "sizes": sizes}
    with open(os.path.join(OUT, "stack_sizes.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote stack_sizes.json:", sum(len(v) for v in sizes.values()), "entries")


if __name__ == "__main__":
    main()
