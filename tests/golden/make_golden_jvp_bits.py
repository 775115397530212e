"""Bits of the analytic-derivative passes (siren_jvp_forward_ex / siren_jvp_backward_ex), recorded at one
commit and compared at later ones (tests/test_gpu_jvp_bits.py): per case the SHA-256 of the forward
result and, after backward(cotangent), of x.grad, of every weight gradient and of every bias gradient
that is not None.

    python tests/golden/make_golden_jvp_bits.py [out.json]   # on the MI355X; default tests/golden/jvp_bits.json

The file names the commit it was recorded at (git's HEAD, or JVP_BITS_COMMIT where the tree has no .git).
The kernels have no atomics and sum their slabs in a fixed order, so the same kernels with the same
grids and arguments give the same bits: a mismatch means that an argument or a grid moved.
Shapes: cases a, b, c, d, e, f and h of make_golden_jvp_plan.py, rows capped at 300 per weight set except
case a (1000 rows: the only one with more than one row split). Every order the case admits, the default
options and each of jvp_adj / jvp_tan / jvp_tn2 at 0, and for fp32 with and without the plain forward's
saved buffer as the primal stream (y._siren_primal, as tests/test_gpu_jvp.py obtains it). Inputs come
from seeded CPU generators. Every case runs twice with fresh tensors and both runs must agree. Only
calls the package has had since the Hessian was added.
"""
import hashlib
import json
import os
import subprocess
import sys

import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
OUT = os.path.join(GOLDEN, "jvp_bits.json")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, ROOT)
from make_golden_jvp_plan import CASES, SETTINGS, admits  # noqa: E402
from make_golden_stack_sizes import setting  # noqa: E402

BITS_CASES = ("a", "b", "c", "d", "e", "f", "h")
ORDERS = (1, 2, 3, 4)
W0 = 30.0


def rows_of(case):
    return CASES[case][3] if case == "a" else min(CASES[case][3], 300)


def names(case):
    """The records of a case: "case|order|setting|own" and, for fp32, "...|primal"."""
    prec = CASES[case][0]
    return [f"{case}|{o}|{s}|{p}" for o in ORDERS if admits(case, o) for s in SETTINGS
            for p in (("own", "primal") if prec == "fp32" else ("own",))]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


_INPUTS = {}


def inputs(case):
    """x [sets or 1, rows, C], weights and biases (per set where the case has weight sets), on the device (made once)."""
    hit = _INPUTS.get(case)
    if hit is None:
        from oracle import siren_oracle as orc
        _, dims, sets, _ = CASES[case]
        rows = rows_of(case)
        g = torch.Generator().manual_seed(100 * rows + sets + len(dims))
        lead = (sets,) if sets else ()
        ws, bs = [], []
        for W, b in orc.siren_init(dims, seed=7):
            # per-set weights: the initialisation, scaled a little differently for every set
            ws.append((W * (1 + 0.05 * torch.rand(lead + (1, 1), generator=g))).contiguous())
            bs.append((b * (1 + 0.05 * torch.rand(lead + (1,), generator=g))).contiguous())
        x = torch.rand(max(sets, 1), rows, dims[0], generator=g) * 2 - 1
        dev = torch.device("cuda:0")
        hit = _INPUTS[case] = (x.to(dev), [w.to(dev) for w in ws], [b.to(dev) for b in bs])
    return hit


def cotangent(case, order, shape):
    key = (case, order)
    hit = _INPUTS.get(key)
    if hit is None:
        g = torch.Generator().manual_seed(31 * order + rows_of(case))
        hit = _INPUTS[key] = torch.randn(shape, generator=g).to(torch.device("cuda:0"))
    return hit


def run(name):
    """One forward and backward of a record's case under its setting, on fresh tensors."""
    from siren_mri_amd import _native, jvp  # noqa: F401  (jvp registers the op)
    from siren_mri_amd.ops import siren_mlp
    case, order, s, primal = name.split("|")
    order = int(order)
    prec, _, sets, _ = CASES[case]
    x0, ws0, bs0 = inputs(case)
    x = x0.clone().requires_grad_(True)
    ws = [w.clone().requires_grad_(True) for w in ws0]
    bs = [b.clone().requires_grad_(True) for b in bs0]
    with setting(s):
        p = None
        if primal == "primal":
            p = getattr(siren_mlp(x, ws, bs, w0=W0, precision="fp32"), "_siren_primal", None)
            assert p is not None
        out, _ = torch.ops.siren_mri_amd.sine_mlp_jvp(x, ws, bs, W0, _native.PRECISIONS[prec], bool(sets), order, True, p)
        out.backward(cotangent(case, order, out.shape))
    return {"out": sha(out), "dx": sha(x.grad), "dW": [sha(w.grad) for w in ws],
            "db": [sha(b.grad) for b in bs if b.grad is not None]}


def pack(rec):
    """The records as jvp_bits.json keeps them: every distinct digest once, in "digests" (many records share
    most of theirs: a setting moves one kernel), and per record the digests' indices."""
    table = sorted({h for r in rec.values() for h in [r["out"], r["dx"], *r["dW"], *r["db"]]})
    at = {h: i for i, h in enumerate(table)}
    return {"digests": table, "cases": {n: {"out": at[r["out"]], "dx": at[r["dx"]], "dW": [at[h] for h in r["dW"]],
                                            "db": [at[h] for h in r["db"]]} for n, r in rec.items()}}


def unpack(doc):
    """jvp_bits.json as {"commit", "cases": name -> the record run() returns}."""
    t = doc["digests"]
    return {"commit": doc["commit"], "cases": {n: {"out": t[r["out"]], "dx": t[r["dx"]], "dW": [t[i] for i in r["dW"]],
                                                   "db": [t[i] for i in r["db"]]} for n, r in doc["cases"].items()}}


def load(path=OUT):
    with open(path) as f:
        return unpack(json.load(f))


def dump(commit, rec, path):
    doc = dict(pack(rec), commit=commit)
    assert unpack(doc)["cases"] == rec  # nothing lost in packing
    row = lambda v: json.dumps(v, sort_keys=True)  # noqa: E731
    with open(path, "w") as f:
        f.write('{\n "commit": %s,\n "digests": [\n  ' % row(commit) + ",\n  ".join(row(h) for h in doc["digests"]) + "\n ],\n")
        f.write(' "cases": {\n  ' + ",\n  ".join(f"{row(n)}: {row(r)}" for n, r in sorted(doc["cases"].items())) + "\n }\n}\n")


def main():
    rec = {}
    for case in BITS_CASES:
        for name in names(case):
            first, second = run(name), run(name)
            if first != second:
                raise SystemExit(f"{name}: two runs with fresh tensors differ: {first} / {second}")
            rec[name] = first
        print(case, len(names(case)), "records")
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    dump(os.environ.get("JVP_BITS_COMMIT") or commit, rec, path)
    print(f"wrote {path}: {len(rec)} records")


if __name__ == "__main__":
    main()
