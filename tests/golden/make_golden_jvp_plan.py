"""Buffer sizes and launch plans of the analytic-derivative passes (siren_jvp_*) over a grid of small
shapes, orders, flags and option settings (CPU only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jvp_plan.py

  jvp_plan.json  as load() returns it: "cases": the shapes; "settings"; "sizes": per "case|order|setting",
                 [siren_jvp_saved_bytes, siren_jvp_workspace_bytes] of the library at the commit BEFORE the
                 passes became a plan (-1 where it refuses the shape); "plans": the plan text per
                 "case|order|setting|flags" (flags of siren_jvp_plan: bit 0 an input gradient is wanted,
                 bit 1 a primal buffer is given); "refused": the error message of the entries the library
                 refuses (the Hessian of four inputs; a primal buffer in bf16 mode), from that library too.
                 The file keeps every distinct launch line once (pack / unpack).
The plan texts do NOT come from the library. parent_forward() / parent_backward() below are a
transcription, statement by statement, of jvp_forward_impl / jvp_backward_impl and of jlayout_of, jtn_split,
jcol_split, jtn2_split, jvp_adj_fused, jvp_tn2_ok, grid1d and reduce_blocks of siren_mri_amd/csrc as they
stood at commit 8849abc, before the plan existed: the same conditions in the same order, with a text
line where that code launched a kernel. They read the options through siren_config_get and nothing else
from the library. The library's sizes and texts are only compared with them (here, as a check before
writing where the library has siren_jvp_plan, and in tests/test_jvp_plan.py).
The file pins what a rewrite of the launch code must not move, so it is committed unchanged.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_stack_sizes import OUT, setting  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

# name -> (precision, dims, weight sets (0: shared weights), rows per weight set)
CASES = {
    "a": ("fp32", [2, 256, 256, 256, 1], 0, 1000),  # jvp_tn2, the fused adjoint, row-stacked tangents with a primal
    "b": ("fp32", [1, 128, 128, 1], 0, 128),        # one input; 128x128 weight-gradient tiles; jvp_adj_kernel<., 3, true>
    "c": ("fp32", [3, 64, 128, 64, 2], 2, 512),     # batched weights, two outputs, six pair streams
    "d": ("fp32", [4, 256, 256, 1], 0, 333),        # five streams: the two-launch adjoint; no Hessian
    "e": ("bf16", [2, 256, 256, 256, 1], 0, 1000),
    "f": ("bf16", [3, 128, 128, 2], 3, 300),
    "g": ("bf16", [2, 512, 512, 1], 0, 300),        # a layer below wider than JADJ_BN: two-launch adjoint, two column tiles
    "h": ("fp32", [2, 64, 64, 2], 0, 129),
    "i": ("fp32", [2, 256, 1], 0, 200),             # no hidden GEMM layer
    "j": ("bf16", [1, 128, 128, 1], 0, 128),        # b in bf16: the one-input bf16 forms, which a..i do not reach
}
ORDERS = (1, 2, 3, 4)  # SIREN_JVP_GRADIENT, _LAPLACE, _JACOBIAN, _HESSIAN
SETTINGS = ("default", "jvp_adj=0", "jvp_tan=0", "jvp_tn2=0")
FLAGS = {"fp32": (0, 1, 2, 3), "bf16": (0, 1)}
BF16_PRIMAL = "e|1|default|2"  # the one bf16 entry with a primal buffer: refused


def describe(case):
    prec, dims, sets, rows = CASES[case]
    return _native.describe_only(dims, prec=_native.PRECISIONS[prec], weights_batched=sets > 0, batch=max(sets, 1),
                                 rows_per_batch=rows)


def admits(case, order):
    """jvp_check: the Hessian carries at most three inputs."""
    return not (order == 4 and CASES[case][1][0] > 3)


def keys():
    out = [f"{c}|{o}|{s}|{f}" for c, v in CASES.items() for o in ORDERS for s in SETTINGS for f in FLAGS[v[0]]]
    return out + [BF16_PRIMAL]


def sizes(desc, order):
    lib = _native.load_library()
    return [int(lib.siren_jvp_saved_bytes(ctypes.byref(desc), order)),
            int(lib.siren_jvp_workspace_bytes(ctypes.byref(desc), order))]


def plan_text(desc, order, flags):
    """siren_jvp_plan's text, or None where it refuses (the message is then _native.last_error())."""
    lib = _native.load_library()
    n = lib.siren_jvp_plan(ctypes.byref(desc), order, flags, None, 0)
    if n < 0:
        return None
    buf = ctypes.create_string_buffer(n)
    assert lib.siren_jvp_plan(ctypes.byref(desc), order, flags, buf, n) == n
    return buf.value.decode()


# ------------------------------------------------------------------ the parent's launch code, transcribed
def cdiv(a, b):
    return (a + b - 1) // b


def align_up(v, a):
    return cdiv(v, a) * a


def split_rows(rows, blocks_per_split, nb, granule):  # kTargetBlocks = 1024
    want = max(1, 1024 // max(1, blocks_per_split * nb))
    rps = max(align_up(cdiv(rows, want), granule), granule)
    return max(1, cdiv(rows, rps)), rps  # (nsplit, rows_per_split)


def grid1d(work, cap=4096):
    return max(1, min(cdiv(work, 256), cap))


def reduce_blocks(nb, slab):
    return cdiv(nb * slab, 128)


class Shape:
    """geo_of and the constants both passes read."""

    def __init__(self, case, order):
        self.prec, self.dims, sets, rows_per_set = CASES[case]
        self.bf16 = self.prec == "bf16"
        self.P = 1 if self.bf16 else 0  # kPrecBF16 / kPrecF32 as the template argument
        self.L = len(self.dims) - 1
        self.nb, self.rows = (sets, rows_per_set) if sets else (1, rows_per_set)
        self.total = self.nb * self.rows
        self.sz = 2 if self.bf16 else 4  # phase_sz = grad_sz = op_sz
        self.order = order
        self.C = self.dims[0]
        self.Su = self.C + (1 if order == 2 else self.C * (self.C + 1) // 2 if order == 4 else 0)
        self.S = self.Sb = 1 + self.Su

    def jtn_split(self, stacked_rows, M, N):
        return split_rows(stacked_rows, cdiv(M, 128) * cdiv(N, 128), self.nb, 32)

    def jcol_split(self):
        return split_rows(self.rows, 1, self.nb, 64)

    def jtn2_split(self, stacked_rows, N):  # JTN2_BN = 128, JTN2_KC = 32
        want = max(1, 256 // (cdiv(N, 128) * self.nb))
        rps = max(32, align_up(cdiv(stacked_rows, want), 32))
        return max(1, cdiv(stacked_rows, rps)), rps

    def split_stride(self, slab):
        return align_up(self.nb * slab, 4)

    def slab(self, l):
        return self.dims[l + 1] * self.dims[l] + self.dims[l + 1]


def parent_layout(case, order):
    """jlayout_of (and the prepared-weight bytes of layout_of it starts from): saved_bytes, ws_bytes, part_off."""
    g = Shape(case, order)
    d, L, nb = g.dims, g.L, g.nb
    off = 0  # layout_of: weights_bytes (1..4 inputs: no wide first layer)
    for l in range(1, L - 1):
        n = nb * d[l + 1] * d[l]
        if g.bf16:
            off = align_up(off + n * g.sz, 256)
        off = align_up(off + n * g.sz, 256)
    fused_shape = g.bf16 and d[L] <= 8 and d[0] <= 4 and all(w == 256 for w in d[1:L]) and L - 2 <= 14
    if fused_shape and L > 2:  # FREG_WL_BYTES = 4096
        off = align_up(off + nb * ((L - 2) * d[1] * d[1] + 4096 // 2) * 2 + nb * (L - 2) * d[1] * 4, 256)
    weights_bytes = off
    for l in range(L - 1):
        off = align_up(off + g.total * d[l + 1] * g.sz, 256)
    for l in range(L - 1):
        off = align_up(off + g.Su * g.total * d[l + 1] * 4, 256)
    saved_bytes = off
    off = align_up(weights_bytes, 256)
    act = g.Sb * g.total * max(d[1:L])
    for _ in range(2):
        off = align_up(off + act * g.sz, 256)
    off = align_up(off + act * 4, 256)
    part = 0
    for l in range(1, L - 1):
        M, N = d[l + 1], d[l]
        part = max(part, g.jtn_split(g.Sb * g.rows, M, N)[0] * g.split_stride(M * N + M))
    ns = g.jcol_split()[0]
    part = max(part, ns * g.split_stride(d[L] * d[L - 1] + d[L]))
    part = max(part, ns * g.split_stride(d[1] * d[0] + d[1]))
    part_off = off
    off = align_up(off + part * 4, 256)
    return {"saved_bytes": saved_bytes, "ws_bytes": off, "part_off": part_off}


def line(tag, sym, layer, cur, grid, block, nsplit=None):
    gr = tuple(grid) + (1,) * (3 - len(grid))
    t = f"{tag} siren::{sym} layer={layer} cur={cur} grid=({gr[0]},{gr[1]},{gr[2]}) block={block}"
    return t + (f" slab=part nsplit={nsplit}" if nsplit is not None else "")


def parent_forward(case, order, primal):
    """What jvp_forward_impl of commit 8849abc launches (after prep_weights), as plan lines."""
    opt = _native.get_option
    g = Shape(case, order)
    d, L, nb, rows, P = g.dims, g.L, g.nb, g.rows, g.P
    lap, hess = order == 2, order == 4
    out = [line("fwd", f"jvp_first_kernel<{P}>", 0, 0, (grid1d(rows * d[1], max(1, 4096 // nb)), nb), 256)]
    for l in range(1, L - 1):
        K, Nout = d[l], d[l + 1]
        srow0 = rows if primal else 0
        if (not g.bf16 and primal and not lap and not hess and opt("jvp_tan") and 1 <= g.C <= 4 and Nout <= 256 and
                K % 32 == 0):  # JADJ_BN = 256, JNT_KC = 32
            out.append(line("fwd", f"jvp_tan_kernel<0, {g.C}>", l, 0, (cdiv(rows, 64), nb), 512))  # JADJ_ROWS = 64
            continue
        grid = (cdiv(g.S * rows - srow0, 128), cdiv(Nout, 256), nb)  # JNT_BM = 128, JNT_BN = 256
        form = ", true" if lap else ", false, true" if hess else ""
        out.append(line("fwd", f"jvp_nt_kernel<{P}, JMODE_FWD{form}>", l, 0, grid, 256))
    lgrid = (min(cdiv(rows, 8), 4096 // nb + 1), nb)
    sym = f"jvp_last_hess_kernel<{P}, {g.C}>" if hess else f"jvp_last_kernel<{P}>"
    out.append(line("fwd", sym, L - 1, 0, lgrid, 256))
    return out


def parent_backward(case, order, want_dx):
    """What jvp_backward_impl of commit 8849abc launches, as plan lines."""
    opt = _native.get_option
    g = Shape(case, order)
    d, L, nb, rows, P = g.dims, g.L, g.nb, g.rows, g.P
    lap, hess, jac = order == 2, order == 4, order == 3
    out, cur = [], 0

    def reduce(l, nsplit):  # launch_reduce
        out.append(line("bwd", "reduce_kernel", l, cur, (reduce_blocks(nb, g.slab(l)),), 256, nsplit))

    def hess_combine(top):
        return f"jvp_hess_combine_kernel<{P}, {g.C}, {'true' if top else 'false'}>"

    ns, _ = g.jcol_split()
    sym = hess_combine(True) if hess else f"jvp_combine_jac_kernel<{P}>" if jac else f"jvp_combine_kernel<{P}>"
    out.append(line("bwd", sym, L - 1, cur, (ns, nb), 256, ns))
    reduce(L - 1, ns)
    for l in range(L - 2, 0, -1):
        M, N = d[l + 1], d[l]
        s = g.jtn_split(g.Sb * rows, M, N)
        if not g.bf16 and not hess and (opt("jvp_tn2") and M == 256 and N % 4 == 0):  # jvp_tn2_ok
            s2 = g.jtn2_split(g.Sb * rows, N)
            out.append(line("bwd", f"jvp_tn2_kernel<{'true' if lap else 'false'}>", l, cur, (cdiv(N, 128), s2[0], nb), 512,
                            s2[0]))
            reduce(l, s2[0])
        else:
            form = ", true" if lap else ", false, true" if hess else ""
            out.append(line("bwd", f"jvp_tn_kernel<{P}{form}>", l, cur, (cdiv(M, 128) * cdiv(N, 128), s[0], nb), 256, s[0]))
            reduce(l, s[0])
        # jvp_adj_fused(Sb, lapmode, N)
        if not hess and (opt("jvp_adj") and 2 <= g.Sb <= 4 and not (lap and g.Sb < 3) and N <= 256):
            out.append(line("bwd", f"jvp_adj_kernel<{P}, {g.Sb}, {'true' if lap else 'false'}>", l, cur,
                            (cdiv(rows, 64), nb), 512))
            cur ^= 1
            continue
        out.append(line("bwd", f"jvp_nt_kernel<{P}, JMODE_BWD>", l, cur, (cdiv(g.Sb * rows, 128), cdiv(N, 256), nb), 256))
        sym = hess_combine(False) if hess else f"jvp_combine_kernel<{P}>"
        out.append(line("bwd", sym, l, cur, (g.jcol_split()[0], nb), 256))
        cur ^= 1
    ns, _ = g.jcol_split()
    out.append(line("bwd", f"jvp_first_bwd_kernel<{P}>", 0, cur, (ns, nb), 256, ns))
    reduce(0, ns)
    if want_dx:
        out.append(line("bwd", f"jvp_first_dx_kernel<{P}>", 0, cur, (min(cdiv(rows, 8), 4096 // nb + 1), nb), 256))
    return out


def parent_plan(case, order, flags):
    g = Shape(case, order)
    fwd, bwd = parent_forward(case, order, bool(flags & 2)), parent_backward(case, order, bool(flags & 1))
    head = f"# order={order} prec={g.prec} flags={flags} streams={g.S} fwd={len(fwd)} bwd={len(bwd)}\n"
    return head + "".join(t + "\n" for t in fwd + bwd)


def parent_refusal(case, order, flags):
    """The message with which the library refuses an entry (None: it does not): jvp_check through the size
    query, the primal rule through siren_jvp_forward_ex, which applies it before it looks at a buffer."""
    lib = _native.load_library()
    d = describe(case)
    if lib.siren_jvp_saved_bytes(ctypes.byref(d), order) < 0:
        return _native.last_error()
    if flags & 2 and CASES[case][0] != "fp32":
        rc = lib.siren_jvp_forward_ex(ctypes.byref(d), order, None, None, None, None, 0, None, 0, 256, 0, None)
        assert rc != 0
        return _native.last_error()
    return None


def pack(recorded, plans, refused):
    """The recorded sizes, plan texts and refusals as jvp_plan.json keeps them: every distinct launch line once,
    in "lines", and per "case|order|setting" the sizes, the stream count and the lines' indices of the forward
    pass (without / with a primal buffer), of the backward pass and of its input-gradient launch."""
    table = sorted({ln for t in plans.values() for ln in t.splitlines()[1:]})
    at = {ln: i for i, ln in enumerate(table)}
    entries = {}
    for key, sz in recorded.items():
        case = key.split("|")[0]
        e = entries[key] = {"sizes": sz}
        if f"{key}|0" in refused:
            e["refused"] = refused[f"{key}|0"]
            continue
        texts = [plans[f"{key}|{f}"].splitlines() for f in FLAGS[CASES[case][0]]]
        e["streams"] = int(texts[0][0].split("streams=")[1].split()[0])
        e["fwd"] = [[at[ln] for ln in t[1:] if ln.startswith("fwd ")] for t in texts[::2]]
        e["bwd"] = [at[ln] for ln in texts[0][1:] if ln.startswith("bwd ")]
        e["dx"] = at[texts[1][-1]]
    return {"cases": {k: {"precision": v[0], "dims": v[1], "weight_sets": v[2], "rows": v[3]} for k, v in CASES.items()},
            "settings": list(SETTINGS), "lines": table, "entries": entries, "bf16_primal": {BF16_PRIMAL: refused[BF16_PRIMAL]}}


def unpack(doc):
    """jvp_plan.json as {"sizes": per "case|order|setting", "plans" and "refused": per "case|order|setting|flags"}."""
    out = {"cases": doc["cases"], "settings": doc["settings"], "sizes": {}, "plans": {}, "refused": dict(doc["bf16_primal"])}
    for key, e in doc["entries"].items():
        case, order, _ = key.split("|")
        prec = doc["cases"][case]["precision"]
        out["sizes"][key] = e["sizes"]
        for flags in FLAGS[prec]:
            if "refused" in e:
                out["refused"][f"{key}|{flags}"] = e["refused"]
                continue
            fwd = [doc["lines"][i] for i in e["fwd"][flags >> 1]]
            bwd = [doc["lines"][i] for i in e["bwd"] + ([e["dx"]] if flags & 1 else [])]
            head = f"# order={order} prec={prec} flags={flags} streams={e['streams']} fwd={len(fwd)} bwd={len(bwd)}"
            out["plans"][f"{key}|{flags}"] = "".join(t + "\n" for t in [head] + fwd + bwd)
    return out


def load():
    with open(os.path.join(OUT, "jvp_plan.json")) as f:
        return unpack(json.load(f))


def main():
    lib = _native.load_library()
    has_plan = hasattr(lib, "siren_jvp_plan")
    recorded, plans, refused, differ = {}, {}, {}, []
    for case in CASES:
        d = describe(case)
        assert lib.siren_mlp_check(ctypes.byref(d)) == 0, (case, _native.last_error())
        for order in ORDERS:
            for s in SETTINGS:
                with setting(s):
                    got = recorded[f"{case}|{order}|{s}"] = sizes(d, order)
                    if admits(case, order):
                        lay = parent_layout(case, order)
                        assert got == [lay["saved_bytes"], lay["ws_bytes"] + lay["saved_bytes"]], (case, order, s, got, lay)
                    else:
                        assert got == [-1, -1], (case, order, got)
    for key in keys():
        case, order, s, flags = key.split("|")
        order, flags = int(order), int(flags)
        with setting(s):
            msg = parent_refusal(case, order, flags)
            if msg is not None:
                refused[key] = msg
            else:
                plans[key] = parent_plan(case, order, flags)
            if has_plan and plan_text(describe(case), order, flags) != plans.get(key):
                differ.append(key)
    doc = pack(recorded, plans, refused)
    back = unpack(doc)
    assert (back["sizes"], back["plans"], back["refused"]) == (recorded, plans, refused)  # nothing lost in packing
    row = lambda v: json.dumps(v, sort_keys=True)  # noqa: E731
    with open(os.path.join(OUT, "jvp_plan.json"), "w") as f:
        f.write('{\n "cases": %s,\n "settings": %s,\n "bf16_primal": %s,\n' % tuple(row(doc[k]) for k in ("cases", "settings", "bf16_primal")))
        f.write(' "lines": [\n  ' + ",\n  ".join(row(ln) for ln in doc["lines"]) + "\n ],\n")
        f.write(' "entries": {\n  ' + ",\n  ".join(f"{row(k)}: {row(e)}" for k, e in sorted(doc["entries"].items())) + "\n }\n}\n")
    print("wrote jvp_plan.json:", len(recorded), "sizes,", len(plans), "plans in", len(doc["lines"]), "distinct lines,",
          len(refused), "refused;",
          ("the library's plan differs in %d %s" % (len(differ), differ[:8])) if has_plan else "the library has no siren_jvp_plan")


if __name__ == "__main__":
    main()
