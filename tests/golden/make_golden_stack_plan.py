"""The backward launch plans of the case grid of make_golden_stack_sizes.py (CPU only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stack_plan.py [class_counts.json]

  stack_plan.json  "variants": per case, the flags of siren_mlp_backward_plan it is planned with (bit 0
                   an input gradient is wanted, bit 1 x is 16-byte aligned, bit 2 dy is); "gpu_variants":
                   those a GPU run can produce (dy from autograd is always aligned); "plans": the plan
                   text per "case|setting|flags"; "class_counts": per "case|setting|flags" of the GPU
                   variants under the settings GPU_SETTINGS, the launches of each kernel class 1..14 in
                   one forward + backward, MEASURED with _native.KernelTimer on an MI355X at the commit
                   before the backward became a plan (the file given on the command line replaces
                   them; without one the recorded counts are kept).
The plan texts do NOT come from the library's plan_backward. parent_plan() below is a transcription,
statement by statement, of backward_impl / launch_pair / launch_nt / dispatch_first_bwd of
siren_mri_amd/csrc/rt_mlp.hip as they stood at commit 87ad356, before the plan existed: the same
booleans (fuse, rec, top_ok, ring_top, top, ring_bot, bot, is_top, is_bot, rec1, ring_t, ring), the same
`kind`, the same flush() positions and slab ping-pong, with a text line where that code launched a
kernel. It reads the options through siren_config_get and nothing else from the library. The library's
text is only compared with it (here, as a check before writing, and in tests/test_stack_plan.py).
tests/test_gpu_stack_plan.py checks on the GPU that the launches counted per class are the recorded
ones and the ones the plan text names.
"""
import ctypes
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_stack_sizes import CASES, OUT, SETTINGS, describe, setting  # noqa: E402
from siren_mri_amd import _native  # noqa: E402

GPU_VARIANTS = {"a": [6, 7, 5], "b": [6], "c": [6], "d": [6, 7], "e": [6, 7], "f": [6, 7], "g": [6], "h": [6, 7],
                "i": [6, 7], "j": [6, 7]}
# + a misaligned dy (no output-layer fusion) and a misaligned wide x (no vector reads), which only the C ABI can be handed
VARIANTS = {k: v + {"a": [3], "d": [2], "f": [4]}.get(k, []) for k, v in GPU_VARIANTS.items()}
GPU_SETTINGS = ("default", "pair_ring=0")
FORWARD_CLASSES = (_native.KCLASS_FWD_GEMM, _native.KCLASS_FWD_FUSED)  # not in a backward plan


def plan_text(desc, flags):
    lib = _native.load_library()
    n = lib.siren_mlp_backward_plan(ctypes.byref(desc), flags, None, 0)
    assert n > 0, _native.last_error()
    buf = ctypes.create_string_buffer(n)
    assert lib.siren_mlp_backward_plan(ctypes.byref(desc), flags, buf, n) == n
    return buf.value.decode()


def plan_class_counts(text):
    """Launches per kernel class (> 0) that a plan text names."""
    counts = {}
    for line in text.splitlines():
        m = re.search(r" class=(\d+) ", line)
        if m and int(m.group(1)) > 0:
            counts[m.group(1)] = counts.get(m.group(1), 0) + 1
    return counts


# ------------------------------------------------------------------ the parent's launch code, transcribed
def cdiv(a, b):
    return (a + b - 1) // b


def align_up(v, a):
    return cdiv(v, a) * a


def split_rows(rows, blocks_per_split, nb, granule):  # kTargetBlocks = 1024
    want = max(1, 1024 // max(1, blocks_per_split * nb))
    rps = max(align_up(cdiv(rows, want), granule), granule)
    return max(1, cdiv(rows, rps)), rps  # (nsplit, rows_per_split)


def parent_plan(case, flags):
    """What backward_impl of commit 87ad356 launches for `case` under the current options, as plan text."""
    opt = _native.get_option
    prec, dims, sets, rows_per_set = CASES[case]
    bf16 = prec == "bf16"
    want_dx, x16, dy16 = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    L = len(dims) - 1
    nb, rows = (sets, rows_per_set) if sets else (1, rows_per_set)  # geo_of (shared weights: batch 1)
    O, C, F0 = dims[L], dims[0], dims[1]
    wide_input = C > 16
    # fused_shape / fused_wide / p0_recompute / Layout::part2_off
    fused_wide = 4 < C <= 16
    fused_shape = (bf16 and O <= 8 and (not fused_wide or (opt("fused_forward_reg") and 1 <= L - 2 <= 6)) and
                   (fused_wide or C <= 4) and all(dims[l] == 256 for l in range(1, L)) and L - 2 <= 14)
    rec = bool(not opt("debug_keep_p0") and fused_shape and not fused_wide and L >= 3)
    has_part2 = fused_shape and L >= 4

    def tn_split(M, N):
        return split_rows(rows, cdiv(M, 128) * cdiv(N, 128), nb, 64)

    valu_split = split_rows(rows, 1, nb, 64)
    rps_ring = max(32, align_up(cdiv(rows, max(1, 256 // nb)), 32))
    dw_ring_split = (max(1, cdiv(rows, rps_ring)), rps_ring)
    npair = min(max(8, (128 // nb) // 8 * 8), align_up(cdiv(rows, 32), 8))  # pair_count
    pair_ok = nb <= 64

    def nt_grid(K, N):
        ntn = cdiv(N, 256)
        bm = (64 * 256 // (256 if K <= 256 else 512)) if bf16 else 32
        return (min(cdiv(rows, bm), max(1, 256 // max(1, nb * ntn))), nb, ntn)

    ring_grid = (min(cdiv(rows, 32), max(1, 256 // nb)), nb, 1)
    P = 1 if bf16 else 0  # kPrecBF16 / kPrecF32 as the template argument
    lines, pend = [], [None]

    def slab_elems(l):
        return dims[l + 1] * dims[l] + dims[l + 1]

    def emit(sym, kclass, layer, grid, block, slabs=(), reduce=""):
        g = tuple(grid) + (1,) * (3 - len(grid))
        lines.append({"sym": sym, "head": f"class={kclass} layer={layer} grid=({g[0]},{g[1]},{g[2]}) block={block}",
                      "slabs": list(slabs), "layers": [], "extra": "", "reduce": reduce})
        return lines[-1]

    def launch_reduce(layer, buf, nsplit):  # grid: cdiv(nb * slab, 128)
        emit("siren::reduce_kernel", 0, layer, (cdiv(nb * slab_elems(layer), 128),), 256, [(buf, nsplit)])

    def flush():  # ReduceList::launch of the pending pair launch's slabs
        if pend[0] is None:
            return
        src = pend[0]
        src["reduce"] = "flush"
        blocks = sum(cdiv(nb * slab_elems(l), 128) for l in src["layers"])
        emit("siren::reduce_multi_kernel", 0, src["layer"], (blocks,), 256, src["slabs"])
        pend[0] = None

    if rec and not x16:  # hipMemcpyAsync of x into the workspace; x is aligned from here on
        lines.append({"sym": "hipMemcpyAsync", "head": "class=0 layer=0 grid=(0,0,0) block=0", "slabs": [], "layers": [],
                      "extra": "", "reduce": ""})
    copied = rec and not x16
    x16 = x16 or copied
    fuse = bf16 and bool(opt("fused_backward")) and L >= 3
    top_ok = (fuse and O <= 2 and (rows * O) % 4 == 0 and rows * O >= 4 and dy16 and not (rec and L == 3))  # outermost_linear
    ring_top = bool(top_ok and opt("ring_output_fusion") and L >= 4 and dims[L - 1] == 256 and dims[L - 2] == 256)
    top = bool(ring_top or (top_ok and opt("fuse_output_layer") and dims[L - 1] <= 256))
    ring_bot = bool(rec or (fuse and opt("dx_ring") and not wide_input and C <= 4 and F0 == 256 and dims[2] == 256 and
                            not (top and L == 3) and (rows * C) % 4 == 0 and rows * C >= 4 and x16))
    bot = bool(ring_bot or (fuse and not want_dx and not wide_input and C <= 4 and F0 <= 256 and (rows * C) % 4 == 0 and
                            rows * C >= 4 and x16 and not (top and L == 3)))
    it = lambda F: 1 if F <= 256 else 2 if F <= 512 else 4  # noqa: E731
    topo = 1 if O == 1 else 2
    npair_launches = 0
    done = False
    if not top:  # output layer: dispatch_last_bwd + launch_reduce
        ns, _ = valu_split
        emit(f"siren::last_bwd_kernel<{P}, {it(dims[L - 1])}, {2 if O <= 2 else 8}>", 0, L - 1, (ns, nb), 256,
             [("part", ns)], "own")
        launch_reduce(L - 1, "part", ns)
    for l in range(L - 2, 0, -1):
        M, N = dims[l + 1], dims[l]
        is_top, is_bot, rec1, ring_t = top and l == L - 2, bot and l == 1, rec and l == 1, ring_top and l == L - 2
        if bf16 and opt("pair_ring") and pair_ok and M == 256 and N == 256:
            kind = (3 if rec1 and not is_top else 2 if ring_t and not is_bot else
                    1 if not is_top and not is_bot and not rec1 and opt("dw_ring") and opt("dx_ring") else 0)
            if kind:
                pp = "part"
                if not opt("pair_tail_reduce"):
                    flush()
                if has_part2:
                    if npair_launches & 1:
                        pp = "part2"
                    npair_launches += 1
                else:
                    flush()
                # launch_pair
                if pend[0] is not None:
                    pend[0]["reduce"] = "next_pair"  # prev = pend.a: reduced in this launch's tail
                if kind == 1:
                    sym, kcls, slabs, layers = "0, false, false, 0, 0", 12, [(pp, npair)], [l]
                elif kind == 2:
                    sym, kcls, slabs, layers = f"0, false, false, {topo}, 0", 13, [(pp, npair), ("partL", npair)], [l, L - 1]
                else:
                    cc = min(C, 4)
                    sym = f"{cc}, {'true' if want_dx else 'false'}, true, 0, {cc}"
                    kcls, slabs, layers = 14, [(pp, npair), ("partB", npair)], [l, 0]
                pend[0] = emit(f"siren::pair_ring_bf16_kernel<{sym}>", kcls, l, (2 * npair, nb), 512, slabs)
                pend[0]["layers"], pend[0]["layer"] = layers, l
                if kind == 3:
                    flush()
                    done = True  # first layer done
                    break
                continue
        flush()  # the per-layer kernels below reuse `part`
        ring = rec1 or ring_t or (bf16 and bool(opt("dw_ring")) and not is_top and M == 256 and N == 256)
        ns, _ = dw_ring_split if ring else tn_split(M, N)
        tn_grid = (cdiv(M, 128) * cdiv(N, 128), ns, nb)
        w_slabs = [("part", ns)] + ([("partL", ns)] if is_top else [])
        if bf16:
            if rec1:
                emit(f"siren::dw_ring_bf16_kernel<{min(C, 4)}, 0>", 9, l, (ns, nb), 512, w_slabs, "own")
            elif ring_t:
                emit(f"siren::dw_ring_bf16_kernel<0, {topo}>", 11, l, (ns, nb), 512, w_slabs, "own")
            elif ring:
                emit("siren::dw_ring_bf16_kernel<0, 0>", 7, l, (ns, nb), 512, w_slabs, "own")
            elif is_top:
                emit("siren::tn_dw_kernel<1, false, true>", 3, l, tn_grid, 256, w_slabs, "own")
            else:
                emit("siren::tn_dw_kernel<1, false, false>", 3, l, tn_grid, 256, w_slabs, "own")
            nsplit_used = ns
        elif opt("f32_rows") and opt("jvp_tn2") and M == 256 and N % 4 == 0:  # jvp_tn2_ok; jtn2_split
            rps2 = max(32, align_up(cdiv(rows, max(1, 256 // (cdiv(N, 128) * nb))), 32))
            nsplit_used = max(1, cdiv(rows, rps2))
            emit("siren::jvp_tn2_kernel<false>", 3, l, (cdiv(N, 128), nsplit_used, nb), 512, [("part", nsplit_used)], "own")
        else:
            emit("siren::tn_dw_kernel<0, false, false>", 3, l, tn_grid, 256, w_slabs, "own")
            nsplit_used = ns
        launch_reduce(l, "part", nsplit_used)
        if is_top:
            launch_reduce(L - 1, "partL", ns)
        # input gradient
        kmax = 256 if M <= 256 else 512
        b = lambda v: "true" if v else "false"  # noqa: E731
        if bf16 and is_bot and ring_bot:  # launch_dx_ring_bot
            last = emit(f"siren::dx_ring_bf16_kernel<{min(C, 4)}, {b(want_dx)}, {b(rec1)}, 0>", 8, l, ring_grid, 512)
            nslab = ring_grid[0]
        elif bf16 and ring_t:
            last = emit(f"siren::dx_ring_bf16_kernel<0, false, false, {topo}>", 10, l, ring_grid, 512)
        elif bf16:  # launch_nt<bf16, MODE_DX, is_top, is_bot>
            if not is_top and not is_bot and opt("dx_ring") and M == 256 and N == 256:
                last = emit("siren::dx_ring_bf16_kernel<0, false, false, 0>", 6, l, ring_grid, 512)
            else:
                last = emit(f"siren::nt_bf16_kernel<1, {kmax}, {b(is_top)}, {b(is_bot)}>", 2, l, nt_grid(M, N), 512)
                nslab = nt_grid(M, N)[0]
        elif opt("f32_rows") and M % 32 == 0 and M <= 512 and N <= 256:  # launch_nt<f32, MODE_DX>: the row-stacked tile
            last = emit("siren::jvp_tan_kernel<0, 2, 2>", 2, l, (cdiv(rows, 128), nb), 512)
        else:
            last = emit(f"siren::nt_f32_kernel<1, {kmax}>", 2, l, nt_grid(M, N), 512)
        if is_bot:
            last["slabs"], last["reduce"] = [("part", nslab)], "own"
            launch_reduce(0, "part", nslab)
            done = True  # first layer done
            break
    if not done:
        flush()
        if wide_input:  # tn_dw<RAW> + reduce (+ MODE_DXLIN)
            ns, _ = tn_split(F0, C)
            emit(f"siren::tn_dw_kernel<{P}, true, false>", 0, 0, (cdiv(F0, 128) * cdiv(C, 128), ns, nb), 256, [("part", ns)],
                 "own")["extra"] = f" p_vec={1 if C % 4 == 0 and (flags & 2) else 0}"
            launch_reduce(0, "part", ns)
            if want_dx:
                k = f"nt_bf16_kernel<3, {256 if F0 <= 256 else 512}, false, false>" if bf16 else \
                    f"nt_f32_kernel<3, {256 if F0 <= 256 else 512}>"
                emit("siren::" + k, 0, 0, nt_grid(F0, C), 512)
        else:  # dispatch_first_bwd + reduce
            ns, rps = valu_split
            sl = [("part", ns)]
            if C <= 4:
                emit(f"siren::first_bwd_kernel<{P}, {it(F0)}, 4>", 0, 0, (ns, nb), 256, sl, "own")
            elif F0 <= 256 and (not want_dx or (bf16 and F0 == 256)):
                if bf16 and F0 == 256 and rps % 32 == 0:
                    emit("siren::first_bwd_wide_mfma_kernel", 0, 0, (ns, nb), 256, sl, "own")
                else:
                    emit(f"siren::first_bwd_wide_kernel<{P}, {16 if C == 16 else 0}>", 0, 0, (ns, nb), 256, sl, "own")
                if want_dx:
                    emit("siren::first_dx_wide_kernel", 0, 0, (cdiv(cdiv(rows, 32), 4), nb), 256)
            else:
                emit(f"siren::first_bwd_kernel<{P}, {1 if F0 <= 256 else 2}, 16>", 0, 0, (ns, nb), 256, sl, "own")
            launch_reduce(0, "part", ns)
    out = "ring" if ring_top else "tiled" if top else "last_bwd"
    first = "ring" if ring_bot else "tiled" if bot else "mfma" if wide_input else "valu"
    text = f"# out={out} first={first} xcopy={1 if copied else 0} launches={len(lines)}\n"
    for ln in lines:
        text += ln["sym"] + " " + ln["head"]
        if ln["slabs"]:
            text += " slab=" + "+".join(s for s, _ in ln["slabs"]) + " nsplit=" + "+".join(str(n) for _, n in ln["slabs"])
        text += ln["extra"] + (" reduce=" + ln["reduce"] if ln["reduce"] else "") + "\n"
    return text


def main():
    path = os.path.join(OUT, "stack_plan.json")
    if len(sys.argv) > 1:
        counts = json.load(open(sys.argv[1]))
    else:
        counts = json.load(open(path))["class_counts"]
    plans, differ = {}, []
    for case in CASES:
        d = describe(case)
        for s in SETTINGS:
            with setting(s):
                for flags in VARIANTS[case]:
                    key = f"{case}|{s}|{flags}"
                    plans[key] = parent_plan(case, flags)
                    if plan_text(d, flags) != plans[key]:
                        differ.append(key)
    want = {f"{c}|{s}|{f}" for c in CASES for s in GPU_SETTINGS for f in GPU_VARIANTS[c]}
    assert set(counts) == want, sorted(set(counts) ^ want)
    doc = {"variants": VARIANTS, "gpu_variants": GPU_VARIANTS, "gpu_settings": list(GPU_SETTINGS), "plans": plans,
           "class_counts": {k: {c: n for c, n in v.items() if n} for k, v in counts.items()}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote stack_plan.json:", len(plans), "plans,", len(counts), "measured cases;",
          "the library's plan differs in", len(differ), differ[:8])


if __name__ == "__main__":
    main()
