"""Exact-arithmetic data, references and the mismatch report for the conv encoder's kernels
(siren_conv.hip behind siren_conv_fwd_k5 / siren_conv_fwd / siren_conv_fwd_k5_res /
siren_conv_dgrad_k5_fused / siren_conv_wrw_k5 / siren_conv_wrw). No GPU in this file.

A convolution has no transcendental in it. bf16 operands holding small integers have exact products,
and fp32 sums of them are exact in any order while sum |x| |w| stays below 2^24; the conversion of an
exact fp32 value to bf16 is then a pure function of the value. So on such data the fp64 convolution
followed by the roundings include/siren_mri_amd.h documents must equal a kernel's output element for
element (torch.equal): no tolerance, no element left out. tests/test_exact_cpu.py asserts every
condition named here on the references alone, for every case tests/test_gpu_conv_exact.py runs.

Recipes (a seeded torch.Generator in, integer-valued bf16 tensors out):

  lossless  max |acc| <= 256, so every accumulator is a bf16 value and bf16(acc) loses nothing: any
            mismatch is a wrong or a missing term (indexing, halos, ragged workgroups).
              64 / 128 input channels: x and w in {-1, 0, 1}, each nonzero with probability 0.25
              2 input channels (a reduction of 2 k^2 terms only): x dense in [-3, 3], w in [-2, 2]
  rounding  sums reach the hundreds and thousands, where bf16 keeps 8 bits: pins round-to-nearest-even
            of the epilogue's conversion, with exact ties (accumulators halfway between two bf16
            values). x dense in [-mx, mx], w dense in [-mw, mw], (mx, mw) the first step of LADDER =
            (3, 2), (7, 4), (15, 8), (31, 16) at which the sum's standard deviation
            sqrt(K mx (mx + 1) / 3 mw (mw + 1) / 3) reaches SIGMA_MIN = 150, K = ci k min(k, H) the
            terms of a sum that lie inside the image (rounding_range). Ties need sums past 256 and are
            rare below that deviation: (3, 2) gives 21,337 ties at 5x5x128 on 10 rows (sigma 160) but
            16 at 3x3x64 (sigma 68) and 222 at 5x5x128 on 2 rows, hence the ladder. It keeps (3, 2) for
            the 5x5x128 and 7x7 shapes on 10 rows and gives (15, 8) for 2 input channels on 5 or 8
            rows. K mx mw < 2^24 at every step (6272 x 31 x 16 = 3.1e6). The weight gradients take
            the same ladder over their N H W terms at a deviation of SIGMA_WRW = 400.
            Ties: at least MIN_TIES (1000) in the reference of every case with 50,000 outputs or more;
            the one-row 2-channel cases hold as few as 4096 outputs, of which no distribution of sums
            puts a quarter on ties, so below 50,000 outputs the condition is one tie per 50 outputs
            (min_ties). All of this is fixed on the fp64 references alone; nothing here has seen a
            kernel's output.

Side operands: the plain forward's bias is randn rounded to bf16 (non-integers, so that
bf16(bf16(acc) + b) differs from bf16(acc + b)); the fused epilogues' planes and cb are integers in
[-2, 2], so that m == 0 and bf16(pa + cb) == 0 each occur in at least 5 % of the elements (`>` against
`>=`), and so that the channel sums db are sums of integers: exact while sum |.| < 2^24.

Layouts are the kernels': activations NHWC [N][H][W][C], filters [co][kh][kw][ci], dw likewise (fp32).
"""
import functools

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EXACT = 2 ** 24          # fp32 holds every integer up to here
LOSSLESS_MAX = 256       # bf16 holds every integer up to here
MIN_TIES = 1000
MIN_ZERO_SHARE = 0.05
RECIPES = ("lossless", "rounding")
LADDER = ((3, 2), (7, 4), (15, 8), (31, 16))
SIGMA_MIN = 150.0
SIGMA_WRW = 400.0  # weight gradients (fp32 out, a sum over N H W pixels): sums that reach the thousands

# ------------------------------------------------------------------ the cases of the GPU file
FWD_K5 = (5, 128, 128)
FWD_GEN = [(k, ci, co) for k in (3, 5, 7) for ci in (64, 128) for co in (64, 128)] + [(3, 64, 192), (5, 128, 256)]
FWD_NH = [(3, 10), (1, 2)]            # 64 / 128 input channels (W = 128)
FWD_T = [(k, 2, co) for k in (3, 5, 7) for co in (32, 64, 96, 128)]
FWD_T_NH = [(3, 5), (1, 1), (2, 8)]   # 2 input channels: 4 rows per workgroup
BIAS_RELU = [(False, False), (True, False), (True, True)]
EPI_NH = (3, 10)
EPI_BIG_NH = (129, 4)                 # 258 workgroups: conv_chan_reduce_kernel's second iteration
WRW_NHW = [(1, 3, 256), (3, 7, 192)]
WRW_GEN = [(7, 64, 128), (3, 128, 64), (5, 128, 128), (7, 2, 64), (3, 2, 96)]
W_FWD = 128


def gen(*key):
    """A generator seeded by the case (any hashable ints / strings)."""
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
        s = (s * 131 + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def dense(g, shape, m):
    """Integers uniform in [-m, m], bf16."""
    return torch.randint(-m, m + 1, shape, generator=g).to(BF16)


def sparse(g, shape, p=0.25):
    """{-1, 0, 1}, nonzero with probability p, bf16."""
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (sign * (torch.rand(shape, generator=g) < p)).to(BF16)


def rounding_range(terms, sigma_min=SIGMA_MIN):
    """The `rounding` recipe's (mx, mw) for sums of `terms` products (see the module docstring)."""
    for mx, mw in LADDER:
        if (terms * mx * (mx + 1) / 3 * mw * (mw + 1) / 3) ** 0.5 >= sigma_min:
            break
    return mx, mw


def draw_pair(recipe, ci, g, a_shape, b_shape, terms, sigma_min=SIGMA_MIN):
    """The recipe's two operands (the image and the filter; for a weight gradient the image and dy) for
    sums of `terms` products."""
    if recipe == "lossless" and ci != 2:
        return sparse(g, a_shape), sparse(g, b_shape)
    mx, mw = (3, 2) if recipe == "lossless" else rounding_range(terms, sigma_min)
    return dense(g, a_shape, mx), dense(g, b_shape, mw)


def min_ties(numel):
    return MIN_TIES if numel >= 50 * MIN_TIES else numel // 50


# ------------------------------------------------------------------ layouts and roundings
def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def to_bf16(t):
    """Round to nearest, ties to even (through fp32, which holds the exact integers of these tests)."""
    return t.to(F32).to(BF16)


def trunc_bf16(t):
    """Wrong on purpose: drop the low 16 bits of the fp32 value."""
    bits = t.to(F32).contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(F32).to(BF16)


def half_away_bf16(t):
    """Wrong on purpose: round to nearest, ties away from zero."""
    bits = t.to(F32).contiguous().view(torch.int32)
    return (((bits & 0x7FFFFFFF) + 0x8000) & ~0xFFFF | (bits & -0x80000000)).view(F32).to(BF16)


def count_ties(acc):
    """Exact bf16 ties among integer-valued accumulators: halfway between two neighbouring bf16 values."""
    bits = acc.to(F32).contiguous().view(torch.int32)
    return int(((bits & 0xFFFF) == 0x8000).sum())


# ------------------------------------------------------------------ data + references, cached per case
class Case(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=4)
def _forward_cached(recipe, k, ci, co, N, H, W):
    g = gen("fwd", recipe, k, ci, co, N, H, W)
    x, w = draw_pair(recipe, ci, g, (N, H, W, ci), (co, k, k, ci), ci * k * min(k, H))
    bias = torch.randn(co, generator=g).to(BF16)
    acc = F.conv2d(nchw(x).double(), nchw(w).double(), padding=k // 2)  # NCHW fp64: exact
    return Case(x=x, w=w, bias=bias, acc=nhwc(acc), k=k, ci=ci, co=co, recipe=recipe)


def forward_case(recipe, k, ci, co, N, H, W=W_FWD):
    """x [N][H][W][ci], w [co][k][k][ci], a randn bf16 bias [co] and acc = conv(x, w) in fp64, NHWC.
    Shared between the tests of one case and never written to."""
    return _forward_cached(recipe, k, ci, co, N, H, W)


def forward_ref(acc, bias=None, relu=False, cast=to_bf16, single_rounding=False):
    """The header's roundings: y = bf16(acc); with a bias bf16(bf16(acc) + b) (a bf16 add: the fp32 sum
    of two bf16 values, rounded), then ReLU. `cast` and `single_rounding` are for the emulated wrong
    answers of tests/test_exact_cpu.py."""
    if bias is None:
        return cast(acc)
    y = cast(acc.to(F32) + bias.to(F32)) if single_rounding else cast(cast(acc).to(F32) + bias.to(F32))
    return torch.relu(y) if relu else y


@functools.lru_cache(maxsize=2)
def _epilogue_cached(recipe, N, H):
    c = forward_case(recipe, *FWD_K5, N, H) if (N, H) != EPI_BIG_NH else None
    g = gen("epi", recipe, N, H)
    if c is None:  # its own draw, kept apart from the forward cache (17 MB an operand)
        x, w = draw_pair(recipe, 128, g, (N, H, W_FWD, 128), (128, 5, 5, 128), 128 * 5 * min(5, H))
        acc = nhwc(F.conv2d(nchw(x).double(), nchw(w).double(), padding=2))
    else:
        x, w, acc = c.x, c.w, c.acc
    side = {n: dense(g, (N, H, W_FWD, 128), 2) for n in ("g2", "t", "m", "pa")}
    return Case(x=x, w=w, acc=acc, cb=dense(g, (128,), 2), recipe=recipe, **side)


def epilogue_case(recipe, N, H):
    """The 128 -> 128 5x5 operands of the recipe with the fused epilogues' side operands: planes g2, t,
    m, pa [N][H][128][128] and cb [128], integers in [-2, 2]."""
    return _epilogue_cached(recipe, N, H)


def res_ref(c):
    """siren_conv_fwd_k5_res: a = bf16(acc), out = relu(bf16(relu(bf16(a + cb)) + t))."""
    a = to_bf16(c.acc)
    return a, torch.relu(torch.relu(a + c.cb) + c.t)  # bf16 adds


def dgrad_ref(c, mode, with_g2, ge=False, blocks=None):
    """siren_conv_dgrad_k5_fused: g = bf16(acc); out = bf16((g [+ g2]) * (m > 0)); mode 2: out2 = out *
    (bf16(pa + cb) > 0); db = channel sums of out (mode 1) or out2 (mode 2), fp64 (exact). Wrong on
    purpose: ge (m >= 0), blocks (db over the first `blocks` workgroups' rows only: a workgroup is a
    pair of image rows)."""
    g = to_bf16(c.acc)
    s = g + c.g2 if (with_g2 or mode == 2) else g  # a bf16 add
    out = s * ((c.m >= 0) if ge else (c.m > 0))
    res = {"out": out}
    last = out
    if mode == 2:
        last = res["out2"] = out * ((c.pa + c.cb) > 0)
    pairs = last.double().reshape(-1, 2 * W_FWD, 128)  # [workgroup][its pixels][channel]
    res["db"] = pairs[:blocks].sum((0, 1))
    res["db_abs"] = last.double().abs().sum((0, 1, 2))
    return res


@functools.lru_cache(maxsize=2)
def _wrw_cached(recipe, k, ci, co, N, H, W):
    g = gen("wrw", recipe, k, ci, co, N, H, W)
    x, dy = draw_pair(recipe, ci, g, (N, H, W, ci), (N, H, W, co), N * H * W, SIGMA_WRW)
    xd, dyd = nchw(x).double(), nchw(dy).double()
    dw = torch.nn.grad.conv2d_weight(xd, (co, ci, k, k), dyd, padding=k // 2)
    bound = torch.nn.grad.conv2d_weight(xd.abs(), (co, ci, k, k), dyd.abs(), padding=k // 2)
    return Case(x=x, dy=dy, dw=nhwc(dw), abs_max=float(bound.max()), recipe=recipe)


def wrw_case(recipe, k, ci, co, N, H, W):
    """x [N][H][W][ci], dy [N][H][W][co], dw [co][k][k][ci] = the fp64 weight gradient, and abs_max =
    max over dw's elements of sum |x| |dy| (below 2^24: dw.float() is what any fp32 order gives)."""
    return _wrw_cached(recipe, k, ci, co, N, H, W)


# ------------------------------------------------------------------ the old criterion, for the CPU pins
def norm_rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def old_criterion(got, ref):
    """tests/test_gpu_encoder.py's forward criterion: (norm_rel, share of elements within one bf16 step,
    verdict of `norm_rel < 4e-3 and share > 0.999`)."""
    got, ref = got.float(), ref.float()
    nr = norm_rel(got, ref)
    share = float(((got - ref).abs() <= ref.abs() * 2 ** -7 + 1e-6).float().mean())
    return nr, share, nr < 4e-3 and share > 0.999


# ------------------------------------------------------------------ the report
def _ordered(t):
    """Bit patterns as integers that count representable values in order (bf16 or fp32)."""
    t = t.contiguous()
    if t.dtype == BF16:
        b = t.view(torch.int16).to(torch.int64)
        return torch.where(b < 0, -(b & 0x7FFF), b)
    b = t.to(F32).view(torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def mismatch_report(got, ref, dims=("n", "h", "w", "c")):
    """Where `got` differs from `ref`: the number of differing elements, their counts along every
    dimension (the first 8 indices that have any, as index:count), and the largest difference in steps of
    the format (bf16 steps for bf16 tensors). An empty string when they are equal."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype} against {tuple(ref.shape)} {ref.dtype}"
    bad = _ordered(got) != _ordered(ref)  # (+0 and -0 are one value)
    bad |= got.isnan() != ref.isnan()
    n = int(bad.sum())
    if n == 0:
        return ""
    names = list(dims[-got.dim():]) if got.dim() <= len(dims) else [f"d{i}" for i in range(got.dim())]
    lines = [f"{n} of {bad.numel()} elements differ"]
    for d, name in enumerate(names):
        cnt = bad.sum([i for i in range(got.dim()) if i != d]) if got.dim() > 1 else bad.long()
        idx = cnt.nonzero().flatten()
        first = " ".join(f"{int(i)}:{int(cnt[i])}" for i in idx[:8])
        lines.append(f"  per {name} ({len(idx)} of {cnt.numel()} have any): {first}{' ...' if len(idx) > 8 else ''}")
    steps = (_ordered(got) - _ordered(ref)).abs()
    at = int(steps.argmax())
    where = [int(i) for i in torch.unravel_index(torch.tensor(at), got.shape)]
    unit = "bf16 steps" if got.dtype == BF16 else "fp32 steps"
    lines.append(f"  largest difference {int(steps.flatten()[at])} {unit} at {dict(zip(names, where))}: "
                 f"got {float(got.flatten()[at])!r}, reference {float(ref.flatten()[at])!r}")
    return "\n".join(lines)


def assert_equal(got, ref, what, dims=("n", "h", "w", "c")):
    got = got.detach().cpu()
    assert torch.equal(got, ref), f"{what}\n{mismatch_report(got, ref, dims)}"
