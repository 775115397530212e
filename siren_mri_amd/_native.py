"""ctypes binding of the C ABI in include/siren_mri_amd.h (libsiren_mri_amd.so).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950) and
loaded lazily at the first kernel call, after ``torch`` so that the kernels register with the
HIP runtime PyTorch already holds. There is deliberately NO fallback: if the library or a GPU
is missing, every SIREN kernel entry point raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch

MAX_LAYERS = 16
PREC_F32 = 0
PREC_BF16 = 1
PREC_F64 = 2  # float64 tensors (siren_mlp64_*): chosen by dtype, not by the precision string
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "float32": PREC_F32,
              "bf16": PREC_BF16, "bfloat16": PREC_BF16}

LIB_NAME = "libsiren_mri_amd.so"
# SIREN_MRI_AMD_LIB: load another build of the same ABI (A/B timing of kernel variants)
LIB_PATH = os.environ.get("SIREN_MRI_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

KCLASS_FWD_GEMM = 1
KCLASS_DX_GEMM = 2
KCLASS_DW_GEMM = 3
KCLASS_FWD_FUSED = 4
KCLASS_BWD_FUSED = 5  # reserved (formerly bwd_ring): nothing launches in it
KCLASS_DX_RING = 6
KCLASS_DW_RING = 7
KCLASS_DX_RING_BOT = 8
KCLASS_DW_RING_REC = 9
KCLASS_DX_RING_TOP = 10
KCLASS_DW_RING_TOP = 11
KCLASS_PAIR_RING = 12
KCLASS_PAIR_RING_TOP = 13
KCLASS_PAIR_RING_BOT = 14


class SirenMLPDesc(ctypes.Structure):
    """Mirror of ``siren_mlp_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("num_layers", ctypes.c_int32),
        ("dims", ctypes.c_int32 * (MAX_LAYERS + 1)),
        ("outermost_linear", ctypes.c_int32),
        ("prec", ctypes.c_int32),
        ("weights_batched", ctypes.c_int32),
        ("w0", ctypes.c_float),
        ("batch", ctypes.c_int64),
        ("rows_per_batch", ctypes.c_int64),
        ("weight", ctypes.c_void_p * MAX_LAYERS),
        ("bias", ctypes.c_void_p * MAX_LAYERS),
        ("ff_B", ctypes.c_void_p),
        ("ff_in", ctypes.c_int32),
    ]


class SirenLossDesc(ctypes.Structure):
    """Mirror of ``siren_loss_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("target", ctypes.c_void_p),
        ("k0", ctypes.c_void_p),
        ("mask", ctypes.c_void_p),
        ("hf", ctypes.c_void_p),
        ("hf_len", ctypes.c_int64),
        ("noise", ctypes.c_float),
        ("weight", ctypes.c_float),
        ("y_dc", ctypes.c_void_p),
        ("dy", ctypes.c_void_p),
        ("loss", ctypes.c_void_p),
        ("loss_workspace", ctypes.c_void_p),
        ("loss_workspace_bytes", ctypes.c_int64),
    ]


# siren_kspace_loss_forward / _backward kinds (SIREN_KLOSS_* of include/siren_mri_amd.h)
KLOSS_ASINH = 0
KLOSS_CUBIC = 1
KLOSS_SMAPE = 2
KLOSS_L1 = 3
KLOSS_PERP = 4
KLOSS_LOG = 5
KLOSS_KINDS = 6


class SirenKlossDesc(ctypes.Structure):
    """Mirror of ``siren_kloss_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("weight", ctypes.c_float),
        ("eps", ctypes.c_float),
        ("scale", ctypes.c_float),
        ("divisor", ctypes.c_float),
        ("mag_weight", ctypes.c_float),
        ("phase_weight", ctypes.c_float),
    ]


class SirenKiftDesc(ctypes.Structure):
    """Mirror of ``siren_kift_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("img_weight", ctypes.c_float),
        ("l1_weight", ctypes.c_float),
        ("kspace_weight", ctypes.c_float),
    ]


# sides of siren_kspace_fft2 and siren_kspace_ift_loss_* (one workgroup transforms one slice in LDS)
KFFT_SIDES = (8, 16, 32, 64, 128)

HYPER_MAXG = 32
HYPER_MAXD = 4


class SirenHyperDesc(ctypes.Structure):
    """Mirror of ``siren_hyper_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("heads", ctypes.c_int32),
        ("depth", ctypes.c_int32),
        ("rows", ctypes.c_int32),
        ("in_features", ctypes.c_int32),
        ("hidden", ctypes.c_int32),
        ("out_features", ctypes.c_int32 * HYPER_MAXG),
        ("weight", ctypes.c_void_p * (HYPER_MAXG * (HYPER_MAXD + 1))),
        ("bias", ctypes.c_void_p * (HYPER_MAXG * (HYPER_MAXD + 1))),
    ]


ADAM_MAX_TENSORS = 48


class SirenAdamDesc(ctypes.Structure):
    """Mirror of ``siren_adam_desc`` (include/siren_mri_amd.h)."""

    _fields_ = [
        ("num_tensors", ctypes.c_int32),
        ("maximize", ctypes.c_int32),
        ("lr", ctypes.c_float),
        ("beta1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("eps", ctypes.c_float),
        ("weight_decay", ctypes.c_float),
        ("one_minus_beta1", ctypes.c_float),
        ("one_minus_beta2", ctypes.c_float),
        ("step_size", ctypes.c_float),
        ("bias_correction2_sqrt", ctypes.c_float),
        ("numel", ctypes.c_int64 * ADAM_MAX_TENSORS),
        ("param", ctypes.c_void_p * ADAM_MAX_TENSORS),
        ("grad", ctypes.c_void_p * ADAM_MAX_TENSORS),
        ("exp_avg", ctypes.c_void_p * ADAM_MAX_TENSORS),
        ("exp_avg_sq", ctypes.c_void_p * ADAM_MAX_TENSORS),
        ("dev_scalars", ctypes.c_void_p),
        ("dev_steps", ctypes.c_void_p),
        ("dev_table", ctypes.c_void_p),
        ("table_n", ctypes.c_int64),

    ]


class NativeError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def _signatures():
    """symbol -> (restype, argtypes) of every function include/siren_mri_amd.h declares."""
    ci, i64, f32, f64, vp, cstr = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                                   ctypes.c_char_p)
    pvp, pi64 = ctypes.POINTER(vp), ctypes.POINTER(i64)
    P, LP, HP = ctypes.POINTER(SirenMLPDesc), ctypes.POINTER(SirenLossDesc), ctypes.POINTER(SirenHyperDesc)
    KP, AP = ctypes.POINTER(SirenKlossDesc), ctypes.POINTER(SirenAdamDesc)
    KIP = ctypes.POINTER(SirenKiftDesc)
    fwd = [P, vp, vp, vp, i64, vp, i64, vp]                   # desc, x, y, saved, bytes, workspace, bytes, stream
    bwd = [P, vp, vp, vp, i64, vp, i64, pvp, pvp, vp, vp]     # desc, x, dy, saved, .., dweight, dbias, dx, stream
    return {
        "siren_mlp_check": (ci, [P]),
        "siren_mlp_saved_bytes": (i64, [P]),
        "siren_mlp_workspace_bytes": (i64, [P]),
        "siren_mlp_forward": (ci, fwd),
        "siren_mlp_backward": (ci, bwd),
        "siren_mlp_loss_check": (ci, [P, LP]),
        "siren_mlp_forward_loss": (ci, [P, LP, vp, vp, vp, i64, vp, i64, vp]),
        "siren_mlp_backward_ex": (ci, [P, vp, vp, vp, vp, i64, vp, i64, pvp, pvp, vp, vp]),
        "siren_mlp_backward_plan": (i64, [P, ci, cstr, i64]),
        "siren_mlp64_saved_bytes": (i64, [P]),
        "siren_mlp64_workspace_bytes": (i64, [P]),
        "siren_mlp64_forward": (ci, fwd),
        "siren_mlp64_backward": (ci, bwd),
        "siren_hyper_saved_bytes": (i64, [HP]),
        "siren_hyper_workspace_bytes": (i64, [HP]),
        "siren_hyper_forward": (ci, [HP, vp, pvp, vp, i64, vp]),
        "siren_hyper_backward": (ci, [HP, vp, pvp, vp, i64, vp, i64, pvp, pvp, vp, vp]),
        "siren_jvp_saved_bytes": (i64, [P, ci]),
        "siren_jvp_workspace_bytes": (i64, [P, ci]),
        "siren_jvp_forward": (ci, [P, ci, vp, vp, vp, vp, i64, vp, i64, vp]),
        "siren_jvp_backward": (ci, [P, ci, vp, vp, vp, i64, vp, i64, pvp, pvp, vp, vp]),
        "siren_jvp_forward_ex": (ci, [P, ci, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp]),
        "siren_jvp_backward_ex": (ci, [P, ci, vp, vp, vp, i64, vp, i64, pvp, pvp, vp, vp, i64, vp]),
        "siren_jvp_plan": (i64, [P, ci, ci, cstr, i64]),
        "siren_timing_enable": (ci, [ci, ci]),
        "siren_timing_collect": (ci, [ctypes.POINTER(f64), pi64]),
        "siren_timing_disable": (None, []),
        "siren_config_set": (ci, [cstr, i64]),
        "siren_config_get": (i64, [cstr]),
        "siren_adam_step": (ci, [AP, vp]),
        "siren_adam_num_blocks": (i64, [AP]),
        "siren_adam_scalars": (ci, [vp, f64, f64, f64, vp, vp]),
        "siren_adam_scalars_table": (ci, [vp, vp, i64, vp, vp]),
        "siren_sse_workspace_bytes": (i64, []),
        "siren_enc_workspace_bytes": (i64, []),
        "siren_conv_wrw_workspace_bytes": (i64, [ci, ci, ci]),
        "siren_conv_wrw_k5": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, i64, vp]),
        "siren_conv_fwd_k5": (ci, [vp, vp, vp, ci, vp, ci, ci, ci, ci, vp]),
        "siren_conv_dgrad_k5_fused": (ci, [ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, i64, vp]),
        "siren_conv_fwd_k5_res": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
        "siren_conv_check": (ci, [ci, ci, ci, ci, ci, ci, ci]),
        "siren_conv_fwd": (ci, [vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp]),
        "siren_conv_wrw_ws_bytes": (i64, [ci, ci, ci, ci, ci, ci]),
        "siren_conv_wrw": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, i64, vp]),
        "siren_enc_bias_relu": (ci, [vp, vp, i64, ci, vp]),
        "siren_enc_prep": (ci, [ci, pvp, pvp, pi64, pvp, pvp, pvp, vp]),
        "siren_sumsq_workspace_bytes": (i64, [i64]),
        "siren_sumsq_forward": (ci, [ci, pvp, pi64, vp, vp, i64, vp]),
        "siren_sumsq_backward": (ci, [ci, pvp, pi64, vp, pvp, vp]),
        "siren_enc_relu_bwd": (ci, [vp, vp, vp, vp, vp, i64, ci, vp, i64, vp]),
        "siren_enc_res_fwd": (ci, [vp, vp, vp, vp, i64, ci, vp]),
        "siren_enc_res_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, i64, ci, vp, i64, vp]),
        "siren_enc_pixfc_fwd": (ci, [vp, vp, vp, vp, vp, ci, i64, ci, vp, i64, vp]),
        "siren_enc_pixfc_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, i64, ci, vp, i64, vp]),
        "siren_sse_forward": (ci, [vp, vp, vp, i64, i64, f32, vp, vp, vp, i64, vp]),
        "siren_sse_backward": (ci, [vp, vp, i64, i64, vp, f32, vp, vp]),
        "siren_dc_forward": (ci, [vp, vp, vp, i64, i64, ci, f32, vp, vp]),
        "siren_dc_backward": (ci, [vp, vp, i64, i64, ci, f32, vp, vp]),
        "siren_kspace_sse_forward": (ci, [vp, vp, vp, vp, vp, i64, i64, ci, f32, f32, vp, vp, vp, i64, vp]),
        "siren_kspace_sse_backward": (ci, [vp, vp, vp, i64, i64, ci, f32, vp, f32, vp, vp]),
        "siren_kspace_loss_forward": (ci, [ci, KP, vp, vp, vp, vp, i64, i64, ci, f32, vp, vp, i64, vp]),
        "siren_kspace_loss_backward": (ci, [ci, KP, vp, vp, vp, vp, i64, i64, ci, f32, vp, vp, vp]),
        "siren_kspace_fft2": (ci, [vp, vp, i64, ci, ci, vp]),
        "siren_kspace_ift_loss_forward": (ci, [KIP, vp, vp, vp, vp, vp, i64, i64, ci, f32, vp, vp, i64, vp]),
        "siren_kspace_ift_loss_backward": (ci, [KIP, vp, vp, vp, vp, vp, i64, i64, ci, f32, vp, vp, vp]),
        "siren_sdf_loss_forward": (ci, [vp, vp, vp, vp, i64, ci, vp, vp, i64, vp]),
        "siren_sdf_loss_backward": (ci, [vp, vp, vp, vp, i64, ci, vp, vp, vp, vp]),
        "siren_wave_loss_forward": (ci, [vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, i64, vp]),
        "siren_wave_loss_backward": (ci, [vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]),
        "siren_helmholtz_loss_forward": (ci, [vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, i64, vp]),
        "siren_helmholtz_loss_backward": (ci, [vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]),
        "siren_fourier_features": (ci, [vp, vp, i64, ci, ci, vp, vp]),
        "siren_sincos_f32": (ci, [vp, vp, vp, i64, ci, vp]),
        "siren_last_error": (cstr, []),
        "siren_version": (cstr, []),
    }


_SIGNATURES = _signatures()
# Every symbol include/siren_mri_amd.h declares (checked by tests/test_native_abi.py).
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _declare(lib):
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes


def load_library(path: str | None = None):
    """Load (once) and return the native library. Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise NativeError(
                f"siren_mri_amd: native library {p} not found. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950).")
        lib = ctypes.CDLL(p)
        _declare(lib)
        if path is None:
            _lib = lib
        return lib


def lib():
    return _lib if _lib is not None else load_library()


_OPTIONS_EPOCH = [0]


def options_epoch() -> int:
    """Bumped by every set_option (buffer sizes may depend on the options)."""
    return _OPTIONS_EPOCH[0]


def set_option(key: str, value: int) -> None:
    """siren_config_set: process-wide execution options (e.g. "fused_forward")."""
    _OPTIONS_EPOCH[0] += 1
    if lib().siren_config_set(key.encode(), int(value)) != 0:
        raise NativeError(last_error())


def get_option(key: str) -> int:
    v = lib().siren_config_get(key.encode())
    if v < 0:
        raise NativeError(f"unknown option {key!r}")
    return int(v)


def last_error() -> str:
    return lib().siren_last_error().decode(errors="replace")


def check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"siren_mri_amd.{what} failed ({rc}): {last_error()}")


def precision_code(precision) -> int:
    if isinstance(precision, int):
        return precision
    try:
        return PRECISIONS[str(precision).lower()]
    except KeyError:
        raise ValueError(f"unknown precision {precision!r}; use 'fp32' or 'bf16'") from None


def stream_handle(device: torch.device) -> int:
    """The current HIP stream of `device` as an integer (torch's raw getter: no Stream object)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


_WORKSPACES: dict = {}


def _stream_workspace(kind: str, device) -> torch.Tensor:
    """The zero-initialised `siren_<kind>_workspace_bytes()` buffer of (device, current stream), made once:
    two launches that may run concurrently never share one."""
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None:
        nbytes = getattr(lib(), f"siren_{kind}_workspace_bytes")()
        ws = _WORKSPACES[key] = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
    return ws


def sse_workspace(device) -> torch.Tensor:
    """The per-(device, stream) partial-sum / hand-off-counter workspace of the deterministic loss
    reductions (siren_sse_workspace_bytes; zeroed once, left zeroed by every launch)."""
    return _stream_workspace("sse", device)


def enc_workspace(device) -> torch.Tensor:
    """Per-(device, stream) workspace of the encoder passes (siren_enc_workspace_bytes; zeroed once). The
    partial sums at its front are scratch that launches overwrite; only the ticket word behind them
    (byte ENC_WS_FLOATS * 4) must stay zero, and every launch that takes it puts it back to zero."""
    return _stream_workspace("enc", device)


def _fill_desc(dims, weight_ptrs, bias_ptrs, ff_ptr, ff_in, *, w0, prec, outermost_linear, weights_batched, batch,
               rows_per_batch) -> SirenMLPDesc:
    d = SirenMLPDesc()
    d.num_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    d.outermost_linear = 1 if outermost_linear else 0
    d.prec = int(prec)
    d.weights_batched = 1 if weights_batched else 0
    d.w0 = float(w0)
    d.batch = int(batch)
    d.rows_per_batch = int(rows_per_batch)
    for l in range(d.num_layers):
        d.weight[l] = weight_ptrs[l]
        d.bias[l] = bias_ptrs[l]
    if ff_ptr is not None:  # Fourier-feature input: x holds the raw coordinates
        d.ff_B = ff_ptr
        d.ff_in = int(ff_in)
    return d


def make_desc(dims, weights, biases, *, w0: float, prec: int, outermost_linear: bool,
              weights_batched: bool, batch: int, rows_per_batch: int, ff_B=None) -> SirenMLPDesc:
    L = len(dims) - 1
    if not 2 <= L <= MAX_LAYERS:
        raise ValueError(f"siren_mri_amd: {L} linear layers outside [2, {MAX_LAYERS}]")
    return _fill_desc(dims, [w.data_ptr() for w in weights[:L]], [b.data_ptr() for b in biases[:L]],
                      ff_B.data_ptr() if ff_B is not None else None, ff_B.shape[0] if ff_B is not None else 0,
                      w0=w0, prec=prec, outermost_linear=outermost_linear, weights_batched=weights_batched,
                      batch=batch, rows_per_batch=rows_per_batch)


def describe_only(dims, *, prec: int, outermost_linear: bool = True, weights_batched: bool = False,
                  batch: int = 1, rows_per_batch: int = 1, w0: float = 30.0, ff_in: int = 0):
    """Descriptor with fake (aligned, non-null) pointers — for size queries and validation."""
    L = len(dims) - 1
    return _fill_desc(dims, [256 * (l + 1) for l in range(L)], [256 * (l + 1) + 64 for l in range(L)],
                      256 * (L + 2) if ff_in else None, ff_in, w0=w0, prec=prec, outermost_linear=outermost_linear,
                      weights_batched=weights_batched, batch=batch, rows_per_batch=rows_per_batch)


class KernelTimer:
    """Context manager: HIP-event timing of every launch of one kernel class (see
    siren_timing_enable in include/siren_mri_amd.h)."""

    def __init__(self, kernel_class: int, max_launches: int = 4096):
        self.kernel_class = kernel_class
        self.max_launches = max_launches
        self.total_ms = 0.0
        self.launches = 0

    def __enter__(self):
        check(lib().siren_timing_enable(self.kernel_class, self.max_launches), "siren_timing_enable")
        return self

    def __exit__(self, *exc):
        tot = ctypes.c_double(0.0)
        n = ctypes.c_int64(0)
        try:
            check(lib().siren_timing_collect(ctypes.byref(tot), ctypes.byref(n)), "siren_timing_collect")
        finally:
            lib().siren_timing_disable()
        self.total_ms = tot.value
        self.launches = n.value
        return False

    def reset(self):
        """Drop the launches recorded so far and start again (same class and capacity)."""
        lib().siren_timing_disable()
        check(lib().siren_timing_enable(self.kernel_class, self.max_launches), "siren_timing_enable")

    @property
    def avg_ms(self) -> float:
        return self.total_ms / self.launches if self.launches else float("nan")
