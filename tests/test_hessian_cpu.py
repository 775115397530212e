"""CPU: the Hessian mode (SIREN_JVP_HESSIAN) of the tangent-stream entry points in the library's
size queries, the TV / FH prior losses and diff_operators.hessian against the reference's recorded
values (tests/golden/priors.npz, written by make_golden_priors.py), and a short CPU run of
experiment_scripts/train_img_inpainting.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import siren_oracle as orc
from siren_mri_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")

# case -> (precision, dims, weights batched, weight sets, rows per set) and the
# (saved, workspace) bytes of orders 1..3 recorded from the commit before the Hessian mode. Every
# per-layer plane (rows x width x 4 or 2 bytes) is a multiple of the layout's 256-byte alignment.
SIZE_CASES = {
    "f32_2x64": ((_native.PREC_F32, [2, 64, 64, 1], False, 1, 256),
                 {1: (409600, 1415168), 2: (540672, 1875968), 3: (409600, 1415168)}),
    "f32_4x256": ((_native.PREC_F32, [2, 256, 256, 256, 256, 1], False, 1, 1024),
                  {1: (13369344, 48857088), 2: (17563648, 64618496), 3: (13369344, 48857088)}),
    "bf16_3in_batched": ((_native.PREC_BF16, [3, 64, 128, 64, 2], True, 2, 512),
                         {1: (3801088, 12386304), 2: (4849664, 15548416), 3: (3801088, 12386304)}),
    "f32_1in": ((_native.PREC_F32, [1, 128, 128, 1], False, 1, 128),
                {1: (327680, 1314816), 2: (458752, 1906688), 3: (327680, 1314816)}),
}


def _describe(case):
    prec, dims, batched, batch, rows = SIZE_CASES[case][0]
    return _native.describe_only(dims, prec=prec, weights_batched=batched, batch=batch, rows_per_batch=rows)


@pytest.mark.parametrize("case", sorted(SIZE_CASES))
def test_hessian_size_queries(case):
    lib = _native.load_library()
    (prec, dims, batched, batch, rows), recorded = SIZE_CASES[case]
    d = _describe(case)
    saved = {o: lib.siren_jvp_saved_bytes(ctypes.byref(d), o) for o in (1, 2, 3, 4)}
    work = {o: lib.siren_jvp_workspace_bytes(ctypes.byref(d), o) for o in (1, 2, 3, 4)}
    assert saved[4] > 0 and work[4] > 0
    C = dims[0]
    pairs = C * (C + 1) // 2
    assert saved[4] == saved[1] + pairs * 4 * batch * rows * sum(dims[1:-1])
    assert work[4] > work[1]
    for o in (1, 2, 3):
        assert (saved[o], work[o]) == recorded[o], f"order {o}"


def test_hessian_mode_rejects_four_inputs():
    lib = _native.load_library()
    d = _native.describe_only([4, 64, 64, 1], prec=_native.PREC_F32, rows_per_batch=256)
    assert lib.siren_jvp_saved_bytes(ctypes.byref(d), 3) > 0
    assert lib.siren_jvp_saved_bytes(ctypes.byref(d), 4) == -1
    assert "in_features <= 3" in _native.last_error()
    d = _native.describe_only([2, 64, 64, 1], prec=_native.PREC_F32, rows_per_batch=256, outermost_linear=False)
    assert lib.siren_jvp_saved_bytes(ctypes.byref(d), 4) == -1
    assert "outermost_linear" in _native.last_error()


# ------------------------------------------------------------------ golden priors
@pytest.fixture(scope="module")
def priors():
    return np.load(os.path.join(G, "priors.npz"), allow_pickle=False)


def _golden_model(d):
    from siren_mri_amd import modules
    m = modules.SingleBVPNet(type="sine", mode="mlp", sidelength=(16, 16), hidden_features=64, num_hidden_layers=1)
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("init/")})
    return m


def test_hessian_matches_reference_on_cpu(priors):
    from siren_mri_amd import diff_operators
    m = _golden_model(priors)
    o = m({"coords": torch.from_numpy(priors["coords"])})
    h, status = diff_operators.hessian(o["model_out"], o["model_in"])
    assert status == 0 and h.shape == (1, 256, 1, 2, 2)
    # second derivatives: the tolerance test_api_cpu.py applies to the Laplacian against its fixture
    assert orc.norm_rel(h.detach(), torch.from_numpy(priors["hessian"])) < 1e-4


@pytest.mark.parametrize("tag", ["tv", "fh"])
def test_prior_losses_match_reference_on_cpu(priors, tag):
    """image_mse_TV_prior / image_mse_FH_prior from the reference's seed: the same random
    coordinates (CPU default generator), loss dicts and parameter gradients. 1e-5 relative for the
    values of the image term and of the first-derivative (TV) prior; 1e-4, test_api_cpu.py's
    tolerance for second derivatives, for the Hessian prior and for the parameter gradients
    (double / triple backward passes)."""
    from siren_mri_amd import loss_functions
    m = _golden_model(priors)
    fn = {"tv": loss_functions.image_mse_TV_prior, "fh": loss_functions.image_mse_FH_prior}[tag]
    o = m({"coords": torch.from_numpy(priors["coords"])})
    torch.manual_seed(2)
    losses = fn(torch.from_numpy(priors["mask"]), 0.5, m, o, {"img": torch.from_numpy(priors["img"])})
    assert sorted(losses) == ["img_loss", "prior_loss"]
    sum(losses.values()).backward()
    assert losses["img_loss"].item() == pytest.approx(float(priors[f"{tag}/img_loss"]), rel=1e-5)
    assert losses["prior_loss"].item() == pytest.approx(float(priors[f"{tag}/prior_loss"]),
                                                        rel=1e-5 if tag == "tv" else 1e-4)
    for k, p in m.named_parameters():
        assert orc.norm_rel(p.grad, torch.from_numpy(priors[f"{tag}_grad/{k}"])) < 1e-4, k


def test_prior_coordinates_follow_the_cpu_generator(priors):
    from siren_mri_amd import loss_functions
    torch.manual_seed(2)
    c = loss_functions._prior_coords(torch.from_numpy(priors["coords"]))
    assert torch.equal(c, torch.from_numpy(priors["coords_rand"]))


# ------------------------------------------------------------------ script
def test_train_img_inpainting_script_on_cpu(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "train_img_inpainting.py"),
           "--logging_root", str(tmp_path), "--experiment_name", "run", "--prior", "FH", "--k1", "0.1",
           "--sparsity", "0.5", "--device", "cpu", "--sidelength", "16", "--num_epochs", "3",
           "--steps_til_summary", "100"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    losses = np.atleast_1d(np.loadtxt(tmp_path / "run" / "checkpoints" / "train_losses_final.txt"))
    assert losses.shape == (3,) and np.all(np.isfinite(losses))
