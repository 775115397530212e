"""Dense evaluation of a fitted signed-distance model, and the mesh extracted from it (the role of
sdf_meshing.py of jonbmartin/siren_mri, which follows DeepSDF's).

sdf_volume(model, N, max_batch)   the model on the N^3 grid of [-1, 1]^3 as an [N, N, N] float32 CPU
    tensor: volume[i0, i1, i2] is the model at (-1 + 2 i_k / (N - 1))_k, the reference's sample order
    (= dataio.get_mgrid(N, dim=3) reshaped). Runs under no_grad through the model's own forward (the
    native stack on a GPU) in chunks of max_batch rows.
create_mesh(model, filename, N, max_batch)   marching cubes at level 0 on that volume, written to
    filename + ".ply". Needs scikit-image and plyfile, which are optional: without them it raises an
    ImportError that names them (sdf_volume needs neither).
"""
from __future__ import annotations

import numpy as np
import torch

from .dataio import get_mgrid


def sdf_volume(model, N=256, max_batch=64 ** 3):
    """[N, N, N] float32 CPU tensor of the model's output on get_mgrid(N, dim=3)."""
    dev = next(model.parameters()).device
    grid = get_mgrid(N, dim=3)
    out = torch.empty(grid.shape[0], dtype=torch.float32)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for head in range(0, grid.shape[0], max_batch):
                chunk = grid[head:head + max_batch].to(dev)
                y = model({"coords": chunk[None]})["model_out"]
                out[head:head + chunk.shape[0]] = y.reshape(-1).float().cpu()
    finally:
        model.train(was_training)
    return out.view(N, N, N)


def _mesh_backends():
    missing = []
    try:
        import skimage.measure as measure
    except ImportError:
        measure = None
        missing.append("scikit-image (skimage)")
    try:
        import plyfile
    except ImportError:
        plyfile = None
        missing.append("plyfile")
    if missing:
        raise ImportError("siren_mri_amd.sdf_meshing.create_mesh needs " + " and ".join(missing) + ", which "
                          "are not installed; sdf_meshing.sdf_volume gives the dense volume without them")
    return measure, plyfile


def create_mesh(model, filename, N=256, max_batch=64 ** 3, offset=None, scale=None):
    """The zero level set of the model on the N^3 grid as a triangle mesh in filename + '.ply'
    (vertices in the model's coordinates, then / scale and - offset if given)."""
    measure, plyfile = _mesh_backends()
    volume = sdf_volume(model, N, max_batch).numpy()
    voxel = 2.0 / (N - 1)
    marching_cubes = getattr(measure, "marching_cubes", None) or measure.marching_cubes_lewiner
    try:
        verts, faces, _, _ = marching_cubes(volume, level=0.0, spacing=(voxel,) * 3)
    except (ValueError, RuntimeError):  # no zero crossing in the volume: an empty mesh, as the reference writes
        verts, faces = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    points = verts - 1.0
    if scale is not None:
        points = points / scale
    if offset is not None:
        points = points - offset
    vert_el = np.zeros(points.shape[0], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    vert_el["x"], vert_el["y"], vert_el["z"] = points[:, 0], points[:, 1], points[:, 2]
    face_el = np.zeros(faces.shape[0], dtype=[("vertex_indices", "i4", (3,))])
    face_el["vertex_indices"] = faces
    plyfile.PlyData([plyfile.PlyElement.describe(vert_el, "vertex"),
                     plyfile.PlyElement.describe(face_el, "face")]).write(filename + ".ply")
