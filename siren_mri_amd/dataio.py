"""Data layouts and producers feeding the SIREN path (dataio.py of jonbmartin/siren_mri).

Restated from the reference:
  get_mgrid                  dataio.py:28-48   row-major grid, x_k = 2 i_k/(S_k - 1) - 1
  lin2img                    dataio.py:51-63   [B, N, C] -> [B, C, H, W]
  Camera                     dataio.py:474-492 (cameraman, siren_mri_amd/assets/camera512_u8.npz)
  MRIImageDomain             dataio.py:507-525 (data/IRData.mat -> siren_mri_amd/assets/irdata.npz)
  Implicit2DWrapper          dataio.py:746-827 (PIL bilinear resize, /255, Normalize; sobel /
                                                laplace ground truth via scipy.ndimage)
  ImageGeneralizationWrapper dataio.py:861-986 (CS-Cartesian masks, conv_cnp inputs)
  FastMRIBrainKspace layout  dataio.py:585-664 (fftshift(fft2(slice)) stacked [H, W, 2])
  PointCloud                 dataio.py:401-453 (oriented point cloud -> on- / off-surface SDF batches;
                                                write_synthetic_point_cloud writes an analytic one)
  gaussian, WaveSource       dataio.py:115-121, 305-398 (wave-equation batches: (t, x, y) rows, source
                                                pulse, Dirichlet mask, squared slowness)
  SingleHelmholtzSource      dataio.py:220-302 (Helmholtz batches: (x0, x1) rows, the complex source, squared
                                                slowness, wavenumber, the closed-form field)

Deviation (bug 0.7): fastMRI .h5 volumes are not available, so
SyntheticMRIKspace produces k-space of seeded phantoms with the same [H, W, 2] float32 layout:
the reference tree's own IRData slices under the 8 flips/rotations and seeded
random-ellipse phantoms; the CS mask RNG is seeded.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

# data assets shipped with the package (tools/make_assets.py, tests/golden/make_golden.py)
ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")


def get_mgrid(sidelen, dim=2):
    if isinstance(sidelen, int):
        sidelen = dim * (sidelen,)
    axes = [np.arange(s, dtype=np.float32) / np.float32(max(s - 1, 1)) for s in sidelen]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).astype(np.float32)
    grid = (grid - np.float32(0.5)) * np.float32(2.0)
    return torch.from_numpy(np.ascontiguousarray(grid)).view(-1, dim)


def lin2img(tensor, image_resolution=None):
    b, n, c = tensor.shape
    if image_resolution is None:
        h = w = int(np.sqrt(n))
    else:
        h, w = image_resolution
    return tensor.permute(0, 2, 1).reshape(b, c, h, w)


def camera_image() -> np.ndarray:
    """The 512x512 uint8 cameraman (the image skimage.data.camera() returns)."""
    path = os.path.join(ASSETS, "camera512_u8.npz")
    with np.load(path, allow_pickle=False) as d:
        return d["img"]


class Camera(Dataset):
    def __init__(self, downsample_factor=1):
        super().__init__()
        from PIL import Image
        self.img = Image.fromarray(camera_image())
        self.img_channels = 1
        self.downsample_factor = downsample_factor
        if downsample_factor > 1:
            size = (int(512 / downsample_factor),) * 2
            self.img_downsampled = self.img.resize(size, Image.LANCZOS)

    def __len__(self):
        return 1

    def __getitem__(self, idx):
        return self.img_downsampled if self.downsample_factor > 1 else self.img


def irdata() -> np.ndarray:
    """IRData [128, 128, 9] float32 (np.squeeze of data/IRData.mat's 'IRData', dataio.py:519-520)."""
    with np.load(os.path.join(ASSETS, "irdata.npz"), allow_pickle=False) as d:
        return d["IRData"]


class MRIImageDomain(Dataset):
    """dataio.py:507-525: the 9 IRData magnitude slices, item = [128, 128] float32. `split` is
    checked as in the reference and otherwise unused (the reference reads one file for all)."""

    def __init__(self, split="train", downsampled=False):
        assert split in ["train", "test", "val", "val_small"], "Unknown split"
        self.img_channels = 1
        self.downsampled = downsampled
        self.data = irdata()

    def __len__(self):
        return self.data.shape[2]

    def __getitem__(self, idx):
        return np.squeeze(self.data[:, :, idx])


def irdata_image(idx: int = 0, side: int = 256) -> torch.Tensor:
    """Config C2's fitting target (harness-defined since BASELINE.json says
    256x256 and IRData is 128x128): slice idx -> / max -> x2 - 1 -> bilinear resize to side^2
    (F.interpolate, align_corners=False). Returns [side*side, 1] float32 in the flattened
    get_mgrid row order (row-major over (i, j))."""
    import torch.nn.functional as F
    sl = torch.from_numpy(np.ascontiguousarray(MRIImageDomain()[idx]))
    sl = sl / sl.max() * 2 - 1
    img = F.interpolate(sl[None, None], size=(side, side), mode="bilinear", align_corners=False)
    return img.reshape(-1, 1).contiguous()


def smooth_random_image(side: int, n_waves: int = 32, seed: int = 0, max_freq: float = 16.0) -> np.ndarray:
    """Synthetic throughput target: sum of random 2-D sinusoids in [-1, 1]."""
    rs = np.random.RandomState(seed)
    y, x = np.meshgrid(np.linspace(0, 1, side), np.linspace(0, 1, side), indexing="ij")
    img = np.zeros((side, side), np.float64)
    for _ in range(n_waves):
        fx, fy = rs.uniform(0, max_freq, size=2)
        ph = rs.uniform(0, 2 * np.pi)
        img += np.sin(2 * np.pi * (fx * x + fy * y) + ph)
    img = img - img.min()
    img = img / max(img.max(), 1e-12)
    return (img * 2 - 1).astype(np.float32)


def _image_transform(img, sidelength):
    """Resize(sidelength) -> ToTensor -> Normalize(0.5, 0.5) for a PIL image."""
    from PIL import Image
    if isinstance(img, Image.Image):
        if tuple(img.size[::-1]) != tuple(sidelength):
            img = img.resize((sidelength[1], sidelength[0]), Image.BILINEAR)
        a = np.asarray(img, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        else:
            a = a.transpose(2, 0, 1)
        a = a / np.float32(255.0)
    else:
        a = np.asarray(img, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
    return torch.from_numpy((a - np.float32(0.5)) / np.float32(0.5))


class Implicit2DWrapper(Dataset):
    """Image -> {'coords': grid}, {'img': [N, C] (+ 'gradients' / 'laplace')} (dataio.py:746-812)."""

    def __init__(self, dataset, sidelength=None, compute_diff=None, image=True, kspace=False):
        if isinstance(sidelength, int):
            sidelength = (sidelength, sidelength)
        self.sidelength = sidelength
        self.image = image
        self.compute_diff = compute_diff
        self.dataset = dataset
        self.mgrid = get_mgrid(sidelength)

    def __len__(self):
        return len(self.dataset)

    def _transform(self, item):
        if self.image:
            return _image_transform(item, self.sidelength)
        # k-space arrays [H, W, 2]: ToTensor -> [2, H, W]; Normalize(0, 0.5) -> x2
        a = np.asarray(item, dtype=np.float32).transpose(2, 0, 1)
        return torch.from_numpy(np.ascontiguousarray(a)) / 0.5

    def __getitem__(self, idx):
        import scipy.ndimage
        img = self._transform(self.dataset[idx])
        gt = {}
        if self.compute_diff == "gradients":
            img = img * 1e1
        elif self.compute_diff == "laplacian":
            img = img * 1e4
        if self.compute_diff in ("gradients", "all"):
            gx = scipy.ndimage.sobel(img.numpy(), axis=1).squeeze(0)[..., None]
            gy = scipy.ndimage.sobel(img.numpy(), axis=2).squeeze(0)[..., None]
            gt["gradients"] = torch.cat((torch.from_numpy(gx).reshape(-1, 1),
                                         torch.from_numpy(gy).reshape(-1, 1)), dim=-1)
        if self.compute_diff in ("laplacian", "all"):
            lap = scipy.ndimage.laplace(img.numpy()).squeeze(0)[..., None]
            gt["laplace"] = torch.from_numpy(lap).view(-1, 1)
        channels = img.shape[0]
        gt["img"] = img.permute(1, 2, 0).reshape(-1, channels)
        return {"idx": idx, "coords": self.mgrid}, gt

    def get_item_small(self, idx):
        img = self._transform(self.dataset[idx])
        spatial = img.clone()
        channels = img.shape[0]
        return spatial, img.permute(1, 2, 0).reshape(-1, channels), {"img": img.permute(1, 2, 0).reshape(-1, channels)}


def _ellipse_phantom(res: int, rs: np.random.RandomState, n_ellipses: int = 8) -> np.ndarray:
    y, x = np.meshgrid(np.linspace(-1, 1, res), np.linspace(-1, 1, res), indexing="ij")
    img = np.zeros((res, res), np.float64)
    for i in range(n_ellipses):
        a, b = rs.uniform(0.1, 0.8, size=2) if i else (0.85, 0.7)
        cx, cy = rs.uniform(-0.4, 0.4, size=2) if i else (0.0, 0.0)
        th = rs.uniform(0, np.pi)
        val = rs.uniform(-0.4, 1.0) if i else 1.0
        xr = (x - cx) * np.cos(th) + (y - cy) * np.sin(th)
        yr = -(x - cx) * np.sin(th) + (y - cy) * np.cos(th)
        img[(xr / a) ** 2 + (yr / b) ** 2 <= 1] += val
    return img


class SyntheticMRIKspace(Dataset):
    """Seeded synthetic stand-in for FastMRIBrainKspace (bug 0.7): item = float32 [H, W, 2] of
    fftshift(fft2(slice)) stacked real/imag, the reference's layout (dataio.py:654-664).
    Items 0..71 (with irdata=True) are the 9 IRData slices under the 8 flips/rotations of the
    square (normalised to max 1, bilinear-resized when the resolution is not 128); later items
    are seeded random-ellipse phantoms."""

    def __init__(self, n_slices: int = 256, image_resolution=(128, 128), seed: int = 0, irdata: bool = True):
        self.n = n_slices
        self.res = image_resolution
        self.seed = seed
        self.img_channels = 2
        self._ir = globals()["irdata"]() if irdata else None

    def __len__(self):
        return self.n

    def _ir_slice(self, idx):
        sl = self._ir[:, :, idx % 9].astype(np.float64)
        t = idx // 9
        sl = np.rot90(sl, t % 4)
        if t >= 4:
            sl = sl[:, ::-1]
        sl = sl / max(sl.max(), 1e-12)
        if tuple(self.res) != sl.shape:
            import torch.nn.functional as F
            sl = F.interpolate(torch.from_numpy(np.ascontiguousarray(sl))[None, None], size=tuple(self.res),
                               mode="bilinear", align_corners=False)[0, 0].numpy()
        return sl

    def __getitem__(self, idx):
        rs = np.random.RandomState(self.seed * 100003 + idx)
        if self._ir is not None and idx < 72:
            img = self._ir_slice(idx)
        else:
            img = _ellipse_phantom(self.res[0], rs)
        k = np.fft.fftshift(np.fft.fft2(img))
        k = k / max(np.abs(k).max(), 1e-12)
        return np.float32(np.dstack((k.real, k.imag)))


class ImageGeneralizationWrapper(Dataset):
    """conv_cnp inputs with CS-Cartesian sampling (dataio.py:861-986). The row permutation uses
    a per-item seeded RNG (the reference's is unseeded `random.shuffle`)."""

    def __init__(self, dataset, test_sparsity=None, train_sparsity_range=(10, 200),
                 generalization_mode=None, device="cpu", seed: int = 0):
        self.dataset = dataset
        self.sidelength = dataset.sidelength
        self.mgrid = dataset.mgrid
        self.test_sparsity = test_sparsity
        self.train_sparsity_range = train_sparsity_range
        self.generalization_mode = generalization_mode
        self.device = device
        self.seed = seed

    def __len__(self):
        return len(self.dataset)

    def update_test_sparsity(self, test_sparsity):
        self.test_sparsity = test_sparsity

    def get_generalization_in_dict(self, spatial_img, img, idx):
        if self.generalization_mode not in ("conv_cnp", "conv_cnp_test"):
            return {"idx": torch.tensor(idx), "coords": self.mgrid}
        rng = random.Random(self.seed * 1000003 + idx)
        ny = spatial_img.size(1)
        if self.test_sparsity == "full":
            mask = torch.ones_like(spatial_img)
        elif self.test_sparsity == "half":
            mask = torch.ones_like(spatial_img)
            mask[:, ny // 2:, :] = 0
        elif self.test_sparsity in ("CS_cartesian", "CS_cartesian_noACS"):
            rows = list(range(ny))
            rng.shuffle(rows)
            mask = torch.zeros_like(spatial_img)
            mask[:, rows[: int(0.3333 * ny)], :] = 1
            if self.test_sparsity == "CS_cartesian":
                mask[:, int(ny / 2 - 4):int(ny / 2 + 4), :] = 1
        else:
            raise NotImplementedError(f"test_sparsity={self.test_sparsity!r}")
        img_sparse = mask * spatial_img
        z = torch.fft.ifft2(img_sparse[0] + 1j * img_sparse[1])
        ift = torch.stack((torch.abs(z), torch.angle(z)))
        return {"idx": torch.tensor(idx), "coords": self.mgrid, "img_sparse": img_sparse,
                "ift_zfilled": ift, "dc_mask": mask}

    def __getitem__(self, idx):
        spatial_img, img, gt = self.dataset.get_item_small(idx)
        in_dict = self.get_generalization_in_dict(spatial_img, img, idx)
        if "dc_mask" in in_dict:
            gt["dc_mask"] = in_dict["dc_mask"]
        in_dict = {k: v.to(self.device) for k, v in in_dict.items()}
        gt = {k: v.to(self.device) for k, v in gt.items()}
        return in_dict, gt


class PointCloud(Dataset):
    """An oriented point cloud as signed-distance training batches (dataio.py:401-453): the file holds
    `x y z nx ny nz` rows (np.genfromtxt); the points are centred on their mean and scaled to [-1, 1] by
    the global min/max (keep_aspect_ratio) or per axis. An item is on_surface_points random surface
    points (sdf 0, their normals) followed by as many uniform points of the cube (sdf -1, normals -1),
    drawn from the global numpy generator: np.random.choice, then np.random.uniform."""

    def __init__(self, pointcloud_path, on_surface_points, keep_aspect_ratio=True):
        super().__init__()
        point_cloud = np.genfromtxt(pointcloud_path)
        coords = point_cloud[:, :3]
        self.normals = point_cloud[:, 3:]
        coords -= np.mean(coords, axis=0, keepdims=True)
        if keep_aspect_ratio:
            coord_max, coord_min = np.amax(coords), np.amin(coords)
        else:
            coord_max = np.amax(coords, axis=0, keepdims=True)
            coord_min = np.amin(coords, axis=0, keepdims=True)
        self.coords = (coords - coord_min) / (coord_max - coord_min)
        self.coords -= 0.5
        self.coords *= 2.0
        self.on_surface_points = on_surface_points

    def __len__(self):
        return self.coords.shape[0] // self.on_surface_points

    def __getitem__(self, idx):
        n_on = n_off = self.on_surface_points
        rand_idcs = np.random.choice(self.coords.shape[0], size=n_on)
        off_surface_coords = np.random.uniform(-1, 1, size=(n_off, 3))
        sdf = np.zeros((n_on + n_off, 1))
        sdf[n_on:, :] = -1
        coords = np.concatenate((self.coords[rand_idcs, :], off_surface_coords), axis=0)
        normals = np.concatenate((self.normals[rand_idcs, :], np.ones((n_off, 3)) * -1), axis=0)
        return ({"coords": torch.from_numpy(coords).float()},
                {"sdf": torch.from_numpy(sdf).float(), "normals": torch.from_numpy(normals).float()})


TORUS_RADII = (0.6, 0.25)  # write_synthetic_point_cloud's torus: centre-line and tube radius
SPHERE_RADIUS = 0.6


def write_synthetic_point_cloud(path, shape="torus", n=20000, seed=0):
    """Write an analytic oriented point cloud as `x y z nx ny nz` text rows (.xyz), the input of
    PointCloud: n points uniform by area on the torus (sqrt(x^2 + y^2) - R)^2 + z^2 = r^2 with
    (R, r) = TORUS_RADII (the tube angle v by rejection against the area density R + r cos v), or on the
    sphere of SPHERE_RADIUS, with their exact outward unit normals. Returns the [n, 6] float64 array."""
    rs = np.random.RandomState(seed)
    if shape == "sphere":
        nrm = rs.standard_normal((n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        pts = SPHERE_RADIUS * nrm
    elif shape == "torus":
        R, r = TORUS_RADII
        v = np.empty(0)
        while v.size < n:
            cand = rs.uniform(0.0, 2 * np.pi, size=2 * n)
            keep = rs.uniform(0.0, R + r, size=2 * n) < R + r * np.cos(cand)
            v = np.concatenate((v, cand[keep]))
        v = v[:n]
        u = rs.uniform(0.0, 2 * np.pi, size=n)
        nrm = np.stack((np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)), axis=1)
        pts = np.stack((R * np.cos(u), R * np.sin(u), np.zeros(n)), axis=1) + r * nrm
    else:
        raise ValueError(f"unknown shape {shape!r}; 'torus' or 'sphere'")
    cloud = np.concatenate((pts, nrm), axis=1)
    np.savetxt(path, cloud, fmt="%.12f")
    return cloud


def gaussian(x, mu=(0, 0), sigma=1e-4, d=2):
    """The isotropic d-dimensional Gaussian density of variance sigma at the rows of the CPU tensor x
    [n, d] around mu, evaluated in numpy as the reference does (dataio.py:115-121) and returned as a
    float32 tensor [n]."""
    pts = x.numpy()
    centre = mu.numpy() if isinstance(mu, torch.Tensor) else mu
    exponent = -0.5 * ((pts - centre) ** 2).sum(1)
    peak = 1 / np.sqrt(sigma ** d * (2 * np.pi) ** d)
    return torch.from_numpy(peak * np.exp(exponent / sigma)).float()


class WaveSource(Dataset):
    """Training batches of the wave-equation experiment (dataio.py:305-398): one item is sidelength^2 rows
    (t, x, y), uniform in space, whose last N_src_samples rows are drawn in a disc around the source, with
    the ground truth of loss_functions.wave_pml: the Gaussian source pulse as boundary values, the
    Dirichlet mask of the rows at the start time, and the squared slowness.

    pretrain: every row within 1e-3 of the start time and in the mask; after 2000 items the data set
    switches itself to training and restarts its counter. Training: t uniform in [0, 0.4 counter / 1e5),
    so the time window grows with the items drawn, the last 2 N_src_samples rows at the start time.
    The constructor seeds torch's global generator with 0 and an item draws r, phi, the coordinates and
    the times from it in that order, which makes the coordinates those of the reference.

    velocity: 'uniform' (slowness 1), or a region of velocity 2 (slowness 1/4): 'square' |x|, |y| < 0.3,
    'circle' radius 0.1, tested on the two spatial columns (deviation 14: the reference's
    two branches raise)."""

    def __init__(self, sidelength, velocity="uniform", source_coords=(0., 0., 0.), pretrain=False):
        super().__init__()
        torch.manual_seed(0)
        self.pretrain = pretrain
        self.sidelength = sidelength
        self.mgrid = get_mgrid(self.sidelength).detach()
        self.velocity = velocity
        self.N_src_samples = 1000
        self.sigma = 5e-4
        self.source_coords = torch.tensor(list(source_coords)).view(-1, 3)
        self.counter = 0
        self.full_count = 100e3

    def __len__(self):
        return 1

    def get_squared_slowness(self, coords):
        """[n] squared slowness at rows whose last two columns are (x, y)."""
        x, y = coords[..., -2], coords[..., -1]
        if self.velocity == "square":
            inside = (torch.abs(x) < 0.3) & (torch.abs(y) < 0.3)
        elif self.velocity == "circle":
            inside = torch.sqrt(x ** 2 + y ** 2) < 0.1
        else:
            return torch.ones_like(x)
        perturbation = 2.
        return torch.where(inside, torch.full_like(x, 1. / perturbation ** 2), torch.ones_like(x))

    def __getitem__(self, idx):
        start_time = self.source_coords[0, 0]
        rows, n_src = self.sidelength ** 2, self.N_src_samples

        # the source's disc, uniform by area: the first two draws
        r = 5e2 * self.sigma * torch.rand(n_src, 1).sqrt()
        phi = 2 * np.pi * torch.rand(n_src, 1)
        disc = torch.cat((r * torch.cos(phi) + self.source_coords[0, 1],
                          r * torch.sin(phi) + self.source_coords[0, 2]), dim=1)

        space = torch.zeros(rows, 2).uniform_(-1, 1)
        if self.pretrain:
            time = torch.zeros(rows, 1).uniform_(start_time - 0.001, start_time + 0.001)
        else:
            time = torch.zeros(rows, 1).uniform_(0, 0.4 * (self.counter / self.full_count))
        coords = torch.cat((time, space), dim=1)
        coords[-n_src:, 1:] = disc
        if not self.pretrain:
            coords[-2 * n_src:, 0] = start_time

        normalize = 50 * gaussian(torch.zeros(1, 2), mu=torch.zeros(1, 2), sigma=self.sigma, d=2)
        boundary_values = gaussian(coords[:, 1:], mu=self.source_coords[:, 1:], sigma=self.sigma, d=2)[:, None]
        boundary_values /= normalize

        if self.pretrain:
            dirichlet_mask = torch.ones(rows, 1) > 0
        else:
            dirichlet_mask = coords[:, 0, None] == start_time
            boundary_values = torch.where(dirichlet_mask, boundary_values, torch.Tensor([0]))
        boundary_values[boundary_values < 1e-5] = 0.

        squared_slowness = self.get_squared_slowness(coords)[:, None]
        squared_slowness_grid = self.get_squared_slowness(self.mgrid)[:, None]

        self.counter += 1
        if self.pretrain and self.counter == 2000:
            self.pretrain = False
            self.counter = 0

        return {"coords": coords}, {"source_boundary_values": boundary_values, "dirichlet_mask": dirichlet_mask,
                                    "squared_slowness": squared_slowness,
                                    "squared_slowness_grid": squared_slowness_grid}


class SingleHelmholtzSource(Dataset):
    """Training batches of the Helmholtz experiment (dataio.py:220-302): one item is sidelength^2 rows
    (x0, x1) uniform in [-1, 1]^2, whose last N_src_samples rows are drawn in a disc around the source, with
    the ground truth of loss_functions.helmholtz_pml: the complex source (1 + i) times a Gaussian as
    boundary values [n, 2] (values below 1e-5 are 0, which encodes "no source here"), the squared slowness
    as a complex number [n, 2], and the wavenumber 20. The constructor seeds torch's global generator with
    0 and an item draws the coordinates, r and phi from it in that order, which makes the items those of
    the reference.

    velocity: 'uniform' (slowness 1), or a region of velocity 2 (slowness 1/4): 'square' |x0|, |x1| < 0.3,
    'circle' radius 0.1.

    field [sidelength^2, 2] (gt['gt']) is the closed-form comparison solution of the uniform medium on
    get_mgrid(sidelength), 0.25 i H0^(2)(k r + 1e-6) s hx hy per source; it never enters the loss. The Hankel
    function is J0 - i Y0 of torch.special (the reference calls scipy.special.hankel2), evaluated on the
    reference's float32 argument, rounded to complex64 and accumulated in complex64."""

    def __init__(self, sidelength, velocity="uniform", source_coords=(0., 0.)):
        super().__init__()
        torch.manual_seed(0)
        self.sidelength = sidelength
        self.mgrid = get_mgrid(self.sidelength).detach()
        self.velocity = velocity
        self.wavenumber = 20.
        self.N_src_samples = 100
        self.sigma = 1e-4
        self.source = torch.Tensor([1.0, 1.0]).view(-1, 2)
        self.source_coords = torch.tensor(list(source_coords)).view(-1, 2)

        x = self.mgrid[:, 0].view(sidelength, sidelength)
        y = self.mgrid[:, 1].view(sidelength, sidelength)
        hx = hy = 2 / self.sidelength
        field = torch.zeros(sidelength, sidelength, dtype=torch.complex64)
        for i in range(self.source.shape[0]):
            x0, y0 = self.source_coords[i, 0], self.source_coords[i, 1]
            s = complex(float(self.source[i, 0]), float(self.source[i, 1]))
            arg = self.wavenumber * torch.sqrt((x - x0) ** 2 + (y - y0) ** 2) + 1e-6
            # the float32 argument, the two Bessel functions evaluated in float64 on it (as scipy's float32
            # loop does internally), rounded to complex64
            arg = arg.double()
            hankel = torch.complex(torch.special.bessel_j0(arg), -torch.special.bessel_y0(arg)).to(torch.complex64)
            field = field + 0.25j * hankel * s * hx * hy
        self.field = torch.cat((field.real.reshape(-1, 1), field.imag.reshape(-1, 1)), dim=1)

    def __len__(self):
        return 1

    def get_squared_slowness(self, coords):
        """[n, 2] squared slowness (real, imaginary = 0) at the rows (x0, x1)."""
        x, y = coords[..., 0], coords[..., 1]
        if self.velocity == "square":
            inside = (torch.abs(x) < 0.3) & (torch.abs(y) < 0.3)
        elif self.velocity == "circle":
            inside = torch.sqrt(x ** 2 + y ** 2) < 0.1
        else:
            inside = torch.zeros_like(x, dtype=torch.bool)
        perturbation = 2.
        real = torch.where(inside, torch.full_like(x, 1. / perturbation ** 2), torch.ones_like(x))
        return torch.stack((real, torch.zeros_like(real)), dim=-1)

    def __getitem__(self, idx):
        n_src = self.N_src_samples
        coords = torch.zeros(self.sidelength ** 2, 2).uniform_(-1., 1.)
        # the source's disc, uniform by area
        r = 5e2 * self.sigma * torch.rand(n_src, 1).sqrt()
        phi = 2 * np.pi * torch.rand(n_src, 1)
        coords[-n_src:, :] = torch.cat((r * torch.cos(phi) + self.source_coords[0, 0],
                                        r * torch.sin(phi) + self.source_coords[0, 1]), dim=1)

        # the value 0 encodes "no boundary constraint at this coordinate"
        boundary_values = self.source * gaussian(coords, mu=self.source_coords, sigma=self.sigma)[:, None]
        boundary_values[boundary_values < 1e-5] = 0.

        squared_slowness = self.get_squared_slowness(coords)
        squared_slowness_grid = self.get_squared_slowness(self.mgrid)[:, 0, None]

        return {"coords": coords}, {"source_boundary_values": boundary_values, "gt": self.field,
                                    "squared_slowness": squared_slowness,
                                    "squared_slowness_grid": squared_slowness_grid,
                                    "wavenumber": self.wavenumber}
