"""Generate ``tests/golden/occupancy.npz`` by RUNNING THE REFERENCE's grid and network code (build container only).

    DMNERF_REFERENCE=<reference checkout> python tests/golden/make_golden_occupancy.py      # writes tests/golden/occupancy.npz

What ``mesh_main`` (tools/mesh_generator.py:27-63) computes before marching cubes, on grids small enough to store: for dim 5 and
dim 8, one rotated and translated scene transform and the reference's extents (1.9, 7, 7),

  * ``points_<dim>``: the reference's own ``grid_within_bound`` output (tools/visualizer.py:138-155) after the axis swap of
    mesh_generator.py:28-29, reshaped ``[dim^3, 3]``;
  * ``sigma_<C>_<dim>``: ``DM_NeRF.forward(cat[embed(p), embed(0)])[:, 3]`` (:40-51) of the reference's network with the
    numpy-seeded weights of ``oracle.ref_cpu.make_weights`` (seed and gains stored, weights not), C = 14 at both dims, C = 94 at dim 5;
  * ``occ_<C>_<dim>``: ``occupancy_activation`` (:54-60) with near 4, far 15, N_importance 128.

``open3d``, ``trimesh``, ``cv2`` and the plotting modules the reference imports at the top of ``tools/visualizer.py`` are stubbed;
the arithmetic does not use them.  The float32 restatement ``tests/_occupancy_restate.py`` must reproduce the points bit for bit
(also at dim 16 and 33) before anything is written.  The fixture is data only; no reference source travels.
"""
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("DMNERF_REFERENCE")
if not REF:
    sys.exit("set DMNERF_REFERENCE to a checkout of the reference (its tools/visualizer.py and networks/dm_nerf.py are what runs)")
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
for mod in ("imageio", "lpips", "cv2", "skimage", "skimage.metrics", "skimage.measure", "open3d", "matplotlib", "matplotlib.pyplot",
            "matplotlib.cm", "h5py", "configargparse", "trimesh"):
    sys.modules.setdefault(mod, MagicMock())

import _occupancy_restate as RS  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

import networks.dm_nerf as R_model  # noqa: E402  (reference)
import tools.visualizer as R_vis  # noqa: E402  (reference)

torch.set_num_threads(1)
OUT = os.environ.get("DMNERF_GOLDEN_OUT", HERE)
OCC_RANGE = [-1.0, 1.0]
EXTENTS = np.array([1.9, 7.0, 7.0])
NEAR, FAR, N_IMPORTANCE = 4.0, 15.0, 128
WEIGHTS = {13: dict(seed=901, gain=1.7, sigma_bias=0.0), 93: dict(seed=902, gain=1.7, sigma_bias=0.0)}


def rigid(rng):
    """A random rotation (QR of a Gaussian matrix, determinant +1) and a translation, as a float64 4 x 4."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3] = q
    T[:3, 3] = rng.uniform(-1.5, 1.5, size=3)
    return T


def reference_points(transform, dim):
    """mesh_generator.py:27-31."""
    pts, _ = R_vis.grid_within_bound(OCC_RANGE, EXTENTS, transform, grid_dim=dim)
    pts = pts[:, :, [0, 2, 1]]
    pts[:, :, 1] = pts[:, :, 1] * -1
    return pts.reshape(-1, 3)


def reference_sigma(model, pe, ve, pts, n_test=100):
    """mesh_generator.py:33-51, chunks and ``torch.cat`` included."""
    raw = None
    N = pts.shape[0]
    with torch.no_grad():
        for step in range(0, N, n_test):
            in_pcd = pts[step:step + min(n_test, N - step)]
            embedded = torch.cat([pe.embed(in_pcd), ve.embed(torch.zeros_like(in_pcd))], -1)
            raw_fine = model(embedded)
            raw = raw_fine if raw is None else torch.cat((raw, raw_fine), dim=0)
    return raw[..., 3]


def main():
    rng = np.random.default_rng(20261017)
    transform = rigid(rng)
    for dim in (5, 8, 16, 33):                       # the restatement against the reference, other transforms too
        for T in (transform, rigid(rng)):
            want = reference_points(T, dim).numpy()
            got = RS.grid_points(OCC_RANGE, EXTENTS, T, dim)
            assert got.dtype == np.float32 and np.array_equal(got, want), dim
    pe, _ = R_model.get_embedder(10, 0)
    ve, _ = R_model.get_embedder(4, 0)
    voxel = (FAR - NEAR) / N_IMPORTANCE
    arrays = {"transform": transform, "extents": EXTENTS, "occ_range": np.asarray(OCC_RANGE), "near": np.float64(NEAR),
              "far": np.float64(FAR), "n_importance": np.int64(N_IMPORTANCE), "voxel": np.float64(voxel)}
    for ins_num, w in WEIGHTS.items():
        arrays[f"seed_{ins_num}"] = np.int64(w["seed"])
        arrays[f"gain_{ins_num}"] = np.float64(w["gain"])
        arrays[f"sigma_bias_{ins_num}"] = np.float64(w["sigma_bias"])
    for dim in (5, 8):
        pts = reference_points(transform, dim)
        arrays[f"points_{dim}"] = pts.numpy()
        for ins_num, w in WEIGHTS.items():
            if ins_num == 93 and dim != 5:
                continue
            model = R_model.DM_NeRF(8, 256, 63, 27, [4], ins_num)
            model.load_state_dict(O.make_weights(w["seed"], ins_num, gain=w["gain"], sigma_bias=w["sigma_bias"]))
            sigma = reference_sigma(model.eval(), pe, ve, pts)
            occ = 1.0 - torch.exp(-F.relu(sigma) * voxel)                 # occupancy_activation, mesh_generator.py:54-60
            C = ins_num + 1
            arrays[f"sigma_{C}_{dim}"] = sigma.numpy()
            arrays[f"occ_{C}_{dim}"] = occ.numpy()
            print(f"dim {dim}, C {C}: sigma in [{float(sigma.min()):.3f}, {float(sigma.max()):.3f}], {int((sigma < 0).sum())} of {sigma.numel()} "
                  f"negative; occ max {float(occ.max()):.4f}; |p| max {float(pts.abs().max()):.3f}")
    path = os.path.join(OUT, "occupancy.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
