"""The trained field off the camera rays: density at points, the occupancy grid and the object label of surface points.

This is what the reference's ``mesh_main`` (tools/mesh_generator.py:12-143) does around its two host libraries:

    mesh_generator.py:27-63    grid_within_bound + the fine network on 256^3 points + occupancy_activation  ->  ``occupancy_grid``
    :68-104                    skimage marching cubes, trimesh, open3d clean_mesh                             (stay on the host)
    :106-136                   one ray per vertex against its normal, dm_nerf, argmax                        ->  ``label_points``
    :137                       render_label2world (tools/visualizer.py:208-223)                              ->  ``label_colors``

The density depends on neither the view direction nor the heads, so the grid goes through the trunk-only kernel
(csrc/mlp_fwd_points.hip): no ``[n, 90]`` embedding, no heads, no point tensor, no ``torch.cat`` and no host copy.  Tensors
live on the device; a CPU tensor raises, as everywhere in the package.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .networks import helpers
from .networks import render as R
from .networks.dm_nerf import Embedder

GENERIC_SLAB = 1 << 16          # rows per call of the layer-by-layer path (its [n, 90] operand and activations are per call)


def _voxel(voxel):
    if voxel is None:
        return -1.0
    voxel = float(voxel)
    if not voxel >= 0.0:
        raise ValueError(f"voxel must be >= 0 (or None for sigma), got {voxel}")
    return voxel


def _blob(model, fuse_heads):
    return model.blob_fused() if fuse_heads else model.blob()


def _generic_density(model, points, voxel, out):
    """Any other network shape: ``model(cat[embed(p), embed(0)])[:, 3]`` (mesh_generator.py:40-51) through dm_nerf_amd.generic."""
    Lp, Lv = (model.input_ch_pts - 3) // 6, (model.input_ch_views - 3) // 6
    if 3 + 6 * Lp != model.input_ch_pts or 3 + 6 * Lv != model.input_ch_views:
        raise NotImplementedError("query_density: the encoders must be get_embedder(multires, 0) outputs (3 + 6 L channels)")
    pe = Embedder(include_input=True, input_dims=3, max_freq_log2=Lp - 1, num_freqs=Lp, log_sampling=True)
    ve = Embedder(include_input=True, input_dims=3, max_freq_log2=Lv - 1, num_freqs=Lv, log_sampling=True)
    with torch.no_grad():
        for s in range(0, points.shape[0], GENERIC_SLAB):
            p = points[s:s + GENERIC_SLAB]
            sigma = model(torch.cat([pe.embed(p), ve.embed(torch.zeros_like(p))], -1))[:, 3]
            if voxel < 0:
                out[s:s + GENERIC_SLAB] = sigma
            else:
                out[s:s + GENERIC_SLAB] = 1.0 - torch.exp(-torch.relu(sigma) * voxel)
    return out


def query_density(model, points, voxel=None, fuse_heads=False):
    """Density of ``model`` at ``points [M, 3]`` -> ``[M]`` f32: ``model(cat[embed(p), embed(0)])[:, 3]`` bit for bit
    (mesh_generator.py:40-51), or with ``voxel`` the occupancy ``1 - exp(-relu(sigma) * voxel)`` (:54-60).  One launch of the
    trunk-only kernel; ``fuse_heads`` reads the fused-heads blob instead (the trunk is the same in both)."""
    pts = _lib.f32(points)
    _lib.require_gpu(pts)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"query_density expects points [M, 3], got {tuple(pts.shape)}")
    voxel = _voxel(voxel)
    M = pts.shape[0]
    out = torch.empty(M, dtype=torch.float32, device=pts.device)
    if not model._fused_ok():
        return _generic_density(model, pts, voxel, out)
    _lib.check(_lib.load().dmnerf_mlp_fwd_points_density(_lib.ptr(_blob(model, fuse_heads)), model.ins_num, _lib.ptr(pts), M,
                                                         _lib.ptr(out), voxel, _lib.stream()), "dmnerf_mlp_fwd_points_density")
    return out


def _grid_setup(occ_range, extents, transform, dim):
    """The three host-side constants of ``grid_within_bound`` (tools/visualizer.py:138-155): ``t = linspace(lo, hi, dim)`` as the
    host CPU evaluates it, ``scale = float32(extents / (hi - lo))`` and rows 0..2 of ``float32(transform)``."""
    dim = int(dim)
    if dim < 1:
        raise ValueError("grid_dim must be >= 1")
    lo, hi = float(occ_range[0]), float(occ_range[1])
    t = torch.linspace(lo, hi, steps=dim)
    scale = (np.asarray(extents, dtype=np.float64) / ((hi - lo) * 1.0)).astype(np.float32)
    if torch.is_tensor(transform):
        transform = transform.detach().cpu().numpy()
    T = np.ascontiguousarray(np.asarray(transform).astype(np.float32)[:3, :4])
    if scale.shape != (3,) or T.shape != (3, 4):
        raise ValueError("extents must have 3 entries and transform must be 4 x 4 (or 3 x 4)")
    return dim, t, scale, T


def grid_points(occ_range, extents, transform, dim, device="cuda"):
    """The query points of ``mesh_main`` -> ``[dim^3, 3]`` f32 on the device: ``grid_within_bound(occ_range, extents, transform,
    dim)`` (tools/visualizer.py:111-155) followed by the axis swap of mesh_generator.py:28-29, bit for bit.  The grid kernel
    computes the same values per sample and never reads this tensor; it is here for tests and for callers who want the points.
    Unfused device ops, one rounding each, in the reference's order."""
    dim, t, scale, T = _grid_setup(occ_range, extents, transform, dim)
    t = t.to(device)
    x = (t * float(scale[0]))[:, None, None]
    y = (t * float(scale[1]))[None, :, None]
    z = (t * float(scale[2]))[None, None, :]
    q = [((x * float(T[r, 0]) + y * float(T[r, 1])) + z * float(T[r, 2])) + float(T[r, 3]) for r in range(3)]
    return torch.stack([q[0], -q[2], q[1]], dim=-1).reshape(-1, 3)


def occupancy_grid(model_fine, transform, args, extents=(1.9, 7.0, 7.0), occ_range=(-1.0, 1.0), grid_dim=256, voxel=None,
                   slab=1 << 20, device="cuda"):
    """``occ [dim, dim, dim]`` f32 on the device = mesh_generator.py:27-63: the fine network's density on the oriented grid,
    through ``occupancy_activation`` with ``voxel`` (default ``(args.far - args.near) / args.N_importance``, :59).  The output is
    allocated once and filled by one launch per ``slab`` grid points; nothing touches the host.  ``transform``: the 4 x 4
    ``T_extent_to_scene`` (numpy or tensor)."""
    dim, t, scale, T = _grid_setup(occ_range, extents, transform, grid_dim)
    if voxel is None:
        voxel = (args.far - args.near) / args.N_importance
    voxel = _voxel(voxel)
    slab = int(slab)
    if slab < 1:
        raise ValueError("slab must be >= 1")
    total = dim ** 3
    out = torch.empty(total, dtype=torch.float32, device=device)
    _lib.require_gpu(out)
    if not model_fine._fused_ok():
        pts = grid_points(occ_range, extents, transform, dim, device=device)
        return _generic_density(model_fine, pts, voxel, out).reshape(dim, dim, dim)
    t = t.to(out.device)
    blob = _blob(model_fine, bool(getattr(args, "fuse_heads", False)))
    c_scale = (ctypes.c_float * 3)(*scale.tolist())
    c_T = (ctypes.c_float * 12)(*T.reshape(-1).tolist())
    fn, stream = _lib.load().dmnerf_occupancy_slab, _lib.stream()
    for m0 in range(0, total, slab):
        n = min(slab, total - m0)
        _lib.check(fn(_lib.ptr(blob), model_fine.ins_num, _lib.ptr(t), dim, c_scale, c_T, m0, n, _lib.ptr(out[m0:m0 + n]), voxel, stream),
                   "dmnerf_occupancy_slab")
    return out.reshape(dim, dim, dim)


def label_points(vertices, normals, models, args, chunk=None):
    """The object label of every surface point -> ``(label [V] int64, conf [V] f32)`` = mesh_generator.py:106-136: one ray per
    vertex against its normal, started ``0.03 * args.near`` in front of the surface, rendered with the reference's literal bounds
    ``z_val_sample(n, 0.01, 15, args.N_samples)``; ``label = argmax(ins_fine)``, ``conf`` its maximum.  ``vertices`` / ``normals``
    ``[V, 3]`` in the mesh's axes (the swap of :108-112 happens here); ``models = (model_coarse, model_fine)``; ``chunk`` defaults
    to ``args.N_test``."""
    model_coarse, model_fine = models
    v, n = _lib.f32(vertices), _lib.f32(normals)
    _lib.require_gpu(v, n)
    if v.dim() != 2 or v.shape[1] != 3 or n.shape != v.shape:
        raise ValueError(f"label_points expects vertices and normals [V, 3], got {tuple(v.shape)} and {tuple(n.shape)}")
    chunk = int(args.N_test if chunk is None else chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    rays_d = (-n)[:, [0, 2, 1]]
    rays_d[:, 1] = rays_d[:, 1] * -1
    v = v[:, [0, 2, 1]]
    v[:, 1] = v[:, 1] * -1
    rays_o = v - rays_d * 0.03 * args.near
    V = v.shape[0]
    label = torch.empty(V, dtype=torch.int64, device=v.device)
    conf = torch.empty(V, dtype=torch.float32, device=v.device)
    lib = _lib.load()
    z = None
    with torch.no_grad():
        render = R.dm_nerf_fine if R.fine_eligible(model_coarse, model_fine, args) else R.dm_nerf
        for s in range(0, V, chunk):
            e = min(s + chunk, V)
            if z is None or z.shape[0] != e - s:
                z = helpers.z_val_sample(e - s, 0.01, 15, args.N_samples, device=v.device)
            ins = render(torch.stack([rays_o[s:e], rays_d[s:e]], dim=0), None, None, model_coarse, model_fine, z, args)['ins_fine']
            ins = ins.contiguous()
            _lib.check(lib.dmnerf_ins_label_conf(_lib.ptr(ins), e - s, ins.shape[-1], _lib.ptr(label[s:e]), _lib.ptr(conf[s:e]),
                                                 _lib.stream()), "dmnerf_ins_label_conf")
    return label, conf


def color_table(n_rows, rgbs, color_dict, ins_map):
    """The host-built look-up table behind ``render_label2world`` / ``render_label2img`` (tools/visualizer.py:208-223, :73-86):
    numpy uint8 ``[n_rows, 3]`` whose row ``l`` is ``rgbs[color_dict[str(ins_map[str(l)])]]``, or 0 where ``ins_map`` has no ``l``
    (the reference leaves those pixels of its zero image untouched; ``astype(np.uint8)`` of the float64 image as there)."""
    rgbs = np.asarray(rgbs)
    lut = np.zeros((int(n_rows), 3))
    for k in (int(k) for k in ins_map.keys()):
        if 0 <= k < n_rows:
            lut[k] = rgbs[color_dict[str(ins_map[str(k)])]]
    return lut.astype(np.uint8)


def label_colors(labels, rgbs, color_dict, ins_map):
    """``render_label2world`` (tools/visualizer.py:208-223) -> ``[V, 3]`` uint8 on the device: the colour
    ``rgbs[color_dict[str(ins_map[str(label)])]]`` of every label, 0 for a label that ``ins_map`` does not hold.  The two dicts
    become one look-up table on the host (``color_table``); the device does one gather."""
    _lib.require_gpu(labels)
    if labels.dtype != torch.int64:
        raise ValueError("label_colors expects int64 labels")
    n = max([int(k) for k in ins_map.keys() if int(k) >= 0], default=-1) + 1
    lut = torch.from_numpy(color_table(n + 1, rgbs, color_dict, ins_map)).to(labels.device)   # row n: every label without an entry
    flat = labels.reshape(-1)
    idx = torch.where((flat >= 0) & (flat < n), flat, torch.full_like(flat, n))
    return lut[idx]
