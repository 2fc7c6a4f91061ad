"""The trained field off the camera rays: density at points, the occupancy grid, its iso-surface and the object label of surface
points.

This is the reference's ``mesh_main`` (tools/mesh_generator.py:12-143) without its file output (``mesh_scene`` chains the stages):

    mesh_generator.py:27-63    grid_within_bound + the fine network on 256^3 points + occupancy_activation  ->  ``occupancy_grid``
    :68-69                     skimage marching cubes at level 0.45 (classic table here)       ->  ``extract_surface``
    :71-86, :100               the canonical transform of trimesh                                            ->  ``scene_vertices``
    :93-94                     trimesh_to_open3d's compute_vertex_normals                                    ->  ``vertex_normals``
    :98-104                    open3d clean_mesh(min_num_cluster=400), remove_unreferenced_vertices          ->  ``clean_surface``
    :106-136                   one ray per vertex against its normal, dm_nerf, argmax                        ->  ``label_points``
    :137                       render_label2world (tools/visualizer.py:208-223)                              ->  ``label_colors``
    :89, :140                  the two .ply files                                                            ->  ``write_ply`` (host)

The surface stages are csrc/surface.hip; only the vertex and triangle totals that size the outputs reach the host.
``object_surfaces`` (csrc/object_surface.hip) is :68 per object of a label volume: one closed mesh each, all in one pass.

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
    _lib.launch("dmnerf_mlp_fwd_points_density", _blob(model, fuse_heads), model.ins_num, pts, M, out, voxel)
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
    for m0 in range(0, total, slab):
        n = min(slab, total - m0)
        _lib.launch("dmnerf_occupancy_slab", blob, model_fine.ins_num, t, dim, c_scale, c_T, m0, n, out[m0:m0 + n], voxel)
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
    z = None
    with torch.no_grad():
        render = R.fine_renderer(model_coarse, model_fine, args)
        for s in range(0, V, chunk):
            e = min(s + chunk, V)
            if z is None or z.shape[0] != e - s:
                z = helpers.z_val_sample(e - s, 0.01, 15, args.N_samples, device=v.device)
            ins = render(torch.stack([rays_o[s:e], rays_d[s:e]], dim=0), None, None, model_coarse, model_fine, z, args)['ins_fine']
            ins = ins.contiguous()
            _lib.launch("dmnerf_ins_label_conf", ins, e - s, ins.shape[-1], label[s:e], conf[s:e])
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


# ---- the iso-surface: mesh_generator.py:68-104 on the device (csrc/surface.hip; tests/_surface_restate.py states it in numpy)
def _empty_surface(device):
    return torch.zeros(0, 3, dtype=torch.float32, device=device), torch.zeros(0, 3, dtype=torch.int32, device=device)


def extract_surface(occ, level=0.45):
    """Marching cubes of ``occ [dx, dy, dz]`` at ``level`` (mesh_generator.py:68) -> ``(vertices [V, 3] f32 in index units, faces
    [F, 3] int32)``: the classic 256-case triangulation, a point inside iff ``v > level``, a vertex at ``i + (level - a) / (b - a)``
    in f32, winding of ``gradient_direction='ascent'``.  Vertices are ordered by (owning grid point, axis), triangles by (cell,
    table position).  Everything stays on the device; the two totals that size the outputs are the only values the host reads.  An
    empty surface gives ``[0, 3]`` tensors."""
    occ = _lib.f32(occ)
    _lib.require_gpu(occ)
    if occ.dim() != 3:
        raise ValueError(f"extract_surface expects occ [dx, dy, dz], got {tuple(occ.shape)}")
    dx, dy, dz = occ.shape
    n = occ.numel()
    counts = torch.empty(2, max(n, 1), dtype=torch.uint8, device=occ.device)
    _lib.launch("dmnerf_surface_count", occ, dx, dy, dz, float(level), counts[0], counts[1])
    scans = torch.cumsum(counts, dim=1, dtype=torch.int64)
    V, F = scans[:, -1].tolist()
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"extract_surface: {V} vertices / {F} triangles do not fit int32 ids")
    if V == 0:
        return _empty_surface(occ.device)
    vertices = torch.empty(V, 3, dtype=torch.float32, device=occ.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=occ.device)
    _lib.launch("dmnerf_surface_emit", occ, dx, dy, dz, float(level), counts[0], counts[1], scans[0], scans[1], V, F, vertices, faces)
    return vertices, faces


def scene_vertices(vertices, dim, transform, extents=(1.9, 7.0, 7.0)):
    """Index units -> scene coordinates, mesh_generator.py:72-86 and :100: ``/ (dim - 1)`` (``dim = occ.shape[0]``, as there),
    translate -0.5, scale 2, scale by ``extents / 2``, apply the 4 x 4 ``transform``; float64 torch ops on ``[V, 3]`` where the
    vertices live, rounded once to f32."""
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"scene_vertices expects vertices [V, 3], got {tuple(vertices.shape)}")
    if int(dim) < 2:
        raise ValueError("dim must be >= 2")
    T = torch.as_tensor(np.asarray(transform.detach().cpu() if torch.is_tensor(transform) else transform, dtype=np.float64))
    if T.shape != (4, 4):
        raise ValueError("transform must be 4 x 4")
    T = T.to(vertices.device)
    half = torch.as_tensor(np.asarray(extents, dtype=np.float64) / 2.0, device=vertices.device)
    if half.shape != (3,):
        raise ValueError("extents must have 3 entries")
    v = vertices.double() / (int(dim) - 1)
    v = ((v + (-0.5)) * 2.0) * half
    v = v @ T[:3, :3].T + T[:3, 3]
    return v.float()


def _mesh_args(vertices, faces, normals=None):
    v = _lib.f32(vertices)
    _lib.require_gpu(v, faces, normals)
    if v.dim() != 2 or v.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"expected vertices [V, 3] f32 and faces [F, 3] int32, got {tuple(v.shape)} and {tuple(faces.shape)} {faces.dtype}")
    if normals is not None and (normals.shape != v.shape or normals.dtype != torch.float32):
        raise ValueError("normals must be [V, 3] f32")
    return v


def vertex_normals(vertices, faces, occ_shape=None):
    """The vertex normals of ``trimesh_to_open3d`` -> ``compute_vertex_normals()`` -> ``[V, 3]`` f32: per vertex the f32 sum of the
    unnormalised ``(p1 - p0) x (p2 - p0)`` of its triangles (area weights), normalised; a zero sum stays 0.  The triangles at a vertex
    are those of the <= 4 cells round its grid edge; they are summed in ascending triangle index, which for ``extract_surface``'s
    order is ascending cell index and table order.  A gather over the stably sorted incidence list: no float atomics, the same bits
    every run.  ``occ_shape``, when given, only checks that the mesh can have come from such a grid."""
    v = _mesh_args(vertices, faces)
    V, F = v.shape[0], faces.shape[0]
    if occ_shape is not None and V > 3 * int(np.prod(occ_shape)):
        raise ValueError(f"{V} vertices cannot come from a grid of shape {tuple(occ_shape)}")
    normals = torch.zeros(V, 3, dtype=torch.float32, device=v.device)
    if V == 0 or F == 0:
        return normals
    inc_vertex, inc_slot = torch.sort(faces.reshape(-1), stable=True)
    _lib.launch("dmnerf_surface_normals", v, V, faces, F, inc_vertex, inc_slot, normals)
    return normals


def surface_clusters(faces):
    """``cluster_connected_triangles``: two triangles are connected iff they share a mesh edge (the same unordered vertex pair) ->
    ``(rep [F] int32, size [F] int32)``: the smallest triangle index of every triangle's cluster and that cluster's triangle count."""
    _lib.require_gpu(faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"surface_clusters expects faces [F, 3] int32, got {tuple(faces.shape)} {faces.dtype}")
    rep, count = _clusters(faces)
    return rep, count[rep.long()]


def _clusters(faces):
    F = faces.shape[0]
    rep = torch.empty(F, dtype=torch.int32, device=faces.device)
    count = torch.zeros(F, dtype=torch.int32, device=faces.device)
    if F == 0:
        return rep, count
    a, b = faces.long(), faces[:, [1, 2, 0]].long()
    key, slot = torch.sort(((torch.minimum(a, b) << 32) | torch.maximum(a, b)).reshape(-1))
    parent = torch.arange(F, dtype=torch.int32, device=faces.device)
    _lib.launch("dmnerf_surface_clusters", key, slot, F, parent, rep, count)
    return rep, count


def clean_surface(vertices, normals, faces, min_triangles=400, keep_single_cluster=False):
    """``clean_mesh`` (tools/visualizer.py) and ``remove_unreferenced_vertices`` -> ``(vertices, normals, faces, kept_vertex_index
    [V'] int64)``: triangles whose cluster has fewer than ``min_triangles`` triangles go (with ``keep_single_cluster`` all but the
    largest cluster, ties to the smallest representative), then the vertices nobody references; both compactions keep the order and
    re-index the faces; the normals travel with their vertices."""
    v = _mesh_args(vertices, faces, normals)
    V, F = v.shape[0], faces.shape[0]
    dev = v.device
    rep, count = _clusters(faces)
    single = torch.argmax(count).reshape(1) if keep_single_cluster and F else None        # first maximum: the smallest representative
    keep = torch.zeros(F, dtype=torch.uint8, device=dev)
    used = torch.zeros(V, dtype=torch.uint8, device=dev)
    _lib.launch("dmnerf_surface_clean_mark", faces, F, V, rep, count, int(min_triangles), single, keep, used)
    fscan = torch.cumsum(keep, dim=0, dtype=torch.int32)
    vscan = torch.cumsum(used, dim=0, dtype=torch.int32)
    Fk, Vk = torch.stack([fscan[-1] if F else fscan.sum(), vscan[-1] if V else vscan.sum()]).tolist()
    out_v = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    out_n = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
    kept = torch.empty(Vk, dtype=torch.int64, device=dev)
    _lib.launch("dmnerf_surface_clean_compact", v, normals, faces, V, F, keep, used, fscan, vscan, Vk, Fk, out_v, out_n, out_f, kept)
    return out_v, out_n, out_f, kept


def mesh_scene(models, transform, args, ins_rgbs=None, color_dict=None, ins_map=None, grid_dim=256, level=0.45, min_triangles=400,
               **grid_kw):
    """``mesh_main`` (mesh_generator.py:12-143) without its file output: ``occupancy_grid`` -> ``extract_surface`` ->
    ``scene_vertices`` -> ``vertex_normals`` -> ``clean_surface`` -> ``label_points`` (-> ``label_colors`` when ``ins_rgbs``,
    ``color_dict`` and ``ins_map`` are given).  Returns a namespace with ``vertices``, ``faces``, ``normals``, ``labels``, ``conf``,
    ``colors`` (or None) and the uncleaned ``vertices_raw`` / ``faces_raw`` (the first ``.ply`` of the reference).  No tensor goes
    to the host."""
    import types
    extents = grid_kw.get("extents", (1.9, 7.0, 7.0))
    occ = occupancy_grid(models[1], transform, args, grid_dim=grid_dim, **grid_kw)
    v_idx, faces_raw = extract_surface(occ, level)
    vertices_raw = scene_vertices(v_idx, occ.shape[0], transform, extents)
    normals_raw = vertex_normals(vertices_raw, faces_raw, occ.shape)
    vertices, normals, faces, _ = clean_surface(vertices_raw, normals_raw, faces_raw, min_triangles=min_triangles)
    labels, conf = label_points(vertices, normals, models, args)
    colors = None
    if ins_rgbs is not None and color_dict is not None and ins_map is not None:
        colors = label_colors(labels, ins_rgbs, color_dict, ins_map)
    return types.SimpleNamespace(vertices=vertices, faces=faces, normals=normals, labels=labels, conf=conf, colors=colors,
                                 vertices_raw=vertices_raw, faces_raw=faces_raw)


def write_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY of a mesh (the one host step): ``vertices [V, 3]`` f32, optional ``normals [V, 3]`` f32 and
    ``colors [V, 3]`` uint8 (written as given: red = column 0), ``faces [F, 3]`` as ``uchar 3, int, int, int``."""
    def host(t):
        return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    v = np.ascontiguousarray(host(vertices), dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(host(faces), dtype="<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    rows = np.zeros(v.shape[0], dtype=np.dtype(fields))
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = np.asarray(host(normals), dtype="<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("normals must be [V, 3]")
        rows["nx"], rows["ny"], rows["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        c = np.asarray(host(colors), dtype=np.uint8).reshape(-1, 3)
        if c.shape != v.shape:
            raise ValueError("colors must be [V, 3]")
        rows["red"], rows["green"], rows["blue"] = c[:, 0], c[:, 1], c[:, 2]
    tris = np.zeros(f.shape[0], dtype=np.dtype([("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")]))
    tris["n"], tris["a"], tris["b"], tris["c"] = 3, f[:, 0], f[:, 1], f[:, 2]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rows.tobytes())
        fh.write(tris.tobytes())


# ---- the occupancy bit grid of a render that skips empty space (csrc/skip.hip; tests/_skip_restate.py states it in numpy)
SKIP_OUTSIDE = {"evaluate": 0, "empty": 1}          # DMNERF_SKIP_OUTSIDE_* (include/dmnerf_hip.h)


def _dims3(dims):
    dims = (int(dims),) * 3 if np.ndim(dims) == 0 else tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"dims must be one or three positive integers, got {dims}")
    if dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{dims[0] * dims[1] * dims[2]} cells do not fit int32")
    return dims


def _box(who, lo, hi, dims):
    """The box of ``who`` (``SkipGrid`` / ``LabelGrid``) over ``dims`` (a ``_dims3``) -> float32 ``(lo, hi, cell, inv_cell)``."""
    lo, hi = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(hi, dtype=np.float32).reshape(3)
    if not np.all(hi > lo):
        raise ValueError(f"{who}: hi must be > lo on every axis")
    cell = (hi - lo) / np.asarray(dims, dtype=np.float32)
    return lo, hi, cell, np.float32(1.0) / cell


def _ray_pair(who, rays_o, rays_d):
    """``rays_o``, ``rays_d [N, 3]`` f32 on the device, checked in ``who``'s name -> one ray set ``[2, N, 3]``."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be a float32 tensor")
    _lib.require_gpu(rays_o, rays_d)
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_d.shape != rays_o.shape:
        raise ValueError(f"{who} expects rays_o, rays_d [N, 3], got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
    return torch.stack([rays_o, rays_d])


def _axis_centres(grid, a, n0, n1, dev):
    """The centres of cells ``n0 .. n1 - 1`` of ``grid`` along axis ``a`` on ``dev`` (f32 ops, one rounding each)."""
    return (torch.arange(n0, n1, dtype=torch.float32, device=dev) + 0.5) * float(grid.cell[a]) + float(grid.lo[a])


def or_gathered_words(gathered, world):
    """The bitwise OR over ranks of ``gathered [world * n_words]`` (the ranks' packed words, concatenated as
    ``distributed.all_gather_cat`` returns them) -> ``[n_words]``, same dtype and device.  Plain torch ops: the collective library
    offers no bitwise reduction, so the reduction is local; a 128^3 grid is 256 KB per rank."""
    world = int(world)
    if world < 1 or gathered.dim() != 1 or gathered.shape[0] % world:
        raise ValueError(f"or_gathered_words: {tuple(gathered.shape)} words do not split over {world} ranks")
    parts = gathered.reshape(world, -1)
    out = parts[0].clone()
    for r in range(1, world):
        out |= parts[r]
    return out


class SkipGrid:
    """An axis-aligned box ``[lo, hi)`` in world coordinates, ``dims = (dx, dy, dz)`` cells, one bit per cell: set = the cell may hold
    density, clear = a sample in it is not worth a network evaluation (``render.dm_nerf_fine_skip``).

    ``cell = float32(hi - lo) / float32(dims)`` and ``inv_cell = float32(1) / cell``, each rounded to f32 on its own; a point ``p`` is
    in cell ``c_a = floor((p_a - lo_a) * inv_cell_a)`` (f32 ops, one rounding each) and inside the box iff ``0 <= c_a < dims_a`` on all
    three axes.  ``bits``: uint32 words on the device, held as an int32 tensor ``[ceil(dx dy dz / 32)]`` (the same bits); cell
    ``g = (i * dy + j) * dz + k`` is bit ``g & 31`` of word ``g >> 5``; the unused bits of the last word are 0.  ``outside``: what a
    sample outside the box gets -- ``"evaluate"`` (default, conservative: the network runs there) or ``"empty"``.

    The bits may be overwritten in place (``grid.bits.copy_(other.bits)``): a captured render sees the new grid on its next replay."""

    def __init__(self, lo, hi, dims, bits, outside="evaluate"):
        self.dims = _dims3(dims)
        self.lo, self.hi, self.cell, self.inv_cell = _box("SkipGrid", lo, hi, self.dims)
        if outside not in SKIP_OUTSIDE:
            raise ValueError(f"SkipGrid: outside must be 'evaluate' or 'empty', got {outside!r}")
        self.outside = outside
        _lib.require_gpu(bits)
        if bits.dtype != torch.int32 or bits.dim() != 1 or bits.shape[0] != self.n_words:
            raise ValueError(f"SkipGrid: bits must be int32 [{self.n_words}], got {bits.dtype} {tuple(bits.shape)}")
        self.bits = bits

    @property
    def n_cells(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    @property
    def n_words(self):
        return (self.n_cells + 31) // 32

    def c_struct(self):
        """The ``dmnerf_skip_grid`` of this grid (points into ``bits``)."""
        g = _lib.SkipGridArgs()
        g.lo, _, g.inv_cell, g.dims = _lib.box_args(self)
        g.outside = SKIP_OUTSIDE[self.outside]
        g.d_bits = self.bits.data_ptr()
        return g

    @classmethod
    def from_bits(cls, bits, lo, hi, dims, outside="evaluate", device="cuda"):
        """From packed words: a numpy uint32 / int32 array or a tensor of ``ceil(cells / 32)`` words."""
        if not torch.is_tensor(bits):
            bits = torch.from_numpy(np.ascontiguousarray(np.asarray(bits)).astype(np.uint32).view(np.int32)).to(device)
        return cls(lo, hi, dims, bits.contiguous(), outside)

    @classmethod
    def empty(cls, lo, hi, dims, outside="evaluate", device="cuda"):
        """No cell set: the neutral element of ``|``; with ``outside="empty"`` nothing is evaluated at all."""
        dims = _dims3(dims)
        words = (dims[0] * dims[1] * dims[2] + 31) // 32
        return cls(lo, hi, dims, torch.zeros(words, dtype=torch.int32, device=device), outside)

    @classmethod
    def full(cls, lo, hi, dims, outside="evaluate", device="cuda"):
        """Every cell set: with ``outside="evaluate"`` the render equals the dense one."""
        g = cls.empty(lo, hi, dims, outside, device)
        g.bits.fill_(-1)
        tail = g.n_cells & 31
        if tail:
            g.bits[-1] = (1 << tail) - 1
        return g

    @classmethod
    def from_sigma(cls, sigma, lo, hi, threshold=0.0, dilate=1, outside="evaluate"):
        """From densities ``sigma [dx, dy, dz]`` at the cells: a cell's bit is set iff any sigma in its ``(2 dilate + 1)^3``
        neighbourhood, clipped at the faces, is ``> threshold``; NaN counts as occupied (``dmnerf_skip_grid_build``)."""
        sigma = _lib.f32(sigma)
        _lib.require_gpu(sigma)
        if sigma.dim() != 3:
            raise ValueError(f"SkipGrid.from_sigma expects sigma [dx, dy, dz], got {tuple(sigma.shape)}")
        g = cls.empty(lo, hi, tuple(sigma.shape), outside, sigma.device)
        dx, dy, dz = g.dims
        _lib.launch("dmnerf_skip_grid_build", sigma, dx, dy, dz, float(threshold), int(dilate), g.bits)
        return g

    def cell_centres(self, i0=0, i1=None, device=None):
        """The centres ``lo + (idx + 0.5) * cell`` of the cells of planes ``i0 .. i1 - 1`` -> ``[(i1 - i0) dy dz, 3]`` f32, in cell order
        (f32 ops, one rounding each)."""
        dx, dy, dz = self.dims
        i1 = dx if i1 is None else int(i1)
        dev = device or self.bits.device
        ax = [_axis_centres(self, a, n0, n1, dev) for a, (n0, n1) in enumerate(((int(i0), i1), (0, dy), (0, dz)))]
        ni = i1 - int(i0)
        return torch.stack([ax[0][:, None, None].expand(ni, dy, dz), ax[1][None, :, None].expand(ni, dy, dz),
                            ax[2][None, None, :].expand(ni, dy, dz)], dim=-1).reshape(-1, 3)

    @classmethod
    def from_model(cls, model_fine, lo, hi, dims=128, threshold=0.0, dilate=1, outside="evaluate", slab=1 << 20, fuse_heads=False,
                   device="cuda"):
        """From the network: sigma at the cell centres through ``query_density`` (the trunk-only kernel), in slabs of whole
        i-planes of about ``slab`` points, then ``from_sigma``.  Nothing touches the host."""
        g = cls.empty(lo, hi, dims, outside, device)
        dx, dy, dz = g.dims
        sigma = torch.empty(dx, dy, dz, dtype=torch.float32, device=g.bits.device)
        step = max(1, int(slab) // (dy * dz))
        for i0 in range(0, dx, step):
            i1 = min(i0 + step, dx)
            sigma[i0:i1] = query_density(model_fine, g.cell_centres(i0, i1), fuse_heads=fuse_heads).reshape(i1 - i0, dy, dz)
        return cls.from_sigma(sigma, lo, hi, threshold=threshold, dilate=dilate, outside=outside)

    # ---- the grid from rendered views (dmnerf_skip_grid_mark / dmnerf_skip_grid_dilate; tests/_mark_restate.py states them in numpy)
    def _check_same(self, other, who):
        if not isinstance(other, SkipGrid):
            raise TypeError(f"SkipGrid.{who}: the other operand must be a SkipGrid")
        if (self.dims != other.dims or not np.array_equal(self.lo, other.lo) or not np.array_equal(self.hi, other.hi)
                or self.outside != other.outside):
            raise ValueError(f"SkipGrid.{who}: the two grids must have the same box, dims and outside policy")
        if self.bits.device != other.bits.device:
            raise RuntimeError(f"SkipGrid.{who}: the two grids live on different devices")

    def copy(self):
        """A grid with the same box, dims and policy and its own copy of the bits."""
        return SkipGrid(self.lo, self.hi, self.dims, self.bits.clone(), self.outside)

    def __or__(self, other):
        """Cells set in either grid (same box, dims and ``outside`` required, else ``ValueError``); ``empty`` is neutral."""
        self._check_same(other, "__or__")
        return SkipGrid(self.lo, self.hi, self.dims, self.bits | other.bits, self.outside)

    def __ior__(self, other):
        self._check_same(other, "__ior__")
        self.bits |= other.bits                      # in place: a captured render sees the new bits on its next replay
        return self

    def mark(self, rays_o, rays_d, z, weights, threshold=0.0):
        """Sets, in place, the cell of every sample ``p = o + d z`` that lies inside the box and whose compositing weight is
        ``> threshold`` (NaN counts); returns ``self``.  ``rays_o``, ``rays_d`` ``[N, 3]``, ``z`` and ``weights`` ``[N, S]``, f32 on
        the grid's device.  Bits are only ever set, samples outside the box mark nothing, and ``outside`` plays no part.  The cell
        arithmetic is the select's, so a sample this call marks is a sample ``dm_nerf_fine_skip`` evaluates.  One launch
        (``dmnerf_skip_grid_mark``), no allocation, no synchronisation: it can be captured in a graph."""
        threshold = float(threshold)
        if not threshold >= 0.0:
            raise ValueError(f"SkipGrid.mark: threshold must be >= 0, got {threshold}")
        for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("z", z), ("weights", weights)):
            if not torch.is_tensor(t) or t.dtype != torch.float32:
                raise ValueError(f"SkipGrid.mark: {name} must be a float32 tensor")
        _lib.require_gpu(rays_o, rays_d, z, weights)
        if z.dim() != 2 or weights.shape != z.shape or tuple(rays_o.shape) != (z.shape[0], 3) or rays_d.shape != rays_o.shape:
            raise ValueError(f"SkipGrid.mark expects rays_o, rays_d [N, 3] and z, weights [N, S], got {tuple(rays_o.shape)}, "
                             f"{tuple(rays_d.shape)}, {tuple(z.shape)}, {tuple(weights.shape)}")
        if any(t.device != self.bits.device for t in (rays_o, rays_d, z, weights)):
            raise RuntimeError("SkipGrid.mark: the grid lives on another device than the samples")
        N, S = z.shape
        if N * S >= 2 ** 31:
            raise ValueError(f"SkipGrid.mark: {N * S} samples do not fit int32; mark in smaller chunks")
        if N * S == 0:
            return self
        g = self.c_struct()
        _lib.launch("dmnerf_skip_grid_mark", g, self.bits, rays_o, rays_d, z, weights, N, S, threshold)
        return self

    def dilated(self, r):
        """A new grid, same box and ``outside``: a cell is set iff any cell of its ``(2 r + 1)^3`` neighbourhood, clipped at the faces,
        is set here (``0 <= r <= 4``; ``dmnerf_skip_grid_dilate``).  ``from_sigma(s, dilate=0).dilated(r)`` is ``from_sigma(s, dilate=r)``."""
        out = SkipGrid.empty(self.lo, self.hi, self.dims, self.outside, self.bits.device)
        dx, dy, dz = self.dims
        _lib.launch("dmnerf_skip_grid_dilate", self.bits, dx, dy, dz, int(r), out.bits)
        return out

    @classmethod
    def from_views(cls, poses, hwk, models, args, lo, hi, dims=128, threshold=0.0, dilate=0, levels=("coarse", "fine"), chunk=4096,
                   outside="evaluate"):
        """From renders: every pose of ``poses`` is rendered dense through ``distributed.render_frame(..., mark=grid)`` (near, far and
        ``N_samples`` from ``args``, chunks of ``chunk`` rays) and the cell of every sample whose weight is ``> threshold`` is set, at
        the levels named in ``levels``; then ``dilated(dilate)``.  With ``threshold = 0`` and ``outside="evaluate"``, re-rendering the
        same views through the grid gives the dense frames bit for bit ("The grid from rendered views").  Nothing
        touches the host.  With more than one rank every rank marks its own band of rows; the words are then all-gathered and OR-ed
        locally (``or_gathered_words``: the collective library has no bitwise reduction), so every rank returns the same grid."""
        from . import distributed as D
        H, W, K = hwk
        g = cls.empty(lo, hi, dims, outside, next(models[1].parameters()).device)
        for c2w in poses:
            D.render_frame(H, W, K, c2w, models, args.near, args.far, args, chunk=chunk, n_samples=int(getattr(args, "N_samples", 64)),
                           mark=g, mark_threshold=threshold, mark_levels=levels)
        _, world = D.world_info()
        if D._active(world):
            g.bits.copy_(or_gathered_words(D.all_gather_cat(g.bits), world))
        return g.dilated(dilate)

    def unpack(self):
        """The bits as a bool tensor ``[dx, dy, dz]`` on the device."""
        g = torch.arange(self.n_cells, device=self.bits.device)
        return (((self.bits[g >> 5] >> (g & 31)) & 1) != 0).reshape(self.dims)

    def occupancy(self):
        """Fraction of set cells (a device scalar)."""
        return self.unpack().float().mean()

    def cleaned(self, min_cells, connectivity=26):
        """A new grid, same box and ``outside``, without the isolated cells the render would march into: a set cell stays set iff
        its connected component of set cells has at least ``min_cells`` cells (``LabelGrid.cleaned`` of the bits as a one-label
        volume, then ``skip_grid(0)``).  ``connectivity`` 26 (default) or 6; bad arguments raise ``ValueError``."""
        labels = torch.where(self.unpack(), 0, UNLABELLED).to(torch.uint8)
        grid, _ = LabelGrid.from_labels(labels, self.lo, self.hi, C=1).cleaned(min_cells, connectivity=connectivity)
        return grid.skip_grid(0, outside=self.outside)


class TrainSkip:
    """When the grid of a training run that skips empty space (``autograd.dm_nerf_train(..., skip=)``, ``args.train_skip``) is
    refreshed from the network it trains.  There is no grid kernel of its own here: the object only decides when.

    ``.grid`` is ``SkipGrid.full`` for the first ``warmup`` steps (the step equals the dense one).  ``.step(model_fine)`` is called
    once per optimisation step, after the optimizer; on the call that completes the warm-up and on every ``every``-th call after it
    the bits are overwritten IN PLACE (same tensor, same ``data_ptr``) with
    ``SkipGrid.from_model(model_fine, ..., threshold=threshold, dilate=0).dilated(dilate)``.  Returns True when it refreshed.

    Defaults ("Training through the grid"): ``warmup=500`` -- an untrained network's density has a random sign, and a
    sample that is skipped can never receive the gradient that would raise its density, so the grid must not be read before the
    field has a shape; ``every=16`` -- a 128^3 refresh is one trunk-only pass over 2.1 M points, a fraction of a step when spread
    over 16; ``threshold=0.0`` on the raw density: ``relu(sigma) = 0`` is the only value that is exactly neutral; ``dilate=1`` --
    the centre sample says nothing about the rest of the cell, and a surface can grow by one cell per refresh;
    ``outside="evaluate"``: nothing outside the box is assumed empty."""

    def __init__(self, lo, hi, dims=128, every=16, warmup=500, threshold=0.0, dilate=1, outside="evaluate", device="cuda"):
        self.every, self.warmup = int(every), int(warmup)
        if self.every < 1 or self.warmup < 0:
            raise ValueError(f"TrainSkip: every must be >= 1 and warmup >= 0, got {every}, {warmup}")
        self.threshold, self.dilate = float(threshold), int(dilate)
        self.grid = SkipGrid.full(lo, hi, dims, outside, device)
        self.steps = 0                  # calls of step() so far
        self.refreshes = 0

    def step(self, model_fine):
        self.steps += 1
        if self.steps < self.warmup or (self.steps - self.warmup) % self.every:
            return False
        g = self.grid
        with torch.no_grad():
            new = SkipGrid.from_model(model_fine, g.lo, g.hi, g.dims, threshold=self.threshold, dilate=0, outside=g.outside,
                                      device=g.bits.device).dilated(self.dilate)
            g.bits.copy_(new.bits)
        self.refreshes += 1
        return True


# ---- the occupancy volume labelled by object (csrc/label_grid.hip; tests/_label_grid_restate.py states it in numpy)
UNLABELLED = 255
MAX_LABELS = 128                # DMNERF_MAX_LOGITS (include/dmnerf_hip.h)
MAX_TRACE_SETS = 16             # ray sets of one dmnerf_label_trace
MAX_RENDER_SETS = 4             # ray sets of one dmnerf_baked_render


def label_rays(occ, i0=0, i1=None):
    """The rays whose samples are the label points of planes ``i0 .. i1 - 1`` of ``occ`` -> ``(o [n, 3], d [n, 3], z [n, dz])`` f32 on the
    grid's device, ``n = (i1 - i0) dy``: one ray per ``(i, j)`` column, ``o`` = the ``cell_centres`` value of cell ``(i, j, 0)``,
    ``d = (0, 0, cell_z)``, ``z[n, k] = float(k)``.  The label point of cell ``(i, j, k)`` is DEFINED as the network kernels'
    ``o + d z`` in f32 (multiply, then add, each rounded): x and y are the centre's exactly, z is ``centre_z(0) + cell_z k``, which may
    differ from ``cell_centres``' ``(k + 0.5) cell_z + lo_z`` in the last bits.  Device ops only."""
    dx, dy, dz = occ.dims
    i1 = dx if i1 is None else int(i1)
    dev = occ.bits.device
    ax = [_axis_centres(occ, a, n0, n1, dev) for a, (n0, n1) in enumerate(((int(i0), i1), (0, dy), (0, 1)))]
    ni = i1 - int(i0)
    o = torch.stack([ax[0][:, None].expand(ni, dy), ax[1][None, :].expand(ni, dy), ax[2][None, :].expand(ni, dy)], dim=-1).reshape(-1, 3)
    d = torch.zeros(ni * dy, 3, dtype=torch.float32, device=dev)
    d[:, 2].fill_(float(occ.cell[2]))
    z = torch.arange(dz, dtype=torch.float32, device=dev)[None, :].expand(ni * dy, dz).contiguous()
    return o, d, z


def label_mask_words(labels, C):
    """``labels`` (an int or an iterable of ints in ``[0, C)``, else ``ValueError``) as the four 32-bit words
    ``dmnerf_skip_grid_from_labels`` takes: ``networks.manipulator.keep_words``' two 64-bit words, little end first."""
    from .networks.manipulator import keep_words
    if isinstance(labels, (int, np.integer)):
        labels = [labels]
    try:
        labels = list(labels)
    except TypeError:
        raise ValueError(f"labels must be an int or an iterable of ints, got {labels!r}") from None
    for l in labels:
        if not isinstance(l, (int, np.integer)):
            raise ValueError(f"label {l!r} is not an integer")
    w = keep_words(labels, C)
    return [w[0] & 0xffffffff, w[0] >> 32, w[1] & 0xffffffff, w[1] >> 32]


def _check_label_points(occ):
    """Host arithmetic on ``dx + dy + dz`` floats: every label point lies in its own cell under ``SkipGrid``'s cell arithmetic (it
    does unless the box sits so far from the origin that f32 cannot resolve half a cell)."""
    f = np.float32
    for a in range(3):
        idx = np.arange(occ.dims[a], dtype=f)
        if a < 2:
            p = ((idx + f(0.5)) * occ.cell[a] + occ.lo[a]).astype(f)
        else:
            p = ((f(0.5) * occ.cell[a] + occ.lo[a]).astype(f) + (occ.cell[a] * idx).astype(f)).astype(f)
        c = np.floor(((p - occ.lo[a]).astype(f) * occ.inv_cell[a]).astype(f))
        if not np.array_equal(c, idx):
            raise ValueError(f"label_grid: float32 cannot place the label points of axis {a} in their cells (box {occ.lo} .. {occ.hi}, "
                             f"dims {occ.dims})")


def _label_loop(who, model_fine, occ, sigma_threshold, slab, split, bake):
    """The loop of ``label_grid`` and ``bake_grid`` -> ``(labels, cells or None, C)``: the fine network at the label points of whole
    i-planes, then ``dmnerf_label_cells`` or, with ``bake``, ``dmnerf_bake_cells`` (the same labels, and ``cells [dx, dy, dz, 4]``)."""
    sigma_threshold = float(sigma_threshold)
    if not sigma_threshold >= 0.0:
        raise ValueError(f"{who}: sigma_threshold must be >= 0, got {sigma_threshold}")
    if not isinstance(occ, SkipGrid):
        raise TypeError(f"{who}: occ must be a SkipGrid")
    slab = int(slab)
    if slab < 1:
        raise ValueError("slab must be >= 1")
    _check_label_points(occ)
    dx, dy, dz = occ.dims
    C = model_fine.ins_num + 1
    labels = torch.empty(dx, dy, dz, dtype=torch.uint8, device=occ.bits.device)
    cells = torch.empty(dx, dy, dz, 4, dtype=torch.float32, device=occ.bits.device) if bake else None
    step = max(1, slab // (dy * dz))
    for i0 in range(0, dx, step):
        i1 = min(i0 + step, dx)
        o, d, z = label_rays(occ, i0, i1)
        raw = R.run_network_skip(model_fine, o, d, z, occ, split=split)
        m = (i1 - i0) * dy * dz
        if bake:
            _lib.launch("dmnerf_bake_cells", raw, m, C, sigma_threshold, labels[i0:i1], cells[i0:i1])
        else:
            _lib.launch("dmnerf_label_cells", raw, m, C, sigma_threshold, labels[i0:i1])
    return labels, cells, C


def label_grid(model_fine, occ, sigma_threshold=0.0, slab=1 << 20, split=None):
    """Which object owns each cell of ``occ`` (a ``SkipGrid``) -> ``LabelGrid`` with its box and dims: the fine network at the label
    point of every set cell (``label_rays``), through ``render.run_network_skip`` -- clear cells get the empty row and are not
    evaluated -- then ``dmnerf_label_cells``: the first index of the maximum of all ``C = ins_num + 1`` logits where
    ``sigma > sigma_threshold``, else 255.  Label ``C - 1`` is the field's own "empty" class.  The label points lie inside the box, so
    ``occ.outside`` plays no part.  In slabs of whole i-planes of about ``slab`` cells; nothing reaches the host, so after one warm-up
    call it can be captured in a graph and follows ``occ.bits`` on replay.  ``split``, the network shape and device errors are what
    ``run_network_skip`` raises; ``sigma_threshold < 0`` or NaN raises ``ValueError``."""
    labels, _, C = _label_loop("label_grid", model_fine, occ, sigma_threshold, slab, split, bake=False)
    return LabelGrid(labels, occ.lo, occ.hi, C)


def _stats_of_sums(grid, count, index_sum, lo_idx, hi_idx):
    """The dict of ``LabelGrid.stats()`` (per label) and ``Components.table()`` (per component) from the integer sums of its rows: the
    float64 quantities are derived on the device from python scalars of ``grid``'s box (no host-to-device copy: capturable)."""
    n = count.double()
    lo, cell = grid.lo.astype(np.float64), grid.cell.astype(np.float64)
    per_axis = lambda idx, plus: torch.stack([(idx[:, a] + plus) * float(cell[a]) + float(lo[a]) for a in range(3)], dim=-1)
    return {"count": count, "index_sum": index_sum, "lo_idx": lo_idx, "hi_idx": hi_idx,
            "centre": per_axis(index_sum.double() / n[:, None], 0.5),
            "box_lo": per_axis(lo_idx.double(), 0.0), "box_hi": per_axis(hi_idx.double(), 0.0),
            "volume": n * float(cell[0] * cell[1] * cell[2])}


COMPONENTS_KEEP = {"all": 0, "largest": 1}    # DMNERF_COMPONENTS_KEEP_* (include/dmnerf_hip.h)
COMPONENTS_TILE = (8, 8, 32)                  # CC_TI, CC_TJ, CC_TK (csrc/components.hip): the cells of one workgroup of the tile pass


def _connectivity(who, connectivity):
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (6, 26):
        raise ValueError(f"{who}: connectivity must be 6 or 26, got {connectivity!r}")
    return int(connectivity)


class Components:
    """The connected components of a ``LabelGrid`` (``LabelGrid.components``): ``root`` / ``size`` int32 ``[dx, dy, dz]`` on the device,
    ``connectivity``, and the grid's ``labels``, box (``lo``, ``hi``, ``cell``, ``inv_cell``), ``dims`` and ``C``."""

    def __init__(self, grid, root, size, connectivity):
        self.labels, self.root, self.size, self.connectivity = grid.labels, root, size, connectivity
        self.lo, self.hi, self.cell, self.inv_cell, self.dims, self.C = grid.lo, grid.hi, grid.cell, grid.inv_cell, grid.dims, grid.C

    def largest(self):
        """The largest component of every label -> ``{"root" [C] int32, "size" [C] int32}`` on the device; on equal sizes the one with
        the smallest root; ``-1`` and ``0`` for a label without a cell (``dmnerf_label_components_largest``: ``atomicMax`` of
        ``size << 32 | 0x7fffffff - root`` over the root cells).  Nothing reaches the host."""
        best = torch.empty(self.C, dtype=torch.int64, device=self.labels.device)
        dx, dy, dz = self.dims
        _lib.launch("dmnerf_label_components_largest", self.labels, dx, dy, dz, self.C, self.root, self.size, best)
        size = best >> 32
        return {"root": torch.where(size > 0, 0x7fffffff - (best & 0xffffffff), -1).int(), "size": size.int()}

    def table(self):
        """One row per component, in ascending order of the roots -> a dict of device tensors.  ``id [dx, dy, dz]`` int32: the row of
        the cell's component, ``-1`` for an unlabelled cell.  Per component ``label [K]`` uint8, ``root [K]`` int32 and, with exactly
        ``LabelGrid.stats()``'s definitions and dtypes, ``count [K]``, ``index_sum [K, 3]``, ``lo_idx`` / ``hi_idx [K, 3]``, ``centre``,
        ``box_lo``, ``box_hi [K, 3]`` and ``volume [K]``.  The number of components ``K`` is read on the host (the one host read: the
        call cannot be captured in a graph).  The sums are torch's integer scatter operations: the same every run."""
        dev, n = self.labels.device, self.dims[0] * self.dims[1] * self.dims[2]
        root = self.root.reshape(-1)
        is_root = root == torch.arange(n, dtype=torch.int32, device=dev)
        roots = torch.nonzero(is_root).reshape(-1)                   # ascending; its length is the host read
        K = roots.shape[0]
        rank = torch.cumsum(is_root, 0) - 1
        cell_id = torch.where(root >= 0, rank[root.clamp(min=0).long()], -1)
        member = torch.nonzero(root >= 0).reshape(-1)
        row = cell_id[member]
        dy, dz = self.dims[1], self.dims[2]
        ijk = torch.stack([member // (dy * dz), (member // dz) % dy, member % dz], dim=-1)
        index_sum = torch.zeros(K, 3, dtype=torch.int64, device=dev).index_add_(0, row, ijk)
        rows3 = row[:, None].expand(-1, 3)
        lo_idx = torch.full((K, 3), 2 ** 31 - 1, dtype=torch.int32, device=dev).scatter_reduce_(0, rows3, ijk.int(), "amin")
        hi_idx = torch.zeros(K, 3, dtype=torch.int32, device=dev).scatter_reduce_(0, rows3, ijk.int() + 1, "amax")
        out = {"id": cell_id.int().reshape(self.dims), "label": self.labels.reshape(-1)[roots], "root": roots.int()}
        out.update(_stats_of_sums(self, self.size.reshape(-1)[roots].long(), index_sum, lo_idx, hi_idx))
        return out


class LabelGrid:
    """``labels``: uint8 ``[dx, dy, dz]`` on the device over the box ``[lo, hi)`` of a ``SkipGrid`` (same ``cell`` arithmetic): the object
    that owns each cell, ``0 .. C - 1``, or 255 for none.  ``C`` is the number of labels the reductions cover."""

    def __init__(self, labels, lo, hi, C):
        _lib.require_gpu(labels)
        if labels.dtype != torch.uint8 or labels.dim() != 3:
            raise ValueError(f"LabelGrid: labels must be uint8 [dx, dy, dz], got {labels.dtype} {tuple(labels.shape)}")
        self.dims = _dims3(tuple(labels.shape))
        self.C = int(C)
        if not 1 <= self.C <= MAX_LABELS:
            raise ValueError(f"LabelGrid: C must be in [1, {MAX_LABELS}], got {self.C}")
        self.lo, self.hi, self.cell, self.inv_cell = _box("LabelGrid", lo, hi, self.dims)
        self.labels = labels

    @classmethod
    def from_labels(cls, labels, lo, hi, C=MAX_LABELS):
        """Wraps a given uint8 volume ``[dx, dy, dz]`` on the device.  ``C``: labels ``>= C`` count as unlabelled."""
        return cls(labels, lo, hi, C)

    def stats(self):
        """What every object covers -> a dict of device tensors, row ``l`` for label ``l < C``:

        ``count [C]`` int64 cells, ``index_sum [C, 3]`` int64 sums of their ``(i, j, k)``, ``lo_idx`` / ``hi_idx [C, 3]`` int32 smallest
        index and largest index + 1 per axis (``dims`` and 0 for a label without a cell) -- ``dmnerf_label_stats``, integer atomics
        only, the same every run -- and in float64 from them: ``centre [C, 3] = lo + (index_sum / count + 0.5) cell``, the mean of the
        cell centres (NaN where ``count == 0``), ``box_lo`` / ``box_hi [C, 3] = lo + idx cell``, and ``volume [C] = count cell_x cell_y
        cell_z``, the volume of the object's cells.  Nothing reaches the host."""
        dev, C = self.labels.device, self.C
        dx, dy, dz = self.dims
        count = torch.empty(C, dtype=torch.int64, device=dev)
        index_sum = torch.empty(C, 3, dtype=torch.int64, device=dev)
        lo_idx = torch.empty(C, 3, dtype=torch.int32, device=dev)
        hi_idx = torch.empty(C, 3, dtype=torch.int32, device=dev)
        _lib.launch("dmnerf_label_stats", self.labels, dx, dy, dz, C, count, index_sum, lo_idx, hi_idx)
        return _stats_of_sums(self, count, index_sum, lo_idx, hi_idx)

    def skip_grid(self, labels, dilate=0, outside="evaluate"):
        """The cells owned by ``labels`` (an int or an iterable of ints in ``[0, C)``, else ``ValueError``) as a ``SkipGrid`` over the
        same box: ``dmnerf_skip_grid_from_labels``, then ``dilated(dilate)``.  An unlabelled cell is never set."""
        mask = (ctypes.c_uint32 * 4)(*label_mask_words(labels, self.C))
        g = SkipGrid.empty(self.lo, self.hi, self.dims, outside, self.labels.device)
        _lib.launch("dmnerf_skip_grid_from_labels", self.labels, g.n_cells, mask, g.bits)
        return g.dilated(dilate) if int(dilate) else g

    # ---- what is connected in the volume (csrc/components.hip; tests/_components_restate.py states it in numpy)
    def components(self, connectivity=6):
        """The connected components of the volume -> ``Components``.  Two cells are adjacent iff they carry the same label ``< C`` and
        differ by exactly one in one axis (``connectivity=6``) or by at most one in every axis (``26``), without wrap-around; a
        component is a class of that adjacency.  ``.root [dx, dy, dz]`` int32: the smallest index ``g = (i dy + j) dz + k`` of the
        cell's component, ``-1`` for an unlabelled cell; ``.size``: the component's number of cells, ``0``.  Canonical, so the same
        arrays every run (``dmnerf_label_components``: union-find with integer atomics).  One launch, nothing reaches the host: after
        a warm-up call it can be captured in a graph and follows ``labels`` on replay.  Another connectivity raises ``ValueError``."""
        connectivity = _connectivity("LabelGrid.components", connectivity)
        _lib.require_gpu(self.labels)
        dx, dy, dz = self.dims
        root = torch.empty(self.dims, dtype=torch.int32, device=self.labels.device)
        size = torch.empty(self.dims, dtype=torch.int32, device=self.labels.device)
        _lib.launch("dmnerf_label_components", self.labels, dx, dy, dz, self.C, connectivity, root, size)
        return Components(self, root, size, connectivity)

    def cleaned(self, min_cells=1, keep="all", connectivity=6, labels=None, out=None):
        """The volume without its stray cells -> ``(grid, info)``.  ``grid`` is a volume of this one's class over the same box and ``C``
        (a ``BakedGrid`` stays a ``BakedGrid``): a cell whose label is in ``labels`` (an int or an iterable as in ``skip_grid``;
        default: every label ``< C``) keeps it iff its component (``components(connectivity)``) has at least ``min_cells`` cells and,
        with ``keep="largest"``, is the largest component of its label -- on equal sizes the one with the smallest root.  Otherwise
        the cell becomes 255 and, in a baked volume, its four floats zero (``BakedGrid``'s invariant for an unlabelled cell).  Every
        other cell, and every other cell's floats, pass through bit for bit; with the defaults the result equals the input.
        ``info = {"removed" [C], "kept" [C]}`` int64 on the device: the cells of each label that lost it and that still carry it
        (``removed + kept == stats()["count"]``).  Connectivity is per label: nothing is merged across labels, no hole is filled, and
        a thin bridge of cells joins two blobs into one component.

        ``out``: an earlier result's ``grid`` (same class, dims, ``C``, box and device, sharing no memory with this volume) to write
        into.  Nothing reaches the host: after a warm-up call, ``cleaned(..., out=grid)`` can be captured in a graph and follows
        ``labels`` / ``cells`` on replay.  ``ValueError``: ``min_cells`` not an integer in ``[1, 2^31)``, another ``keep`` or
        ``connectivity``, a label outside ``[0, C)``, an ``out`` that does not fit or aliases the volume."""
        from .editing import _overlaps
        who = "LabelGrid.cleaned"
        if isinstance(min_cells, bool) or not isinstance(min_cells, (int, np.integer)) or not 1 <= min_cells < 2 ** 31:
            raise ValueError(f"{who}: min_cells must be an integer in [1, 2^31), got {min_cells!r}")
        if keep not in COMPONENTS_KEEP:
            raise ValueError(f"{who}: keep must be 'all' or 'largest', got {keep!r}")
        connectivity = _connectivity(who, connectivity)
        mask = (ctypes.c_uint32 * 4)(*label_mask_words(range(self.C) if labels is None else labels, self.C))
        baked = isinstance(self, BakedGrid)
        src_cells = self.cells if baked else None
        if out is not None:
            if out is not self and (type(out) is not type(self) or out.dims != self.dims or out.C != self.C
                                    or not np.array_equal(out.lo, self.lo) or not np.array_equal(out.hi, self.hi)
                                    or out.labels.device != self.labels.device):
                raise ValueError(f"{who}: out must be a {type(self).__name__} of dims {self.dims}, C = {self.C} and the box {self.lo} .. "
                                 f"{self.hi} on {self.labels.device} (an earlier result's grid)")
            if out is self or _overlaps(out.labels, self.labels) or (baked and _overlaps(out.cells, self.cells)):
                raise ValueError(f"{who}: out shares memory with the source volume")
            _lib.require_gpu(out.labels, out.cells if baked else None)
        comp = self.components(connectivity)
        _lib.require_gpu(src_cells)
        dev = self.labels.device
        if out is None:
            new = torch.empty_like(self.labels)
            out = BakedGrid(new, torch.empty_like(self.cells), self.lo, self.hi, self.C) if baked else LabelGrid(new, self.lo, self.hi, self.C)
        info = {"removed": torch.empty(self.C, dtype=torch.int64, device=dev), "kept": torch.empty(self.C, dtype=torch.int64, device=dev)}
        best = torch.empty(self.C, dtype=torch.int64, device=dev)
        dx, dy, dz = self.dims
        _lib.launch("dmnerf_label_components_filter", self.labels, src_cells, dx, dy, dz, self.C, mask, comp.root, comp.size, int(min_cells),
                    COMPONENTS_KEEP[keep], best, out.labels, out.cells if baked else None, info["removed"], info["kept"])
        return out, info

    # ---- rays through the volume (csrc/label_trace.hip; tests/_label_trace_restate.py states it in numpy)
    def _ray_sets(self, who, rays, label_sets, max_sets):
        """What ``trace_sets`` and ``BakedGrid.render_sets`` check of ``rays [R <= max_sets, 2, N, 3]`` and ``label_sets`` -> ``(R, N,
        the 4 R mask words)``."""
        if not torch.is_tensor(rays) or rays.dtype != torch.float32:
            raise ValueError(f"{who}: rays must be a float32 tensor")
        _lib.require_gpu(rays)
        if rays.dim() != 4 or rays.shape[1] != 2 or rays.shape[3] != 3 or not 1 <= rays.shape[0] <= max_sets:
            raise ValueError(f"{who} expects rays [R <= {max_sets}, 2, N, 3], got {tuple(rays.shape)}")
        if rays.device != self.labels.device:
            raise RuntimeError(f"{who}: the volume lives on another device than the rays")
        R, _, N, _ = rays.shape
        label_sets = list(label_sets)
        if len(label_sets) != R:
            raise ValueError(f"{who}: {len(label_sets)} label sets for {R} ray sets")
        return R, N, [w for labels in label_sets for w in label_mask_words(labels, self.C)]

    def trace_sets(self, rays, label_sets, near, far):
        """The first cell along every ray whose label is in the ray set's own label set -> ``{"label" [N] uint8, "t" [N] f32, "cell" [N]
        int32, "source" [N] uint8}`` on the device.  ``rays [R, 2, N, 3]`` f32: ``R <= 16`` sets of N (origin, direction) pairs, the
        n-th rays of all sets belonging to one pixel; ``label_sets``: R entries, each an int or an iterable of ints in ``[0, C)`` (else
        ``ValueError``; an empty iterable accepts nothing).  Per pixel the hit with the smallest ``t`` over the sets wins, the lowest
        set on equal ``t``; ``cell = (i dy + j) dz + k``, ``source`` = the winning set; a pixel without a hit gets (255, +inf, -1, 255).
        The traversal is exact, cell by cell, between ``near`` and ``far`` (``dmnerf_label_trace``); label 255 and labels ``>= C`` are
        never hit.  One launch, nothing reaches the host: after a warm-up call it can be captured in a graph and follows ``labels`` on
        replay."""
        R, N, words = self._ray_sets("LabelGrid.trace_sets", rays, label_sets, MAX_TRACE_SETS)
        dev = rays.device
        out = {"label": torch.empty(N, dtype=torch.uint8, device=dev), "t": torch.empty(N, dtype=torch.float32, device=dev),
               "cell": torch.empty(N, dtype=torch.int32, device=dev), "source": torch.empty(N, dtype=torch.uint8, device=dev)}
        _lib.launch("dmnerf_label_trace", self.labels, *_lib.box_args(self), self.C, rays, R, N,
                    (ctypes.c_uint32 * (4 * R))(*words), float(near), float(far), out["label"], out["t"], out["cell"], out["source"])
        return out

    def trace(self, rays_o, rays_d, near, far, labels=None):
        """``trace_sets`` with one ray set: ``rays_o``, ``rays_d [N, 3]`` f32 -> ``{"label", "t", "cell"}``.  ``labels``: an int or an
        iterable as in ``skip_grid``; the default is every label ``0 .. C - 1``."""
        out = self.trace_sets(_ray_pair("LabelGrid.trace", rays_o, rays_d)[None], [range(self.C) if labels is None else labels], near, far)
        del out["source"]
        return out


# ---- the baked field volume (csrc/label_grid.hip dmnerf_bake_cells, csrc/baked.hip; tests/_baked_restate.py states the render in numpy)
def bake_grid(model_fine, occ, sigma_threshold=0.0, slab=1 << 20, split=None):
    """``label_grid`` that keeps what the network said about colour and density -> ``BakedGrid``: the same loop with
    ``dmnerf_bake_cells`` in place of ``dmnerf_label_cells``, so ``.labels`` equals ``label_grid(...)``'s and ``.cells[i, j, k]`` is
    the first four floats of the cell's network row (three colour logits, sigma) for a labelled cell, zeros for an unlabelled one.
    The baked colour is the field's colour for the label rays' view direction, +z of the box (``label_rays``: ``d = (0, 0, cell_z)``);
    baking for another direction is out of scope.  Same arguments, same errors and the same graph-capture property as ``label_grid``."""
    labels, cells, C = _label_loop("bake_grid", model_fine, occ, sigma_threshold, slab, split, bake=True)
    return BakedGrid(labels, cells, occ.lo, occ.hi, C)


class BakedGrid(LabelGrid):
    """A ``LabelGrid`` with ``cells``: f32 ``[dx, dy, dz, 4]`` on the labels' device, per cell three colour logits and the density.
    Everything ``LabelGrid`` does (``stats``, ``skip_grid``, ``trace``, ``editing.pick`` / ``preview_frame``) works on it unchanged;
    ``render_sets`` / ``render`` volume-render the cells along rays (``dmnerf_baked_render``)."""

    def __init__(self, labels, cells, lo, hi, C):
        super().__init__(labels, lo, hi, C)
        if not torch.is_tensor(cells) or cells.dtype != torch.float32 or tuple(cells.shape) != (*self.dims, 4):
            raise ValueError(f"BakedGrid: cells must be a float32 tensor {(*self.dims, 4)}, got {getattr(cells, 'dtype', type(cells))} "
                             f"{tuple(getattr(cells, 'shape', ()))}")
        _lib.require_gpu(cells)
        if cells.device != labels.device:
            raise RuntimeError("BakedGrid: cells and labels live on different devices")
        self.cells = cells

    @classmethod
    def from_arrays(cls, labels, cells, lo, hi, C=MAX_LABELS):
        """Wraps given volumes on the device: ``labels`` uint8 ``[dx, dy, dz]``, ``cells`` f32 ``[dx, dy, dz, 4]``."""
        return cls(labels, cells, lo, hi, C)

    def render_sets(self, rays, label_sets, near, far, stop=0.0):
        """The cells of every ray set's own label set, volume-rendered along the pixel -> ``{"rgb" [N, 3], "depth" [N], "acc" [N]`` f32,
        ``"label" [N], "source" [N]`` uint8, ``"nseg" [N]`` int32``}`` on the device.  ``rays [R, 2, N, 3]`` and ``label_sets`` as in
        ``trace_sets``, but ``R <= 4`` (``ValueError`` beyond: the kernel keeps every set's walk in registers).  Each set walks the
        volume cell by cell as the trace does; a cell whose label is in the set is a segment from the walk's ``t`` to the next plane
        (or the exit), of length ``(t_out - t_in) |d|``; the segments of all sets are composited in ascending ``t_in``, the lowest
        set first on ties: ``alpha = 1 - exp(-max(sigma, 0) len)``, ``w = T alpha``, ``rgb += w sigmoid(logits)``, ``depth += w
        t_in``, ``acc += w``.  ``label`` / ``source`` are those of the heaviest segment (255 / 255 without a positive weight),
        ``nseg`` counts the segments.  ``stop``: a pixel ends once its transmittance is below it (0: never; negative or NaN raises).
        One launch, nothing reaches the host: after a warm-up call it can be captured in a graph and follows ``labels`` and
        ``cells`` on replay."""
        who = "BakedGrid.render_sets"
        if torch.is_tensor(rays) and rays.dim() == 4 and rays.shape[0] > MAX_RENDER_SETS:
            raise ValueError(f"{who}: {rays.shape[0]} ray sets, at most {MAX_RENDER_SETS}")
        stop = float(stop)
        if not stop >= 0.0:
            raise ValueError(f"{who}: stop must be >= 0, got {stop}")
        R, N, words = self._ray_sets(who, rays, label_sets, MAX_RENDER_SETS)
        dev = rays.device
        out = {"rgb": torch.empty(N, 3, dtype=torch.float32, device=dev), "depth": torch.empty(N, dtype=torch.float32, device=dev),
               "acc": torch.empty(N, dtype=torch.float32, device=dev), "label": torch.empty(N, dtype=torch.uint8, device=dev),
               "source": torch.empty(N, dtype=torch.uint8, device=dev), "nseg": torch.empty(N, dtype=torch.int32, device=dev)}
        _lib.launch("dmnerf_baked_render", self.labels, self.cells, *_lib.box_args(self), self.C,
                    rays, R, N, (ctypes.c_uint32 * (4 * R))(*words), float(near), float(far), stop, out["rgb"], out["depth"], out["acc"],
                    out["label"], out["source"], out["nseg"])
        return out

    def render(self, rays_o, rays_d, near, far, labels=None, stop=0.0):
        """``render_sets`` with one ray set: ``rays_o``, ``rays_d [N, 3]`` f32; ``labels`` as in ``trace`` (default: every label)."""
        return self.render_sets(_ray_pair("BakedGrid.render", rays_o, rays_d)[None], [range(self.C) if labels is None else labels], near, far, stop)


# ---- one closed surface per object of a label volume (csrc/object_surface.hip; tests/_object_surface_restate.py states it in numpy)
def _empty_objects(C, device):
    v, f = _empty_surface(device)
    zeros = torch.zeros(C + 1, dtype=torch.int64, device=device)
    return v, f, zeros, zeros.clone(), torch.zeros(0, dtype=torch.int32, device=device)


def object_surfaces(grid, value=None, level=0.45, voxel=None, labels=None, closed=True):
    """The iso-surface of every object of ``grid`` (a ``LabelGrid`` or a ``BakedGrid``, an ``editing.edit_volume`` result included) in
    one pass over the volume -> ``ObjectSurfaces``: all objects' meshes concatenated in ascending label.  The surface of object ``k`` is
    DEFINED as ``extract_surface(torch.where(grid.labels == k, value, 0), level)``: the same inside rule (``v > level``, NaN outside),
    f32 vertex formula, table, winding and order, bit for bit -- so an edge between two inside points of different labels carries two
    vertices, one per object, and the far end of a crossing edge contributes its real value only if it carries the same label.
    Labels ``>= C``, 255 included, own nothing.  With ``closed`` (the default) every masked field is surrounded by one virtual layer of
    0 points -- ``extract_surface`` on the volume padded by one point on all six sides, 1 subtracted from the vertices, in the padded
    grid's order -- so a mesh is watertight even where its object touches the box, and coordinates in ``[-1, d]`` are legal.

    ``value``: f32 ``[dx, dy, dz]`` on the volume's device.  ``None``: for a ``BakedGrid`` the occupancy ``1 - exp(-relu(sigma) * voxel)``
    of ``cells[..., 3]`` (``query_density``'s formula; ``voxel`` is then required), for a plain ``LabelGrid`` 1.0 everywhere, which gives
    blocky surfaces half-way between cells.  ``level`` must be ``> 0`` and finite in f32 (``ValueError``).  ``labels``: an int or an
    iterable as in ``skip_grid``; only those objects are meshed, the others get empty ranges.

    What it is not: ownership is the nearest cell's, so the surfaces of neighbouring objects do not coincide (a gap of up to one cell
    lies between them), and the table is the classic one, without Lewiner's ambiguity resolution.

    ``dmnerf_object_surface_count``, two ``torch.cumsum``, ``dmnerf_object_surface_emit`` in grid order with a key ``(label << 40) |
    position`` per vertex and triangle, two ``torch.sort`` of the (unique) keys and one ``torch.searchsorted`` that turns a corner's key
    into its vertex id.  The host reads the two totals that size the outputs, once; for that reason the call cannot be captured in a
    graph.  Totals of ``2^31`` or more raise; an empty result gives ``[0, 3]`` tensors and all-zero offsets.  CPU tensors raise: there
    is no fallback."""
    who = "object_surfaces"
    if not isinstance(grid, LabelGrid):
        raise TypeError(f"{who}: grid must be a LabelGrid or a BakedGrid")
    level = float(np.float32(level))
    if not (level > 0.0 and np.isfinite(level)):
        raise ValueError(f"{who}: level must be > 0 and finite in float32, got {level}")
    _lib.require_gpu(grid.labels)
    dev, C = grid.labels.device, grid.C
    if value is None:
        if isinstance(grid, BakedGrid):
            if voxel is None:
                raise ValueError(f"{who}: a BakedGrid without value needs voxel (the occupancy is 1 - exp(-relu(sigma) * voxel))")
            voxel = float(voxel)
            if not voxel >= 0.0:
                raise ValueError(f"{who}: voxel must be >= 0, got {voxel}")
            _lib.require_gpu(grid.cells)
            value = 1.0 - torch.exp(-torch.relu(grid.cells[..., 3]) * voxel)
        else:
            value = torch.ones(grid.dims, dtype=torch.float32, device=dev)
    if not torch.is_tensor(value) or value.dtype != torch.float32 or tuple(value.shape) != tuple(grid.dims):
        raise ValueError(f"{who}: value must be a float32 tensor {tuple(grid.dims)}, got {getattr(value, 'dtype', type(value))} "
                         f"{tuple(getattr(value, 'shape', ()))}")
    value = value.contiguous() if value.is_cuda else value
    _lib.require_gpu(value)
    if value.device != dev:
        raise RuntimeError(f"{who}: value lives on another device than the volume")
    mask = (ctypes.c_uint32 * 4)(*label_mask_words(range(C) if labels is None else labels, C))
    closed = bool(closed)
    dx, dy, dz = grid.dims
    n = (dx + 2 * closed) * (dy + 2 * closed) * (dz + 2 * closed)
    if n >= 2 ** 31:
        raise ValueError(f"{who}: {n} points (with the border) do not fit int32")
    head = (value, grid.labels, dx, dy, dz, C, mask, level, int(closed))
    counts = torch.empty(2, n, dtype=torch.uint8, device=dev)
    _lib.launch("dmnerf_object_surface_count", *head, counts[0], counts[1])
    scans = torch.cumsum(counts, dim=1, dtype=torch.int64)
    V, F = scans[:, -1].tolist()
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"{who}: {V} vertices / {F} triangles do not fit int32 ids")
    if V == 0:
        return ObjectSurfaces(*_empty_objects(C, dev), grid.lo, grid.hi, grid.dims, C)
    vkey = torch.empty(V, dtype=torch.int64, device=dev)
    vpos = torch.empty(V, 3, dtype=torch.float32, device=dev)
    vcell = torch.empty(V, dtype=torch.int32, device=dev)
    tkey = torch.empty(F, dtype=torch.int64, device=dev)
    ckey = torch.empty(F, 3, dtype=torch.int64, device=dev)
    _lib.launch("dmnerf_object_surface_emit", *head, counts[0], counts[1], scans[0], scans[1], V, F, vkey, vpos, vcell, tkey, ckey)
    vkey, vorder = torch.sort(vkey)
    tkey, torder = torch.sort(tkey)
    faces = torch.searchsorted(vkey, ckey[torder]).to(torch.int32)
    first = torch.arange(C + 1, dtype=torch.int64, device=dev) << 40
    return ObjectSurfaces(vpos[vorder], faces, torch.searchsorted(vkey, first), torch.searchsorted(tkey, first), vcell[vorder],
                          grid.lo, grid.hi, grid.dims, C)


class ObjectSurfaces:
    """What ``object_surfaces`` returns, all on the device: ``vertices [V, 3]`` f32 in index units (grid point ``p`` is the centre of cell
    ``p``), ``faces [F, 3]`` int32 with GLOBAL vertex ids, ``vertex_offset`` / ``face_offset [C + 1]`` int64 (object ``k`` owns
    ``vertices[vo[k]:vo[k + 1]]`` and ``faces[fo[k]:fo[k + 1]]``), ``vertex_cell [V]`` int32: the linear index ``(i dy + j) dz + k`` of the
    end of the vertex's grid edge that is inside the object -- gather anything per vertex with it, the baked colour for example -- and
    the volume's ``lo``, ``hi``, ``dims``, ``cell``, ``C``."""

    def __init__(self, vertices, faces, vertex_offset, face_offset, vertex_cell, lo, hi, dims, C, normals=None, kept_vertex_index=None):
        self.vertices, self.faces, self.vertex_offset, self.face_offset, self.vertex_cell = vertices, faces, vertex_offset, face_offset, vertex_cell
        self.dims, self.C = _dims3(dims), int(C)
        self.lo, self.hi, self.cell, _ = _box("ObjectSurfaces", lo, hi, self.dims)
        self._normals = normals
        self.kept_vertex_index = kept_vertex_index          # of ``cleaned()``: the index of every vertex in the uncleaned object

    def _range(self, k):
        k = int(k)
        if not 0 <= k < self.C:
            raise ValueError(f"ObjectSurfaces: label {k} outside [0, {self.C})")
        return self.vertex_offset[k:k + 2].tolist(), self.face_offset[k:k + 2].tolist()

    def object(self, k):
        """``(vertices, faces)`` of object ``k``: a view of its vertices and its faces with local ids.  Reads the object's four
        offsets on the host."""
        (v0, v1), (f0, f1) = self._range(k)
        return self.vertices[v0:v1], self.faces[f0:f1] - v0

    def world_vertices(self):
        """``lo + (v + 0.5) * cell`` in float64, rounded once to f32 (as ``scene_vertices`` does) -> ``[V, 3]``."""
        cell = torch.as_tensor(self.cell.astype(np.float64), device=self.vertices.device)
        lo = torch.as_tensor(self.lo.astype(np.float64), device=self.vertices.device)
        return (lo + (self.vertices.double() + 0.5) * cell).float()

    def normals(self, world=False):
        """``vertex_normals`` of the concatenation (objects share no vertex, so it applies as it is) -> ``[V, 3]`` f32; of the
        index-unit vertices, or with ``world`` of ``world_vertices()``, which differ where the cells are not cubes."""
        if world:
            return vertex_normals(self.world_vertices(), self.faces)
        if self._normals is None:
            self._normals = vertex_normals(self.vertices, self.faces)
        return self._normals

    def measures(self):
        """``{"area" [C], "volume" [C]}`` float64 on the device, in world units: per object the area ``sum |(p1 - p0) x (p2 - p0)| / 2``
        and the signed volume ``sum p0 . (p1 x p2) / 6`` of its triangles over the vertices multiplied by ``cell`` in float64
        (``dmnerf_object_surface_measures``: one workgroup per object, a fixed summation order, the same bits every run).  The volume
        of a closed mesh does not depend on the origin, so ``lo`` plays no part; an open mesh's is only a partial sum."""
        dev = self.vertices.device
        out = torch.zeros(2, self.C, dtype=torch.float64, device=dev)
        _lib.require_gpu(self.vertices, self.faces, self.face_offset)
        _lib.launch("dmnerf_object_surface_measures", self.vertices, self.vertices.shape[0], self.faces, self.faces.shape[0], self.face_offset,
                    self.C, (ctypes.c_double * 3)(*[float(c) for c in self.cell]), out[0], out[1])
        return {"area": out[0], "volume": out[1]}

    def cleaned(self, min_triangles=400, keep_single_cluster=False):
        """``clean_surface`` on the concatenation with ``normals()`` -> a new ``ObjectSurfaces`` (its ``normals()`` are the ones that
        travelled, its ``kept_vertex_index [V']`` int64 the old global index of every vertex).  A cluster never spans two objects, so
        ``min_triangles`` acts per object; ``keep_single_cluster`` keeps the largest cluster of the whole scene.  The offsets and
        ``vertex_cell`` are recomputed from ``kept_vertex_index`` on the device."""
        v, n, f, kept = clean_surface(self.vertices, self.normals(), self.faces, min_triangles=min_triangles, keep_single_cluster=keep_single_cluster)
        vo = torch.searchsorted(kept, self.vertex_offset)                                  # kept is ascending: the vertices kept below each start
        owner = torch.searchsorted(vo, f[:, 0].long(), right=True) - 1                     # the object of every kept triangle: ascending
        fo = torch.searchsorted(owner, torch.arange(self.C + 1, dtype=torch.int64, device=v.device))
        return ObjectSurfaces(v, f, vo, fo, self.vertex_cell[kept], self.lo, self.hi, self.dims, self.C, normals=n, kept_vertex_index=kept)

    def write(self, pattern, colors=None):
        """One ``write_ply`` per non-empty object (the only host step) -> the list of ``(label, path)`` written: ``pattern.format(k)`` is
        object ``k``'s file, with ``world_vertices()``, ``normals(world=True)`` and, when given, its rows of ``colors [V, 3]`` uint8."""
        if colors is not None and tuple(colors.shape) != tuple(self.vertices.shape):
            raise ValueError("colors must be [V, 3]")
        v, n = self.world_vertices(), self.normals(world=True)
        vo, fo = self.vertex_offset.tolist(), self.face_offset.tolist()
        written = []
        for k in range(self.C):
            if fo[k + 1] == fo[k]:
                continue
            path = pattern.format(k)
            write_ply(path, v[vo[k]:vo[k + 1]], self.faces[fo[k]:fo[k + 1]] - vo[k], n[vo[k]:vo[k + 1]],
                      None if colors is None else colors[vo[k]:vo[k + 1]])
            written.append((k, path))
        return written
