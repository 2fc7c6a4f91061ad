"""Time the iso-surface stages of ``dm_nerf_amd.field`` (csrc/surface.hip), the middle of ``mesh_main``
(tools/mesh_generator.py:68-104), on the device.

    python scripts/time_surface.py                            # 256^3: HIP-event ms, median of --iters after --warmup
    python scripts/time_surface.py --dim 128 --iters 20

Two fields, one JSON line per stage and field:
  model      ``occupancy_grid`` of a fixed-seed network (oracle.ref_cpu.make_weights, sigma spread round the level): a noisy,
             large surface, the worst case for the emit, sort and cluster stages;
  sphere     a synthetic field with a known surface: a ball of radius 0.4 dim (area about 4 pi (0.4 dim)^2 index units^2).
Stages: ``count`` (the LDS-tiled classify pass alone; its achieved bytes/s = 4 B read + 2 B written per grid point, against the
6.3 TB/s that a float4 copy reaches on this part), ``extract`` (count + the two scans + emit, including the one 16-byte read of
the totals), ``scene``, ``normals``, ``clusters``, ``clean``, and ``d2h_grid``: the bare device -> host copy of the same grid into
pinned memory, the one step of the replaced path (copy, skimage, open3d, copy back) that can run here at all.
"""
import argparse
import ctypes
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

EXTENTS, OCC_RANGE, NEAR, FAR, N_IMP = (1.9, 7.0, 7.0), (-1.0, 1.0), 4.0, 15.0, 128
HBM_COPY_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--ins-num", type=int, default=13)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=float, default=0.45)
    ap.add_argument("--min-triangles", type=int, default=400)
    a = ap.parse_args()
    T.require_gpu(__file__)
    if a.iters < 10:
        print("note: fewer than 10 timed runs", file=sys.stderr)

    import torch
    from dm_nerf_amd import _lib, field as F
    from dm_nerf_amd.networks import dm_nerf as M
    from oracle import ref_cpu as O

    dim = a.dim
    trans = np.eye(4)
    trans[:3, :3] = np.linalg.qr(np.random.default_rng(0).standard_normal((3, 3)))[0]
    trans[:3, 3] = (0.3, -0.2, 0.5)
    model = M.DM_NeRF(8, 256, 63, 27, [4], a.ins_num)
    model.load_state_dict(O.make_weights(2, a.ins_num, gain=1.7, sigma_bias=7.5, sigma_gain=10.0))
    model = model.cuda().eval()
    args = types.SimpleNamespace(near=NEAR, far=FAR, N_importance=N_IMP)
    fields = {}
    with torch.no_grad():
        fields["model"] = F.occupancy_grid(model, trans, args, EXTENTS, OCC_RANGE, dim)
    g = torch.arange(dim, dtype=torch.float32, device="cuda") - (dim - 1) / 2.0
    r = torch.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    fields["sphere"] = torch.clamp(1.0 - 0.55 * r / (0.4 * dim), 0.0, 1.0).contiguous()     # 0.45 at r = 0.4 dim
    host = torch.empty(dim, dim, dim, dtype=torch.float32).pin_memory()
    lib = _lib.load()

    for name, occ in fields.items():
        n = occ.numel()
        base = {"field": name, "dim": dim, "points": n, "iters": a.iters, "device": torch.cuda.get_device_name(0)}

        def report(stage, fn, **kw):
            med, mn = T.time_events(fn, a.iters, a.warmup)[:2]
            print(json.dumps({"stage": stage, **base, **kw, "ms_median": med, "ms_min": mn}), flush=True)
            return med

        counts = torch.empty(2, n, dtype=torch.uint8, device="cuda")

        def count():
            _lib.check(lib.dmnerf_surface_count(_lib.ptr(occ), dim, dim, dim, ctypes.c_float(a.level), _lib.ptr(counts[0]), _lib.ptr(counts[1]),
                                                _lib.stream()), "dmnerf_surface_count")
        med, mn = T.time_events(count, a.iters, a.warmup)[:2]
        tbs = 6.0 * n / (med * 1e-3) / 1e12
        print(json.dumps({"stage": "count", **base, "ms_median": med, "ms_min": mn, "bytes_per_point": 6, "achieved_TB_per_s": tbs,
                          "fraction_of_hbm_copy_rate": tbs / HBM_COPY_TBS}), flush=True)
        v_idx, faces = F.extract_surface(occ, a.level)
        V, Fn = v_idx.shape[0], faces.shape[0]
        report("extract", lambda: F.extract_surface(occ, a.level), vertices=V, triangles=Fn)
        report("scene", lambda: F.scene_vertices(v_idx, dim, trans, EXTENTS))
        v = F.scene_vertices(v_idx, dim, trans, EXTENTS)
        report("normals", lambda: F.vertex_normals(v, faces, occ.shape))
        nrm = F.vertex_normals(v, faces, occ.shape)
        report("clusters", lambda: F.surface_clusters(faces))
        rep, _ = F.surface_clusters(faces)
        cv, _, cf, _ = F.clean_surface(v, nrm, faces, min_triangles=a.min_triangles)
        report("clean", lambda: F.clean_surface(v, nrm, faces, min_triangles=a.min_triangles), clusters=int(torch.unique(rep).numel()),
               kept_vertices=cv.shape[0], kept_triangles=cf.shape[0])
        report("d2h_grid", lambda: host.copy_(occ, non_blocking=True), megabytes=4 * n / 1e6)


if __name__ == "__main__":
    main()
