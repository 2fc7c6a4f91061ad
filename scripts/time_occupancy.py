"""Time the occupancy grid of ``mesh_main`` (tools/mesh_generator.py:27-63) on the device: ``field.occupancy_grid``
(csrc/mlp_fwd_points.hip) against the same query through the package's public drop-in path.

    python scripts/time_occupancy.py                          # 256^3 at ins_num 13: HIP-event ms, median of --iters
    python scripts/time_occupancy.py --legs grid              # the new path alone
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/time_occupancy.py --legs grid --iters 3      # kernel breakdown

Legs, one JSON line each:
  grid       ``occupancy_grid``: one ``dmnerf_occupancy_slab`` launch per slab, no point tensor, no embedding, no heads.
  points     ``query_density`` on the ``[dim^3, 3]`` point tensor made beforehand (the points prologue).
  baseline   what a caller of the drop-in can do today with every fairness: the points made beforehand, chunks of ``--n-test``,
             ``position_embedder.embed`` + ``view_embedder.embed(zeros)`` + ``cat`` + ``model_fine(embedded)``, column 3 written
             into a preallocated buffer (no growing ``cat``), the activation as one device op.
  reference_loop   the reference-shaped loop (``raw = torch.cat((raw, raw_fine))`` per chunk, all channels kept) at ``--loop-dim``,
             small enough to finish; its cost grows with the square of the chunk count.
The weights are synthetic (oracle.ref_cpu.make_weights); the time does not depend on them.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

EXTENTS, OCC_RANGE, NEAR, FAR, N_IMP = (1.9, 7.0, 7.0), (-1.0, 1.0), 4.0, 15.0, 128
MFMA_DENSITY, MFMA_FULL_C14 = 7680, 10880          # per 32 samples (csrc/mlp_fwd_points.hip, mlp_fwd_impl.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--loop-dim", type=int, default=64)
    ap.add_argument("--ins-num", type=int, default=13)
    ap.add_argument("--n-test", type=int, default=4096)
    ap.add_argument("--slab", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", nargs="*", default=["grid", "points", "baseline", "reference_loop"])
    a = ap.parse_args()
    T.require_gpu(__file__)

    import torch
    from dm_nerf_amd import field as F
    from dm_nerf_amd.networks import dm_nerf as M
    from oracle import ref_cpu as O

    model = M.DM_NeRF(8, 256, 63, 27, [4], a.ins_num)
    model.load_state_dict(O.make_weights(2, a.ins_num, gain=1.7, sigma_bias=0.3))
    model = model.cuda().eval()
    pe, ve = M.get_embedder(10, 0)[0], M.get_embedder(4, 0)[0]
    args = types.SimpleNamespace(near=NEAR, far=FAR, N_importance=N_IMP)
    voxel = (FAR - NEAR) / N_IMP
    trans = np.eye(4)
    trans[:3, :3] = np.linalg.qr(np.random.default_rng(0).standard_normal((3, 3)))[0]
    trans[:3, 3] = (0.3, -0.2, 0.5)
    n = a.dim ** 3
    base = {"dim": a.dim, "points": n, "ins_num": a.ins_num, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    results = {}

    def report(leg, med, mn, **kw):
        results[leg] = med
        print(json.dumps({"leg": leg, **base, **kw, "ms_median": med, "ms_min": mn}), flush=True)

    with torch.no_grad():
        if "grid" in a.legs:
            med, mn = T.time_events(lambda: F.occupancy_grid(model, trans, args, EXTENTS, OCC_RANGE, a.dim, slab=a.slab), a.iters, a.warmup)[:2]
            report("grid", med, mn, slab=a.slab, gsamples_per_s=n / med / 1e6)
        pts = F.grid_points(OCC_RANGE, EXTENTS, trans, a.dim) if {"points", "baseline"} & set(a.legs) else None
        if "points" in a.legs:
            med, mn = T.time_events(lambda: F.query_density(model, pts, voxel), a.iters, a.warmup)[:2]
            report("points", med, mn)
        if "baseline" in a.legs:
            out = torch.empty(n, dtype=torch.float32, device="cuda")

            def baseline():
                for s in range(0, n, a.n_test):
                    p = pts[s:s + a.n_test]
                    emb = torch.cat([pe.embed(p), ve.embed(torch.zeros_like(p))], -1)
                    out[s:s + a.n_test] = model(emb)[..., 3]
                return 1.0 - torch.exp(-torch.relu(out) * voxel)
            med, mn = T.time_events(baseline, a.iters, a.warmup)[:2]
            report("baseline", med, mn, n_test=a.n_test)
            if "grid" in results:
                got = F.occupancy_grid(model, trans, args, EXTENTS, OCC_RANGE, a.dim, slab=a.slab).reshape(-1)
                print(json.dumps({"leg": "compare", "max_abs_diff_grid_vs_baseline": float((got - baseline()).abs().max()),
                                  "time_ratio_grid_over_baseline": results["grid"] / med,
                                  "mfma_count_ratio": MFMA_DENSITY / MFMA_FULL_C14}), flush=True)
        if "reference_loop" in a.legs:
            lp = F.grid_points(OCC_RANGE, EXTENTS, trans, a.loop_dim)
            nl = lp.shape[0]

            def loop():
                raw = None
                for s in range(0, nl, a.n_test):
                    p = lp[s:s + a.n_test]
                    raw_fine = model(torch.cat([pe.embed(p), ve.embed(torch.zeros_like(p))], -1))
                    raw = raw_fine if raw is None else torch.cat((raw, raw_fine), dim=0)
                return (1.0 - torch.exp(-torch.relu(raw[..., 3]) * voxel)).cpu()
            med, mn = T.time_events(loop, a.iters, a.warmup)[:2]
            g_med, g_mn = T.time_events(lambda: F.occupancy_grid(model, trans, args, EXTENTS, OCC_RANGE, a.loop_dim, slab=a.slab), a.iters, a.warmup)[:2]
            print(json.dumps({"leg": "reference_loop", **base, "dim": a.loop_dim, "points": nl, "n_test": a.n_test, "ms_median": med, "ms_min": mn,
                              "grid_ms_median_same_dim": g_med}), flush=True)


if __name__ == "__main__":
    main()
