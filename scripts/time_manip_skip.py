"""Time the manipulation render that skips empty space (``manipulate_frame(..., skip=grid)``) against the dense one, by grid occupancy.

    python scripts/time_manip_skip.py [--out profiles/manip_skip/timing_f32.jsonl]
    python scripts/time_manip_skip.py --mfma-split f16x2 [--out profiles/manip_skip/timing_f16x2.jsonl]
    python scripts/time_manip_skip.py --tree ../parent --label parent --dense-only [--mfma-split f16x2]     (the yardstick: another checkout's dense frame)

One 640 x 480 frame, 64 + 128 samples, chunks of 4096 rays, ins_num 13, the benchmark's models and camera, one rigid move (T = 1):
2 + 4 T = 6 network launches per chunk, 1152 samples per ray.  The grids are synthetic: a 128^3 box round the scene whose cells are
set at random with probability 5, 10, 25, 50 and 100 %, ``outside="empty"``.  The ``dense`` row is ``ManipulationFrameRenderer``
without ``skip=``; with ``--tree`` the package is imported from that checkout instead of this one (its library must be built), which
is how the parent commit's dense frame is timed in the same session.  Per row: HIP-event milliseconds of the whole frame, median and
minimum of ``--iters`` runs after ``--warmup``, rays/s, and ``n_eval`` = (samples evaluated, samples) of the frame.  The first line
records the device and its clocks as ``rocm-smi --showclocks`` reports them (read-only).  One JSON object per line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {"error": r.stderr[-200:]}
    except Exception as e:                                           # the tool is optional
        return {"error": repr(e)}


def time_frame(make, iters, warmup):
    """``make()`` -> a ManipulationFrameRenderer; -> (median ms, min ms, the last renderer) of rendering all its chunks."""
    ms = []
    for it in range(warmup + iters):
        fr = make()
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        for i in range(fr.n_chunks):
            fr.step(i)
        e.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(b.elapsed_time(e))
    return float(np.median(ms)), float(np.min(ms)), fr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--mfma-split", default=None, choices=["f16x2"], help="render with args.mfma_split (default: the f32 kernels)")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (default: the one this script lies in)")
    ap.add_argument("--label", default=None, help="what to record as the tree instead of its path")
    ap.add_argument("--dense-only", action="store_true", help="time the dense frame only (a checkout without skip=)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    import types
    import bench_common as C
    from dm_nerf_amd import distributed as D, field as F
    from oracle import ref_cpu as O
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    H, W = 480, 640
    K = O.dmsr_intrinsics(H, W)
    pose = O.pose_spherical(30.0, -65.0, 7.0).to(dev)
    ang = 0.2
    trans = torch.tensor([[np.cos(ang), -np.sin(ang), 0., 0.3], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]],
                         dtype=torch.float32)
    args = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=4096, target_labels=[2])
    if a.mfma_split:
        args.mfma_split = a.mfma_split
    lo, hi = (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)
    lines = [{"leg": "device", "name": torch.cuda.get_device_name(0), "clocks": clocks(), "iters": a.iters, "warmup": a.warmup,
              "tree": a.label or os.path.relpath(tree),
              "package_in_tree": os.path.relpath(os.path.dirname(os.path.abspath(D.__file__)), tree)}]
    if a.mfma_split:
        lines[0]["mfma_split"] = a.mfma_split

    def renderer(**kw):
        torch.manual_seed(7)                                         # the same draws in every run and every row
        return D.ManipulationFrameRenderer(H, W, K, pose, [trans], (mc, mf), args, chunk=4096, **kw)

    with torch.no_grad():
        med, mn, _ = time_frame(renderer, a.iters, a.warmup)
        lines.append({"leg": "dense", "ms_median": med, "ms_min": mn, "rays_per_s": H * W / med * 1e3})
        for pct in (() if a.dense_only else (5, 10, 25, 50, 100)):
            occ = np.random.RandomState(pct).rand(a.dims, a.dims, a.dims) < pct / 100.0
            words = np.packbits(occ.reshape(-1), bitorder="little")
            words = np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)
            grid = F.SkipGrid.from_bits(words, lo, hi, a.dims, outside="empty")
            med, mn, fr = time_frame(lambda: renderer(skip=grid), a.iters, a.warmup)
            n_eval = fr.n_eval.tolist()
            lines.append({"leg": "skip", "grid_occupancy": float(grid.occupancy()), "ms_median": med, "ms_min": mn,
                          "rays_per_s": H * W / med * 1e3, "n_eval": n_eval, "evaluated_fraction": n_eval[0] / max(n_eval[1], 1)})
    text = "\n".join(json.dumps(l) for l in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
