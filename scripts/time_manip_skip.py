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
records the device and its clocks as ``rocm-smi`` reports them (read-only).  One JSON object per line."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402


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
    T.require_gpu(__file__)
    tree = os.path.abspath(a.tree) if a.tree else T.ROOT
    sys.path.insert(0, tree)
    import types
    import bench_common as C
    from dm_nerf_amd import distributed as D, field as F
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    H, W, K, pose = T.study_view()
    pose = pose.to(dev)
    trans = torch.tensor(T.rigid(), dtype=torch.float32)
    args = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=4096, target_labels=[2])
    if a.mfma_split:
        args.mfma_split = a.mfma_split
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, tree=a.label or os.path.relpath(tree),
                           package_in_tree=os.path.relpath(os.path.dirname(os.path.abspath(D.__file__)), tree))]
    if a.mfma_split:
        lines[0]["mfma_split"] = a.mfma_split

    def renderer(**kw):
        torch.manual_seed(7)                                         # the same draws in every run and every row
        return D.ManipulationFrameRenderer(H, W, K, pose, [trans], (mc, mf), args, chunk=4096, **kw)

    with torch.no_grad():
        t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=renderer)
        lines.append({"leg": "dense", "ms_median": t.median, "ms_min": t.min, "rays_per_s": H * W / t.median * 1e3})
        for pct in (() if a.dense_only else (5, 10, 25, 50, 100)):
            grid = F.SkipGrid.from_bits(T.random_bits(pct, a.dims), *T.BOX, a.dims, outside="empty")
            t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=lambda: renderer(skip=grid))
            n_eval = t.last.n_eval.tolist()
            lines.append({"leg": "skip", "grid_occupancy": float(grid.occupancy()), "ms_median": t.median, "ms_min": t.min,
                          "rays_per_s": H * W / t.median * 1e3, "n_eval": n_eval, "evaluated_fraction": n_eval[0] / max(n_eval[1], 1)})
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
