"""Time the render that skips empty space (render.dm_nerf_fine_skip) against the dense fine-only render, by grid occupancy.

    python scripts/time_skip.py [--out profiles/skip/timing.jsonl]
    python scripts/time_skip.py --mfma-split f16x2 [--out profiles/skip_f16/timing.jsonl]      (the opt-in split-f16 kernels)

One 640 x 480 frame, 64 + 128 samples, chunks of 4096 rays, ins_num 13, the benchmark's models and camera.  The grids are synthetic:
a 128^3 box round the scene whose cells are set at random with probability 5, 10, 25, 50 and 100 %, ``outside="empty"`` so that the
occupancy is the fraction of in-box samples that is evaluated.  The 100 % row is the overhead of select, zero-fill and the
over-sized launch; the ``dense`` row is ``FrameRenderer`` without ``skip=`` in the same process.  Per row: HIP-event milliseconds
of the whole frame, median and minimum of ``--iters`` runs after ``--warmup``, rays/s, and the samples evaluated per level.  The
first line records the device and its clocks as ``rocm-smi`` reports them (read-only).  One JSON object per line."""
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    import types
    import bench_common as C
    from dm_nerf_amd import distributed as D, field as F
    from dm_nerf_amd.networks import render as R
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    H, W, K, c2w = T.study_view()
    c2w = c2w.to(dev)
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    if a.mfma_split:
        args.mfma_split = a.mfma_split
    lines = [T.device_line(iters=a.iters, warmup=a.warmup)]
    if a.mfma_split:
        lines[0]["mfma_split"] = a.mfma_split

    def renderer(**kw):
        return D.FrameRenderer(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=4096, n_samples=64, **kw)

    with torch.no_grad():
        t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=renderer)
        lines.append({"leg": "dense", "ms_median": t.median, "ms_min": t.min, "rays_per_s": H * W / t.median * 1e3})
        for pct in (5, 10, 25, 50, 100):
            grid = F.SkipGrid.from_bits(T.random_bits(pct, a.dims), *T.BOX, a.dims, outside="empty")
            t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=lambda: renderer(skip=grid))
            fr = renderer()
            n_eval = torch.zeros(2, dtype=torch.int64, device=dev)
            for i in range(fr.n_chunks):
                s, e = i * 4096, min((i + 1) * 4096, H * W)
                out = R.dm_nerf_fine_skip(torch.stack([fr.rays_o[s:e], fr.rays_d[s:e]]), None, None, mc, mf, fr.z_full[:e - s], args, grid)
                n_eval += out["n_eval"]
            lines.append({"leg": "skip", "grid_occupancy": float(grid.occupancy()), "ms_median": t.median, "ms_min": t.min,
                          "rays_per_s": H * W / t.median * 1e3, "n_eval": n_eval.tolist(), "n_dense": [H * W * 64, H * W * 192]})
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
