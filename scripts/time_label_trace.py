"""Time the label trace (LabelGrid.trace_sets, editing.preview_frame) next to the manipulation frame it previews.

    python scripts/time_label_trace.py [--out profiles/label_trace/timing.jsonl]

One 640 x 480 view (the pose, intrinsics, transformation and box of scripts/time_manip_skip.py), a 128^3 label volume over [-8, 8)^3,
near 4 / far 15, ins_num 13 (C = 14).  The volumes are synthetic: cells labelled at random with probability 0, 5, 25 and 100 %, the
label uniform in 0 .. 13 (0 %: every ray walks the whole box and hits nothing, the longest walk there is).  Per volume and for
R = 1 (the plain frame) and R = 2 (one rigid move of label 2), median and minimum of ``--iters`` runs after ``--warmup``:

    trace_ms     ``dmnerf_label_trace`` alone on rays that are already there: HIP events round ``--batch`` back-to-back launches,
                 divided by the batch (one launch is too short for an event pair to resolve)
    preview_ms   one ``editing.preview_frame`` call end to end: the rays (``ManipulationFrameRenderer(models=None)``), the trace
                 and the reshapes; a host clock round the call and a device synchronise

and the fraction of pixels with a hit.  The last line is ONE dense ``manipulate_frame`` of the same view and transformation with the
benchmark's models (``--no-frame`` leaves it out): the frame the preview stands in for; its code is untouched by the trace.  There
is no earlier implementation of the trace: these are absolute times of this tree.  The first line records the device and its clocks
(sclk among them) as ``rocm-smi`` reports them (read-only).  One JSON object per line."""
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
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true", help="do not render the manipulation frame")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    import types
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    dev = torch.device("cuda")
    H, W, K, pose = T.study_view()
    C, target = 14, 2
    near, far = 4.0, 15.0
    trans = torch.tensor(T.rigid(), dtype=torch.float32)
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, batch=a.batch, dims=a.dims, frame=[H, W], near=near, far=far, ins_num=C - 1)]
    fr = D.ManipulationFrameRenderer(H, W, K, pose, [trans], None, types.SimpleNamespace(N_importance=0, target_labels=[target]),
                                     ins_num=C - 1, rank=0, world=1)
    rays = {1: fr.ori[None].contiguous(), 2: torch.cat([fr.ori[None], fr.tar], 0)}
    sets = {1: [range(C)], 2: [[l for l in range(C) if l != target], [target]]}
    edits = {1: ((), ()), 2: ([trans], [target])}
    for pct in (0, 5, 25, 100):
        lg = F.LabelGrid.from_labels(torch.from_numpy(T.random_labels(pct, a.dims, C)).to(dev), *T.BOX, C)
        for R in (1, 2):
            out = lg.trace_sets(rays[R], sets[R], near, far)
            row = {"leg": "trace", "labelled_fraction": float((lg.labels != F.UNLABELLED).float().mean()), "R": R,
                   "hit_fraction": float((out["label"] != F.UNLABELLED).float().mean())}

            def batch():
                for _ in range(a.batch):
                    lg.trace_sets(rays[R], sets[R], near, far)

            t = T.time_events(batch, a.iters, a.warmup)
            row["trace_ms_median"], row["trace_ms_min"] = t.median / a.batch, t.min / a.batch
            t = T.time_host(lambda: Ed.preview_frame(lg, H, W, K, pose, *edits[R], near=near, far=far), a.iters, a.warmup)
            row["preview_ms_median"], row["preview_ms_min"] = t.median, t.min
            lines.append(row)
    if not a.no_frame:
        import bench_common as B
        _, _, mc, mf = B.build_models(dev)
        args = types.SimpleNamespace(N_samples=64, N_importance=128, near=near, far=far, N_test=4096, target_labels=[target])

        def renderer():
            torch.manual_seed(7)
            return D.ManipulationFrameRenderer(H, W, K, pose.to(dev), [trans], (mc, mf), args, chunk=4096)

        with torch.no_grad():
            t = T.time_events(T.render_chunks, 1, 1, setup=renderer)
        lines.append({"leg": "manipulate_frame_dense", "runs": 1, "warmup": 1, "ms": t.median})
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
