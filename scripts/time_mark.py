"""Time the marking render (FrameRenderer(mark=grid) -> render.dm_nerf_fine_mark) against the dense fine-only frame.

    python scripts/time_mark.py [--out profiles/mark/timing_f32.jsonl]
    python scripts/time_mark.py --mfma-split f16x2 [--out profiles/mark/timing_f16x2.jsonl]      (the opt-in split-f16 kernels)

One 640 x 480 frame, 64 + 128 samples, chunks of 4096 rays, ins_num 13, the benchmark's models and camera; a 128^3 grid over
[-8, 8)^3, marked at threshold 0 at both levels.  Legs, in this order: ``dense`` (``FrameRenderer`` without ``mark=``: the code of the
dense route is untouched by ``mark=``), ``mark`` into a grid that starts empty on every run, ``mark_saturated`` into a grid that
already holds the frame's bits (the steady state: the mark kernel only loads), and ``dense`` again -- the two dense legs give the
run-to-run spread the overhead has to be read against.  Per leg: HIP-event milliseconds of the whole frame, median and minimum of
``--iters`` runs after ``--warmup``.  The last line times the two stand-alone passes on one chunk's worth of samples:
``SkipGrid.mark`` on 4096 x 192 samples and ``dilated(1)`` of the 128^3 grid.  The first line records the device and its clocks as
``rocm-smi`` reports them (read-only).  One JSON object per line.

The quality of a ``from_views`` grid on a trained field (occupancy, evaluated fraction, PSNR against the dense render of held-out
poses) is NOT measured by this script."""
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

    def leg(name, make, **extra):
        t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=make)
        lines.append(dict({"leg": name, "ms_median": t.median, "ms_min": t.min, "rays_per_s": H * W / t.median * 1e3}, **extra))

    def call(fn):
        t = T.time_events(fn, a.iters, a.warmup)
        return t.median, t.min

    grid = F.SkipGrid.empty(*T.BOX, a.dims, device=dev)

    def fresh():
        grid.bits.zero_()
        return renderer(mark=grid)

    with torch.no_grad():
        leg("dense", renderer)
        leg("mark", fresh)
        leg("mark_saturated", lambda: renderer(mark=grid), grid_occupancy=float(grid.occupancy()))
        leg("dense", renderer)
        fr = renderer()
        z, w = torch.rand(4096, 192, device=dev) * 11.0 + 4.0, torch.rand(4096, 192, device=dev)
        ro, rd = fr.rays_o[:4096].contiguous(), fr.rays_d[:4096].contiguous()
        scratch = F.SkipGrid.empty(*T.BOX, a.dims, device=dev)
        first = call(lambda: (scratch.bits.zero_(), scratch.mark(ro, rd, z, w)))       # (with the 256 KB clear)
        steady = call(lambda: scratch.mark(ro, rd, z, w))
        dil = call(lambda: grid.dilated(1))
        lines.append({"leg": "passes", "samples": 4096 * 192, "mark_from_empty_ms": first, "mark_saturated_ms": steady,
                      "dilate1_ms": dil, "dims": a.dims})
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
