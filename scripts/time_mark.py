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
``rocm-smi --showclocks`` reports them (read-only).  One JSON object per line.

The quality of a ``from_views`` grid on a trained field (occupancy, evaluated fraction, PSNR against the dense render of held-out
poses) is NOT measured by this script."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_skip import clocks, time_frame  # noqa: E402


def time_call(fn, iters, warmup):
    ms = []
    for it in range(warmup + iters):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(b.elapsed_time(e))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--mfma-split", default=None, choices=["f16x2"], help="render with args.mfma_split (default: the f32 kernels)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import types
    import bench_common as C
    from dm_nerf_amd import distributed as D, field as F
    from oracle import ref_cpu as O
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    H, W = 480, 640
    K = O.dmsr_intrinsics(H, W)
    c2w = O.pose_spherical(30.0, -65.0, 7.0).to(dev)
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    if a.mfma_split:
        args.mfma_split = a.mfma_split
    lo, hi = (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)
    lines = [{"leg": "device", "name": torch.cuda.get_device_name(0), "clocks": clocks(), "iters": a.iters, "warmup": a.warmup}]
    if a.mfma_split:
        lines[0]["mfma_split"] = a.mfma_split

    def renderer(**kw):
        return D.FrameRenderer(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=4096, n_samples=64, **kw)

    def leg(name, make, **extra):
        med, mn = time_frame(make, a.iters, a.warmup)
        lines.append(dict({"leg": name, "ms_median": med, "ms_min": mn, "rays_per_s": H * W / med * 1e3}, **extra))

    grid = F.SkipGrid.empty(lo, hi, a.dims, device=dev)

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
        scratch = F.SkipGrid.empty(lo, hi, a.dims, device=dev)
        first = time_call(lambda: (scratch.bits.zero_(), scratch.mark(ro, rd, z, w)), a.iters, a.warmup)       # (with the 256 KB clear)
        steady = time_call(lambda: scratch.mark(ro, rd, z, w), a.iters, a.warmup)
        dil = time_call(lambda: grid.dilated(1), a.iters, a.warmup)
        lines.append({"leg": "passes", "samples": 4096 * 192, "mark_from_empty_ms": first, "mark_saturated_ms": steady,
                      "dilate1_ms": dil, "dims": a.dims})
    text = "\n".join(json.dumps(l) for l in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
