"""Time the instance-AP evaluation of one 640 x 480 frame (``evaluator.ins_eval_device``, csrc/ins_eval.hip).

    python scripts/time_ins_eval.py                          # device: HIP-event ms per frame at ins_num 13 / 59 / 93
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/time_ins_eval.py --iters 5      # kernel breakdown
    python scripts/time_ins_eval.py --reference-cpu REF      # host leg: REF's own networks/evaluator.py ins_eval (CPU torch),
                                                             # wall time and peak RSS per frame, one child process per ins_num

The frames are synthetic: blocky ground-truth labels (40-pixel tiles, 3 % noise) over ``ins_num - 2`` objects, predictions a
relabelled, shifted, noisier copy, confidences from a few levels plus noise (so that medians of even counts occur).  One JSON
line per ins_num.
"""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

H, W = T.H, T.W


def frame(ins_num, seed=0):
    rng = np.random.default_rng(seed + ins_num)
    n_gt = ins_num - 2
    small = rng.choice(n_gt, size=(-(-H // 40), -(-W // 40)))
    gt = np.kron(small, np.ones((40, 40), dtype=np.int64))[:H, :W]
    flip = rng.random((H, W)) < 0.03
    gt[flip] = rng.integers(0, n_gt, size=int(flip.sum()))
    pl = np.roll(rng.permutation(ins_num)[gt], shift=(3, 5), axis=(0, 1))
    flip = rng.random((H, W)) < 0.05
    pl[flip] = rng.integers(0, ins_num, size=int(flip.sum()))
    conf = (rng.choice(np.float32([0.5, 0.625, 0.75, 0.875]), size=(H, W))
            + rng.integers(0, 64, size=(H, W)).astype(np.float32) / np.float32(4096)).astype(np.float32)
    return pl, conf, gt


def device(ins_nums, iters, warmup):
    import torch
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator as E
    lib = _lib.load()
    for C in ins_nums:
        pl, conf, gt = (torch.from_numpy(x).cuda() for x in frame(C))
        rows = torch.unique(gt)
        t = T.time_events(lambda: E.ins_eval_device(pl, conf, gt, rows, C), iters, warmup)
        _, ap, _ = E.ins_eval_device(pl, conf, gt, rows, C)
        print(json.dumps({"leg": "device", "ins_num": C, "frame": [H, W], "gt_num": int(rows.numel()), "iters": iters,
                          "ms_median": t.median, "ms_min": t.min,
                          "work_bytes": int(lib.dmnerf_ins_eval_work_bytes(H * W, C)), "ap": [round(float(v), 4) for v in ap.cpu()]}),
              flush=True)


def reference_child(ref, C):
    """One frame through the reference's own ins_eval on the CPU (run in a child: its peak RSS is the figure)."""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ref)
    import networks.evaluator as R
    pl, conf, gt = frame(C)
    pred = torch.full((H, W, C), 0.01)
    pred.scatter_(-1, torch.from_numpy(pl)[..., None], torch.from_numpy(conf)[..., None])
    g = torch.from_numpy(gt)
    rows = torch.unique(g)
    gt_ins = torch.zeros(H, W, C)
    gt_ins[..., :len(rows)] = F.one_hot(g)[..., rows].float()
    t0 = time.perf_counter()
    _, ap, _ = R.ins_eval(pred, gt_ins, len(rows), C)
    dt = time.perf_counter() - t0
    print(json.dumps({"leg": "reference_cpu", "ins_num": C, "frame": [H, W], "gt_num": len(rows), "threads": torch.get_num_threads(),
                      "s": dt, "ap": [round(float(v), 4) for v in ap]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ins-num", type=int, nargs="*", default=[13, 59, 93])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference-cpu", metavar="REF", help="checkout of the reference (host leg; no GPU used)")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        reference_child(a.reference_cpu, a.child)
        return
    if a.reference_cpu:
        for C in a.ins_num:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reference-cpu", a.reference_cpu, "--child", str(C)],
                               capture_output=True, text=True)
            line = json.loads(r.stdout.strip().split("\n")[-1])
            line["peak_rss_gb"] = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 2 ** 20   # (max over children so far)
            print(json.dumps(line), flush=True)
        return
    T.require_gpu(__file__)                                          # (the two host legs above use no device)
    device(a.ins_num, a.iters, a.warmup)


if __name__ == "__main__":
    main()
