"""Time the image scores of a rendered frame, SSIM + PSNR (``evaluator.img_metrics_device``, csrc/img_metrics.hip), at 480 x 640 x 3.

    python scripts/time_img_metrics.py                        # device leg and host leg, P = 1 and P = 10, one JSON line each
    python scripts/time_img_metrics.py --skip-host            # device leg only
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/time_img_metrics.py --skip-host --iters 5      # kernel breakdown

Device leg: HIP events around each of ``--iters`` warm calls after a warm-up burst (median, min, max in microseconds), and around one
burst of ``--iters`` back-to-back calls (per-call time with the launch gaps hidden by the queue).
Host leg: the path a user has without the device entry -- ``rgb.cpu().numpy()`` of every frame (the copy synchronises) and the
numpy / scipy restatement of the two ``skimage.metrics`` calls (tests/_img_metrics_restate.py, form (a): the filters skimage
itself calls) -- wall time per frame, at most 16 threads.
The frames are views of the analytic scene (oracle/analytic_scene.py) against a noisy copy (sd 0.02)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

sys.path.insert(0, os.path.join(T.ROOT, "tests"))
H, W, C = 480, 640, 3


def frames(P):
    import _img_metrics_restate as RS
    gt0 = RS.scene_view(H, W)
    rng = np.random.default_rng(0)
    gt = np.stack([np.roll(gt0, 7 * i, axis=1) for i in range(P)])
    pred = np.clip(gt + rng.normal(0, 0.02, gt.shape), 0, 1).astype(np.float32)
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    T.require_gpu(__file__)
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import _img_metrics_restate as RS
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator as E
    lib = _lib.load()
    for P in a.frames:
        pred_h, gt_h = frames(P)
        pred, gt = torch.from_numpy(pred_h).cuda(), torch.from_numpy(gt_h).cuda()
        call = T.time_events(lambda: E.img_metrics_device(pred, gt), a.iters, a.warmup)

        def in_a_burst():
            for _ in range(a.iters):
                E.img_metrics_device(pred, gt)

        burst = 1e3 * T.time_events(in_a_burst, 1, 0).median / a.iters
        s, p = E.img_metrics_device(pred, gt)
        want = [RS.ssim_uniform(pred_h[i], gt_h[i]) for i in range(P)]
        print(json.dumps({"leg": "device", "frames": P, "shape": [H, W, C], "iters": a.iters, "us_median": 1e3 * call.median,
                          "us_min": 1e3 * call.min, "us_max": 1e3 * call.max, "us_per_call_in_a_burst": burst,
                          "us_per_frame_in_a_burst": burst / P, "work_bytes": int(lib.dmnerf_img_metrics_work_bytes(P, H, W, C)),
                          "ssim": [float(v) for v in s.cpu()], "psnr": [float(v) for v in p.cpu()],
                          "max_abs_delta_ssim_vs_host": float(np.max(np.abs(np.array(want) - s.cpu().numpy())))}), flush=True)
        if a.skip_host:
            continue

        def host():
            for i in range(P):
                rgb = pred[i].cpu().numpy()                # tester.py:89-90: the copy and its synchronisation, per pose
                RS.psnr_restate(rgb, gt_h[i])
                RS.ssim_uniform(rgb, gt_h[i])

        t = T.time_host(host, a.host_iters, 0)
        print(json.dumps({"leg": "host", "frames": P, "shape": [H, W, C], "iters": a.host_iters, "threads": torch.get_num_threads(),
                          "ms_per_frame_median": t.median / P, "ms_per_frame_min": t.min / P, "ms_per_frame_max": t.max / P}), flush=True)


if __name__ == "__main__":
    main()
