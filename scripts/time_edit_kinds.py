"""Time one removal frame against the same frame rendered as a rigid move (needs a MI355X and the built library):

  one 640 x 480 view through ``distributed.manipulate_frame``, ins_num 13, 64 + 128 samples, N_test 4096, the same models, pose
  and target label -- once with ``trans_list = [Remove()]`` (1 coarse + 2 fine launches of the original rays per chunk, 192
  samples in the final level), once with ``trans_list = [matrix]`` (T = 1: 2 coarse + 4 fine launches, 320 samples in the final
  level).  Each is warmed up, then timed ``--reps`` times with HIP events around the whole frame; the median is reported (with an
  even ``--reps``, the mean of the two middle runs).

    python scripts/time_edit_kinds.py [--reps 7] [--out profiles/edit_kinds/edit_kinds.json]
"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

from dm_nerf_amd import distributed as D  # noqa: E402
from dm_nerf_amd import editing as E  # noqa: E402
from dm_nerf_amd.networks import dm_nerf as M  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

H, W, INS, LABEL = T.H, T.W, 13, 2


def frame_ms(fn, warm, reps):
    t = T.time_events(fn, reps, warm)
    return dict(median_ms=t.median, min_ms=t.min, max_ms=t.max, runs_ms=t.runs, warm=warm, reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5 timed runs")
    T.require_gpu(__file__)
    models = []
    for seed in (721, 722):
        m = M.DM_NeRF(8, 256, 63, 27, [4], INS)
        m.load_state_dict(O.make_weights(seed, INS, **O.PEAKY))
        models.append(m.cuda().eval())
    K = O.dmsr_intrinsics(H, W)
    pose = O.pose_spherical(75.0, -65.0, 7.0).cuda()
    move = torch.tensor([[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])
    args = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=4096, target_labels=[LABEL])
    rec = dict(device=torch.cuda.get_device_name(0), frame=[H, W], ins_num=INS, N_samples=64, N_importance=128, N_test=4096, label=LABEL)
    with torch.no_grad():
        for name, trans in (("remove", [E.Remove()]), ("move_T1", [move])):
            rec[name] = frame_ms(lambda: D.manipulate_frame(H, W, K, pose, trans, models, args), a.warm, a.reps)
            frame = D.manipulate_frame(H, W, K, pose, trans, models, args)
            rec[name]["finite"] = bool(torch.isfinite(frame[0]).all())
            rec[name]["labels_in_frame"] = sorted(int(v) for v in torch.unique(frame[1].argmax(-1)).cpu())
    rec["move_over_remove"] = rec["move_T1"]["median_ms"] / rec["remove"]["median_ms"]
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
