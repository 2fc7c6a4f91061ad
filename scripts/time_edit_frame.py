"""Time the edited-frame path on the device (needs a MI355X and the built library):

  1. one 640 x 480 view of ``editing.manipulate_demo_path`` with T = 2 objects (a deformation and a rigid move), ins_num 13,
     N_test 4096 -- wall time with one synchronisation at the end, and the share of it spent in ``dmnerf_edit_rays`` and
     ``frame_products``;
  2. ``editing.frame_products`` on a 640 x 480 frame at C = 14 and C = 95 (HIP events, median of 50 warm calls: with an even count,
     the mean of the two middle runs) against what it
     replaces: the float maps copied to the host, ``to8b``, ``argmax`` and the ``torch.unique`` loop of ``render_label2img``.

    python scripts/time_edit_frame.py [--out profiles/edit_frame/edit_frame.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

from dm_nerf_amd import editing as E  # noqa: E402
from dm_nerf_amd.networks import dm_nerf as M  # noqa: E402
from oracle import ref_cpu as O  # noqa: E402

H, W = T.H, T.W


def events_ms(fn, warm=5, reps=50):
    t = T.time_events(fn, reps, warm)
    return dict(median_ms=t.median, min_ms=t.min, max_ms=t.max, reps=reps)


def host_products(rgb, ins, rgbs, color_dict, ins_map):
    """The reference's path: manipulator.py:472-488 with tools/visualizer.py:73-86, on host copies of the float maps."""
    t0 = time.perf_counter()
    rgb_h = rgb.cpu().numpy()
    rgb8 = (255 * np.clip(rgb_h, 0, 1)).astype(np.uint8)
    label = torch.argmax(ins, dim=-1)
    uniq = torch.unique(label).cpu()
    lab_h = label.cpu()
    img = np.zeros((H, W, 3))
    for l in uniq:
        key = str(int(l))
        if key in ins_map:
            img[lab_h == l] = rgbs[color_dict[str(ins_map[key])]]
    img = img.astype(np.uint8)
    mask = np.array(lab_h.numpy(), dtype=np.uint8)
    ins_h = ins.cpu().numpy()                                  # (the float object map also crosses the link in manipulator_eval, :294)
    return (time.perf_counter() - t0) * 1e3, rgb8, img, mask, ins_h.nbytes + rgb_h.nbytes


def time_products(C):
    gen = torch.Generator().manual_seed(C)
    frame = torch.rand(H * W, 2 * (3 + C), generator=gen).cuda()
    rgb, ins = frame[:, 0:3].reshape(H, W, 3), frame[:, 3:3 + C].reshape(H, W, C)
    rgbs = np.random.RandomState(1).randint(0, 256, size=(C, 3))
    color_dict = {str(k): k for k in range(C)}
    ins_map = {str(k): (k * 7) % C for k in range(0, C, 2)}
    lut = E.label_lut(C, rgbs, color_dict, ins_map)
    dev = events_ms(lambda: E.frame_products(rgb, ins, lut))
    rgb8, label, mask, img = E.frame_products(rgb, ins, lut)
    host = sorted(host_products(rgb, ins, rgbs, color_dict, ins_map)[0] for _ in range(5))
    _, h8, himg, hmask, nbytes = host_products(rgb, ins, rgbs, color_dict, ins_map)
    same = bool(np.array_equal(rgb8.cpu().numpy(), h8) and np.array_equal(img.cpu().numpy(), himg) and np.array_equal(mask.cpu().numpy(), hmask))
    read = H * W * 4 * (3 + C)
    return dict(C=C, device=dev, device_GBps_read=read / (dev["median_ms"] * 1e-3) / 1e9, host_median_ms=host[len(host) // 2],
                host_float_bytes=nbytes, device_out_bytes=H * W * 7 + H * W * 8, equal_to_host=same)


def time_demo_view():
    ins_num = 13
    models = []
    for seed in (721, 722):
        m = M.DM_NeRF(8, 256, 63, 27, [4], ins_num)
        m.load_state_dict(O.make_weights(seed, ins_num, **O.PEAKY))
        models.append(m.cuda().eval())
    K = O.dmsr_intrinsics(H, W)
    poses = [O.pose_spherical(75.0, -65.0, 7.0)] * 2
    objs = [dict(obj_name="a", tar_id=2, mani_mode="deform", deform_func="sin"), dict(obj_name="b", tar_id=4, mani_mode="translation")]
    objs_trans = {"b": [dict(transformation=[[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])] * 2}
    args = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=4096)
    rgbs = np.random.RandomState(1).randint(0, 256, size=(ins_num + 1, 3))
    tables = (rgbs, {str(k): k for k in range(ins_num + 1)}, {str(k): k for k in range(ins_num + 1)})
    out = {}

    def view():
        out.update(E.manipulate_demo_path(poses[1:], (H, W, K), models, args, objs, {"b": objs_trans["b"][1:]}, *tables))

    with torch.no_grad():
        ts = [ms / 1e3 for ms in T.time_host(view, 3, 0).runs]  # the first one warms up
    off = np.stack([E.deform_offsets(H, "sin", 1), np.zeros(H)])
    rays = events_ms(lambda: E.edit_rays(H, W, K, poses, [1, 0], off))
    return dict(T=2, ins_num=ins_num, N_test=args.N_test, view_s=min(ts[1:]), views_s=ts, shape=list(out["rgb8"].shape),
                edit_rays=rays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    rec = dict(device=torch.cuda.get_device_name(0), frame=[H, W], demo_view=time_demo_view(), products=[time_products(C) for C in (14, 95)])
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
