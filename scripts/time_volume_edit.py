"""Time ``editing.edit_volume`` (csrc/volume_edit.hip) and the frame it makes cheaper: an edit previewed through ray sets on the
original volume against the same frame of the edited volume.

    python scripts/time_volume_edit.py [--out profiles/volume_edit/timing.jsonl]

The configuration of scripts/time_baked.py: one 640 x 480 view (its pose, intrinsics and box), a 128^3 volume over [-8, 8)^3, near 4 /
far 15, ins_num 13 (C = 14), synthetic volumes with 5 / 25 / 100 % of the cells set (label uniform in 0 .. 13, colour logits N(0, 1),
density uniform in 0 .. 8).  Median and minimum of ``--iters`` runs after ``--warmup``; the first line records the device and its
clocks (sclk among them, read-only).

    edit_ms          ``edit_volume`` with E = 1, 4, 16, 32 rigid moves (a small rotation and a shift each, labels 0 .. 13 in turn), on
                     the plain and on the baked volume, ``out=`` given: HIP events round ``--batch`` back-to-back calls / the batch
                     (the entries are packed on the host in every call: what a caller pays)
    r2_preview_ms    one ``render_preview`` of ONE rigid move through ray sets (R = 2) on the original volume, host clock and a device
                     synchronise -- this route's code is the parent commit's: the yardstick
    r1_preview_ms    the same frame as ``render_preview`` without edits (R = 1) on the edited volume, timed the same way
    r2_render_ms / r1_render_ms   ``dmnerf_baked_render`` alone for the two routes, on rays that are already there (HIP events round
                     ``--batch`` back-to-back launches / the batch, as scripts/time_baked.py's ``render_ms``)

The ``edit_volume`` times are absolute times of this tree: there is no earlier implementation.  One JSON object per line."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_label_trace import time_host  # noqa: E402
from time_manip_skip import clocks  # noqa: E402
from time_mark import time_call  # noqa: E402

LO, HI = (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)


def rigid(e):
    """The e-th rigid move: a rotation by 0.1 + 0.02 e about z and a shift that grows with e."""
    ang = 0.1 + 0.02 * e
    return np.array([[np.cos(ang), -np.sin(ang), 0., 0.3 + 0.05 * e], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1 * (e % 5)],
                     [0., 0., 0., 1.]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_volume_edit.py measures on the GPU: no device found")
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    from oracle import ref_cpu as O
    dev = torch.device("cuda")
    H, W, C, target = 480, 640, 14, 2
    near, far = 4.0, 15.0
    K = O.dmsr_intrinsics(H, W)
    pose = O.pose_spherical(30.0, -65.0, 7.0)
    lines = [{"leg": "device", "name": torch.cuda.get_device_name(0), "clocks": clocks(), "iters": a.iters, "warmup": a.warmup,
              "batch": a.batch, "dims": a.dims, "frame": [H, W], "near": near, "far": far, "ins_num": C - 1}]
    move = rigid(0)
    fr = D.ManipulationFrameRenderer(H, W, K, pose, [torch.from_numpy(move).float()], None,
                                     types.SimpleNamespace(N_importance=0, target_labels=[target]), ins_num=C - 1, rank=0, world=1)
    rays1, rays2 = fr.ori[None].contiguous(), torch.cat([fr.ori[None], fr.tar], 0)
    sets1, sets2 = [range(C)], [[l for l in range(C) if l != target], [target]]
    for pct in (5, 25, 100):
        rng = np.random.RandomState(pct)
        shape = (a.dims,) * 3
        set_cells = rng.rand(*shape) < pct / 100.0
        vol = rng.randint(0, C, size=shape).astype(np.uint8)
        vol[~set_cells] = F.UNLABELLED
        cells = np.zeros(shape + (4,), np.float32)
        cells[..., :3] = rng.randn(*shape, 3)
        cells[..., 3] = rng.uniform(0.0, 8.0, size=shape)
        cells[~set_cells] = 0.0
        grids = {"plain": F.LabelGrid.from_labels(torch.from_numpy(vol).to(dev), LO, HI, C),
                 "baked": F.BakedGrid.from_arrays(torch.from_numpy(vol).to(dev), torch.from_numpy(cells).to(dev), LO, HI, C)}
        for kind, grid in grids.items():
            for E in (1, 4, 16, 32):
                trans, labels = [rigid(e) for e in range(E)], [e % C for e in range(E)]
                res = Ed.edit_volume(grid, trans, labels)

                def batch():
                    for _ in range(a.batch):
                        Ed.edit_volume(grid, trans, labels, out=res["grid"])

                med, mn = time_call(batch, a.iters, a.warmup)
                lines.append({"leg": "edit_volume", "set_fraction": float(set_cells.mean()), "volume": kind, "E": E, "edit_ms_median": med / a.batch,
                              "edit_ms_min": mn / a.batch, "claimed": int(res["claimed"].sum()), "collisions": int(res["hits"].sum())})
        baked = grids["baked"]
        edited = Ed.edit_volume(baked, [move], [target])["grid"]
        row = {"leg": "frame", "set_fraction": float(set_cells.mean())}
        for stop_name, stop in (("stop0", 0.0), ("stop256", 1.0 / 256.0)):
            row[stop_name + "_r2_preview_ms_median"], row[stop_name + "_r2_preview_ms_min"] = time_host(
                lambda: Ed.render_preview(baked, H, W, K, pose, [move], [target], near=near, far=far, stop=stop), a.iters, a.warmup)
            row[stop_name + "_r1_preview_ms_median"], row[stop_name + "_r1_preview_ms_min"] = time_host(
                lambda: Ed.render_preview(edited, H, W, K, pose, near=near, far=far, stop=stop), a.iters, a.warmup)
            for name, grid, rays, sets in (("r2", baked, rays2, sets2), ("r1", edited, rays1, sets1)):
                def batch():
                    for _ in range(a.batch):
                        grid.render_sets(rays, sets, near, far, stop)

                med, mn = time_call(batch, a.iters, a.warmup)
                row[f"{stop_name}_{name}_render_ms_median"], row[f"{stop_name}_{name}_render_ms_min"] = med / a.batch, mn / a.batch
        lines.append(row)
    text = "\n".join(json.dumps(l) for l in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
