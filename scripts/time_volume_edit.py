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
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

LO, HI = T.BOX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    dev = torch.device("cuda")
    H, W, K, pose = T.study_view()
    C, target = 14, 2
    near, far = 4.0, 15.0
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, batch=a.batch, dims=a.dims, frame=[H, W], near=near, far=far, ins_num=C - 1)]
    move = T.rigid(0, series="volume")
    fr = D.ManipulationFrameRenderer(H, W, K, pose, [torch.from_numpy(move).float()], None,
                                     types.SimpleNamespace(N_importance=0, target_labels=[target]), ins_num=C - 1, rank=0, world=1)
    rays1, rays2 = fr.ori[None].contiguous(), torch.cat([fr.ori[None], fr.tar], 0)
    sets1, sets2 = [range(C)], [[l for l in range(C) if l != target], [target]]
    for pct in (5, 25, 100):
        set_cells, vol, cells = T.random_baked(pct, a.dims, C)
        grids = {"plain": F.LabelGrid.from_labels(torch.from_numpy(vol).to(dev), LO, HI, C),
                 "baked": F.BakedGrid.from_arrays(torch.from_numpy(vol).to(dev), torch.from_numpy(cells).to(dev), LO, HI, C)}
        for kind, grid in grids.items():
            for E in (1, 4, 16, 32):
                trans, labels = [T.rigid(e, series="volume") for e in range(E)], [e % C for e in range(E)]
                res = Ed.edit_volume(grid, trans, labels)

                def batch():
                    for _ in range(a.batch):
                        Ed.edit_volume(grid, trans, labels, out=res["grid"])

                t = T.time_events(batch, a.iters, a.warmup)
                lines.append({"leg": "edit_volume", "set_fraction": float(set_cells.mean()), "volume": kind, "E": E, "edit_ms_median": t.median / a.batch,
                              "edit_ms_min": t.min / a.batch, "claimed": int(res["claimed"].sum()), "collisions": int(res["hits"].sum())})
        baked = grids["baked"]
        edited = Ed.edit_volume(baked, [move], [target])["grid"]
        row = {"leg": "frame", "set_fraction": float(set_cells.mean())}
        for stop_name, stop in (("stop0", 0.0), ("stop256", 1.0 / 256.0)):
            t = T.time_host(lambda: Ed.render_preview(baked, H, W, K, pose, [move], [target], near=near, far=far, stop=stop), a.iters, a.warmup)
            row[stop_name + "_r2_preview_ms_median"], row[stop_name + "_r2_preview_ms_min"] = t.median, t.min
            t = T.time_host(lambda: Ed.render_preview(edited, H, W, K, pose, near=near, far=far, stop=stop), a.iters, a.warmup)
            row[stop_name + "_r1_preview_ms_median"], row[stop_name + "_r1_preview_ms_min"] = t.median, t.min
            for name, grid, rays, sets in (("r2", baked, rays2, sets2), ("r1", edited, rays1, sets1)):
                def batch():
                    for _ in range(a.batch):
                        grid.render_sets(rays, sets, near, far, stop)

                t = T.time_events(batch, a.iters, a.warmup)
                row[f"{stop_name}_{name}_render_ms_median"], row[f"{stop_name}_{name}_render_ms_min"] = t.median / a.batch, t.min / a.batch
        lines.append(row)
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
