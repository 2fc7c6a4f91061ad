"""Time the baked field volume (field.bake_grid, BakedGrid.render_sets, editing.render_preview) next to the hard preview and the
manipulation frame it stands in for, and -- ``--quality`` -- measure how well the proxies agree with rendered frames.

    python scripts/time_baked.py [--out profiles/baked/timing.jsonl]
    python scripts/time_baked.py --quality [--out profiles/baked/quality.jsonl]

Timing follows scripts/time_label_trace.py: one 640 x 480 view (its pose, intrinsics, transformation and box), a 128^3 volume over
[-8, 8)^3, near 4 / far 15, ins_num 13 (C = 14), synthetic volumes with 0 / 5 / 25 / 100 % of the cells set (label uniform in
0 .. 13, colour logits N(0, 1), density uniform in 0 .. 8: a cell of 0.125 then takes up to 63 % of what reaches it).  Median and
minimum of ``--iters`` runs after ``--warmup``; the first line records the device and its clocks (sclk among them, read-only):

    bake_ms          ``field.bake_grid`` of the benchmark's fine network over an occupancy grid with that share of cells set, f32
                     kernels and ``split="f16x2"`` (the network passes dominate; HIP events round the call)
    render_ms        ``dmnerf_baked_render`` alone on rays that are already there, R = 1 (the plain frame) and R = 2 (one rigid move
                     of label 2), ``stop = 0`` and ``stop = 1/256``: HIP events round ``--batch`` back-to-back launches / the batch
    preview_ms       one ``editing.render_preview`` end to end (rays, render, reshapes), host clock and a device synchronise
    hard_preview_ms  ``editing.preview_frame`` of the same volume, view and edit, timed the same way in the same session

and ONE dense ``manipulate_frame`` of the same view (``--no-frame`` leaves it out).  There is no earlier implementation of the baked
render: these are absolute times of this tree, with the hard preview and the dense frame as yardsticks.

``--quality`` (analytic scene only): the training loop of tests/test_gpu_convergence.py as ``_timing.train_analytic`` runs it (``--steps`` steps of 3072 rays on the
twelve 120 x 160 views of oracle/analytic_scene.py), then ``SkipGrid.from_model`` and ``bake_grid`` over [-8, 8)^3 at 128^3, per
``--sigma-threshold`` value.  On held-out poses: PSNR of ``render_preview``'s ``rgb`` against the dense ``render_frame`` (all pixels,
and the pixels the dense frame gives to an object), and the share of pixels whose label agrees with the dense argmax for
``render_preview`` and for ``preview_frame`` (a pixel without a label counts as the field's "nothing" class).  The same three
numbers for one rigid move of one sphere against ``manipulate_frame``.  One JSON object per line."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

LO, HI = T.BOX


def timing(a, lines):
    import bench_common as B
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    dev = torch.device("cuda")
    H, W, K, pose = T.study_view()
    C, target = 14, 2
    near, far = 4.0, 15.0
    trans = torch.tensor(T.rigid(), dtype=torch.float32)
    lines[0].update({"batch": a.batch, "dims": a.dims, "frame": [H, W], "near": near, "far": far, "ins_num": C - 1})
    _, _, mc, mf = B.build_models(dev)
    fr = D.ManipulationFrameRenderer(H, W, K, pose, [trans], None, types.SimpleNamespace(N_importance=0, target_labels=[target]),
                                     ins_num=C - 1, rank=0, world=1)
    rays = {1: fr.ori[None].contiguous(), 2: torch.cat([fr.ori[None], fr.tar], 0)}
    sets = {1: [range(C)], 2: [[l for l in range(C) if l != target], [target]]}
    edits = {1: ((), ()), 2: ([trans], [target])}
    for pct in (0, 5, 25, 100):
        set_cells, vol, cells = T.random_baked(pct, a.dims, C)
        occ = F.SkipGrid.from_bits(T.pack_bits(set_cells), LO, HI, a.dims)
        with torch.no_grad():
            for split in (None, "f16x2"):
                t = T.time_events(lambda: F.bake_grid(mf, occ, split=split), a.iters, a.warmup)
                lines.append({"leg": "bake_grid", "set_fraction": float(set_cells.mean()), "split": split or "f32", "bake_ms_median": t.median,
                              "bake_ms_min": t.min})
        bg = F.BakedGrid.from_arrays(torch.from_numpy(vol).to(dev), torch.from_numpy(cells).to(dev), LO, HI, C)
        for R in (1, 2):
            row = {"leg": "render", "set_fraction": float(set_cells.mean()), "R": R}
            for name, stop in (("stop0", 0.0), ("stop256", 1.0 / 256.0)):
                out = bg.render_sets(rays[R], sets[R], near, far, stop)
                row[name + "_mean_segments"] = float(out["nseg"].float().mean())
                row[name + "_mean_acc"] = float(out["acc"].mean())

                def batch():
                    for _ in range(a.batch):
                        bg.render_sets(rays[R], sets[R], near, far, stop)

                t = T.time_events(batch, a.iters, a.warmup)
                row[name + "_render_ms_median"], row[name + "_render_ms_min"] = t.median / a.batch, t.min / a.batch
                t = T.time_host(lambda: Ed.render_preview(bg, H, W, K, pose, *edits[R], near=near, far=far, stop=stop), a.iters, a.warmup)
                row[name + "_preview_ms_median"], row[name + "_preview_ms_min"] = t.median, t.min
            t = T.time_host(lambda: Ed.preview_frame(bg, H, W, K, pose, *edits[R], near=near, far=far), a.iters, a.warmup)
            row["hard_preview_ms_median"], row["hard_preview_ms_min"] = t.median, t.min
            lines.append(row)
    if not a.no_frame:
        args = types.SimpleNamespace(N_samples=64, N_importance=128, near=near, far=far, N_test=4096, target_labels=[target])

        def renderer():
            torch.manual_seed(7)
            return D.ManipulationFrameRenderer(H, W, K, pose.to(dev), [trans], (mc, mf), args, chunk=4096)

        with torch.no_grad():
            t = T.time_events(T.render_chunks, 1, 1, setup=renderer)
        lines.append({"leg": "manipulate_frame_dense", "runs": 1, "warmup": 1, "ms": t.median})


def quality(a, lines):
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    from oracle import analytic_scene as S
    dev = torch.device("cuda:0")
    H, W, C = 120, 160, 14
    t0 = time.perf_counter()
    mc, mf = T.train_analytic(a.steps, dev)
    torch.cuda.synchronize()
    lines[0].update({"scene": "analytic scene only", "train_steps": a.steps, "train_s": time.perf_counter() - t0, "frame": [H, W],
                     "dims": a.dims, "box": [LO, HI]})
    K = S.dmsr_intrinsics(H, W)
    poses = [S.pose_spherical(th, -65.0, 7.0) for th in (17.0, 77.0, 197.0)]     # none of the twelve training views
    rargs = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    psnr = lambda x, y: float(-10.0 * torch.log10(((x.double() - y.double()) ** 2).mean()))
    as_label = lambda l: torch.where(l == 255, torch.full_like(l, C - 1), l).long()
    with torch.no_grad():
        occ = F.SkipGrid.from_model(mf, LO, HI, a.dims)
        dense = [D.render_frame(H, W, K, p.to(dev), (mc, mf), S.NEAR, S.FAR, rargs) for p in poses]
        for thr in a.sigma_threshold:
            baked = F.bake_grid(mf, occ, sigma_threshold=thr)
            labelled = float((baked.labels != 255).float().mean())
            rows = {"psnr_all": [], "psnr_object_pixels": [], "agree_render_preview": [], "agree_preview_frame": []}

            def score(soft, hard, rgb, ins):
                want = ins.argmax(-1)
                obj = want < S.N_OBJECTS
                rows["psnr_all"].append(psnr(soft["rgb"], rgb))
                rows["psnr_object_pixels"].append(psnr(soft["rgb"][obj], rgb[obj]))
                rows["agree_render_preview"].append(float((as_label(soft["label"]) == want).float().mean()))
                rows["agree_preview_frame"].append(float((as_label(hard["label"]) == want).float().mean()))

            for p, (rgb, ins, _) in zip(poses, dense):
                score(Ed.render_preview(baked, H, W, K, p, near=S.NEAR, far=S.FAR), Ed.preview_frame(baked, H, W, K, p, near=S.NEAR, far=S.FAR),
                      rgb, ins)
            lines.append({"leg": "held_out_views", "sigma_threshold": thr, "occupancy": float(occ.occupancy()), "labelled_fraction": labelled,
                          "views": len(poses), **{k: float(np.mean(v)) for k, v in rows.items()}, "per_view": dict(rows)})
            # one rigid move of the first sphere: its label is the channel the matching gave it, read from the cell of its centre
            centre = np.asarray(S.SPHERES[0][0])
            i, j, k = [int(np.floor((centre[x] - LO[x]) / (HI[x] - LO[x]) * a.dims)) for x in range(3)]
            target = int(baked.labels[i, j, k])
            if target >= C:
                lines.append({"leg": "rigid_move", "sigma_threshold": thr, "error": "the sphere's centre cell is unlabelled"})
                continue
            trans = np.eye(4, dtype=np.float32)
            trans[:3, 3] = (0.4, 0.3, 0.0)
            margs = types.SimpleNamespace(N_samples=64, N_importance=128, near=S.NEAR, far=S.FAR, N_test=4096, target_labels=[target])
            rows = {k: [] for k in rows}
            for p in poses:
                torch.manual_seed(7)
                rgb, ins, _, _ = D.manipulate_frame(H, W, K, p.to(dev), [torch.from_numpy(trans)], (mc, mf), margs)
                score(Ed.render_preview(baked, H, W, K, p, [trans], [target], near=S.NEAR, far=S.FAR),
                      Ed.preview_frame(baked, H, W, K, p, [trans], [target], near=S.NEAR, far=S.FAR), rgb, ins)
            lines.append({"leg": "rigid_move", "sigma_threshold": thr, "target_label": target, "translation": trans[:3, 3].tolist(),
                          "views": len(poses), **{k: float(np.mean(v)) for k, v in rows.items()}, "per_view": dict(rows)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--no-frame", action="store_true", help="do not render the manipulation frame")
    ap.add_argument("--quality", action="store_true", help="train on the analytic scene and measure the proxies against rendered frames")
    ap.add_argument("--steps", type=int, default=3000, help="training steps of --quality")
    ap.add_argument("--sigma-threshold", type=float, nargs="+", default=[0.0, 5.0], help="bake_grid thresholds of --quality")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    lines = [T.device_line(iters=a.iters, warmup=a.warmup)]
    (quality if a.quality else timing)(a, lines)
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
