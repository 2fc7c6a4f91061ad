"""Time the field-edit render (``manipulate_frame(..., field_edit=edit)``) against the renders that exist, in one session.

    python scripts/time_field_edit.py [--out profiles/field_edit/timing_f32.jsonl]
    python scripts/time_field_edit.py --mfma-split f16x2 [--out profiles/field_edit/timing_f16x2.jsonl]

The configuration of scripts/time_manip_skip.py: one 640 x 480 frame, 64 + 128 samples, chunks of 4096 rays, ins_num 13, the
benchmark's models and camera.  The volume is synthetic: a 128^3 box round the scene whose cells carry a random label with probability
5, 25 and 100 % (``--fills``) and are unlabelled otherwise; ``unowned`` and ``outside`` are ``"empty"``, so the fill is the share of the
box the route evaluates.  The yardsticks, whose code this work leaves unchanged: ``render_frame`` (no edit) and ``manipulate_frame`` with
T = 1 and T = 3 rigid moves, dense and with ``skip=`` the bit grid of the same labelled cells.  The new route: E = 1, 3 and 32 edits
(moves, with a copy and a removal among them from E = 3 on) through ``FieldEdit.from_volume``; the ``edit_volume`` call is outside the
timed window (it is made once per edit, not per frame).  Per row: HIP-event milliseconds of the whole frame, median and minimum of
``--iters`` runs after ``--warmup``, rays/s, the network launches per chunk, and ``n_eval`` = (samples evaluated, samples).  The first
line records the device and its clocks as ``rocm-smi`` reports them (read-only).  One JSON object per line.

``--quality`` (the ANALYTIC scene only; no real scene is measured): the training loop of tests/test_gpu_convergence.py as
scripts/time_baked.py's ``--quality`` runs it (``--steps`` steps on the twelve 120 x 160 views of oracle/analytic_scene.py), ``SkipGrid.from_model`` and
``bake_grid`` over [-8, 8)^3 at 128^3 per ``--sigma-threshold`` value, then on three held-out poses, with both policies ``"evaluate"``
and with both ``"empty"``:

    no_edit      the field-edit frame of ``FieldEdit.from_volume(baked, [], [])`` against ``render_frame``: PSNR over all pixels and over
                 the pixels the dense frame gives to an object, and the share of pixels whose label (argmax over the object channels
                 both frames have) agrees; ``render_preview`` of the same volume scored the same way next to it
    rigid_move   one translation of the first sphere: the field-edit frame against ``manipulate_frame`` of the same move (the same
                 draws), PSNR as above and label agreement over all C channels; ``render_preview`` next to it

with the evaluated fraction of the field-edit frames.  The timing rows are not produced in this mode."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402


def quality(a, emit):
    import types
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    from oracle import analytic_scene as S
    dev = torch.device("cuda:0")
    H, W, C = 120, 160, 14
    t0 = time.perf_counter()
    LO, HI = T.BOX
    mc, mf = T.train_analytic(a.steps, dev)
    torch.cuda.synchronize()
    emit({"leg": "quality_setup", "scene": "analytic scene only: no real scene was measured", "train_steps": a.steps,
          "train_s": time.perf_counter() - t0, "frame": [H, W], "dims": a.dims, "box": [LO, HI]})
    K = S.dmsr_intrinsics(H, W)
    poses = [S.pose_spherical(th, -65.0, 7.0) for th in (17.0, 77.0, 197.0)]     # none of the twelve training views
    rargs = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    psnr = lambda x, y: float(-10.0 * torch.log10(((x.double() - y.double()) ** 2).mean()))
    as_label = lambda l: torch.where(l == 255, torch.full_like(l, C - 1), l).long()

    def field_frame(edit, pose, margs):
        torch.manual_seed(7)
        fr = D.ManipulationFrameRenderer(H, W, K, pose.to(dev), [], (mc, mf), margs, field_edit=edit)
        for c in range(fr.n_chunks):
            fr.step(c)
        rgb, ins, _, _ = fr.gather()
        n_eval = fr.n_eval.tolist()
        return rgb, ins, n_eval[0] / max(n_eval[1], 1)

    with torch.no_grad():
        occ = F.SkipGrid.from_model(mf, LO, HI, a.dims)
        dense = [D.render_frame(H, W, K, p.to(dev), (mc, mf), S.NEAR, S.FAR, rargs) for p in poses]
        for thr in a.sigma_threshold:
            baked = F.bake_grid(mf, occ, sigma_threshold=thr)
            common = {"sigma_threshold": thr, "occupancy": float(occ.occupancy()), "labelled_fraction": float((baked.labels != 255).float().mean()),
                      "views": len(poses)}
            margs = types.SimpleNamespace(N_samples=64, N_importance=128, near=S.NEAR, far=S.FAR, N_test=4096, target_labels=[])
            centre = np.asarray(S.SPHERES[0][0])
            i, j, k = [int(np.floor((centre[x] - LO[x]) / (HI[x] - LO[x]) * a.dims)) for x in range(3)]
            target = int(baked.labels[i, j, k])
            trans = np.eye(4, dtype=np.float32)
            trans[:3, 3] = (0.4, 0.3, 0.0)
            moved = None
            if target < C:
                mv = types.SimpleNamespace(N_samples=64, N_importance=128, near=S.NEAR, far=S.FAR, N_test=4096, target_labels=[target])
                moved = []
                for p in poses:
                    torch.manual_seed(7)
                    moved.append(D.manipulate_frame(H, W, K, p.to(dev), [torch.from_numpy(trans)], (mc, mf), mv)[:2])
            for policy in ("evaluate", "empty"):
                # ---- no edit, against render_frame (its object map has the C - 1 object channels: both labels are taken over those)
                edit = Ed.FieldEdit.from_volume(baked, [], [], outside=policy, unowned=policy)
                rows = {"psnr_all": [], "psnr_object_pixels": [], "label_agreement": [], "evaluated_fraction": [], "preview_psnr_all": [],
                        "preview_psnr_object_pixels": [], "preview_label_agreement": []}
                for p, (rgb, ins, _) in zip(poses, dense):
                    want = ins.argmax(-1)
                    obj = want < S.N_OBJECTS
                    f_rgb, f_ins, frac = field_frame(edit, p, margs)
                    soft = Ed.render_preview(baked, H, W, K, p, near=S.NEAR, far=S.FAR)
                    rows["psnr_all"].append(psnr(f_rgb, rgb))
                    rows["psnr_object_pixels"].append(psnr(f_rgb[obj], rgb[obj]))
                    rows["label_agreement"].append(float((f_ins[..., :C - 1].argmax(-1) == want).float().mean()))
                    rows["evaluated_fraction"].append(frac)
                    rows["preview_psnr_all"].append(psnr(soft["rgb"], rgb))
                    rows["preview_psnr_object_pixels"].append(psnr(soft["rgb"][obj], rgb[obj]))
                    rows["preview_label_agreement"].append(float((as_label(soft["label"]) == want).float().mean()))
                emit({"leg": "no_edit", "against": "render_frame", "policy": policy, **common, **{k: float(np.mean(v)) for k, v in rows.items()},
                      "per_view": rows})
                # ---- one rigid move of the first sphere, against manipulate_frame
                if moved is None:
                    emit({"leg": "rigid_move", "policy": policy, **common, "error": "the sphere's centre cell is unlabelled"})
                    continue
                edit = Ed.FieldEdit.from_volume(baked, [trans], [target], outside=policy, unowned=policy)
                rows = {k: [] for k in rows}
                for p, (rgb, ins) in zip(poses, moved):
                    want = ins.argmax(-1)
                    obj = want < S.N_OBJECTS
                    f_rgb, f_ins, frac = field_frame(edit, p, margs)
                    soft = Ed.render_preview(baked, H, W, K, p, [trans], [target], near=S.NEAR, far=S.FAR)
                    rows["psnr_all"].append(psnr(f_rgb, rgb))
                    rows["psnr_object_pixels"].append(psnr(f_rgb[obj], rgb[obj]))
                    rows["label_agreement"].append(float((f_ins.argmax(-1) == want).float().mean()))
                    rows["evaluated_fraction"].append(frac)
                    rows["preview_psnr_all"].append(psnr(soft["rgb"], rgb))
                    rows["preview_psnr_object_pixels"].append(psnr(soft["rgb"][obj], rgb[obj]))
                    rows["preview_label_agreement"].append(float((as_label(soft["label"]) == want).float().mean()))
                emit({"leg": "rigid_move", "against": "manipulate_frame", "policy": policy, "target_label": target,
                      "translation": trans[:3, 3].tolist(), "moved_cells": int(edit.volume["won"][1]), **common,
                      **{k: float(np.mean(v)) for k, v in rows.items()}, "per_view": rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--fills", type=int, nargs="+", default=[5, 25, 100], help="labelled cells, per cent")
    ap.add_argument("--edits", type=int, nargs="+", default=[1, 3, 32], help="E of the field-edit rows")
    ap.add_argument("--moves", type=int, nargs="+", default=[1, 3], help="T of the manipulate_frame rows")
    ap.add_argument("--mfma-split", default=None, choices=["f16x2"], help="render with args.mfma_split (default: the f32 kernels)")
    ap.add_argument("--quality", action="store_true", help="train on the analytic scene and compare the route's frames with rendered ones")
    ap.add_argument("--steps", type=int, default=3000, help="training steps of --quality")
    ap.add_argument("--sigma-threshold", type=float, nargs="+", default=[0.0, 5.0], help="bake_grid thresholds of --quality")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    import types
    import bench_common as C
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    ins_num = mf.ins_num
    NC = ins_num + 1
    H, W, K, pose = T.study_view()
    pose = pose.to(dev)
    base = dict(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=4096)
    if a.mfma_split:
        base["mfma_split"] = a.mfma_split
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def emit(row):                                                   # (a row is on disk as soon as it is measured)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    emit(T.device_line(iters=a.iters, warmup=a.warmup, dims=a.dims, mfma_split=a.mfma_split))
    if a.quality:
        return quality(a, emit)

    def row(leg, make, counts=False, **kw):
        t = T.time_events(T.render_chunks, a.iters, a.warmup, setup=make)
        r = dict(leg=leg, ms_median=t.median, ms_min=t.min, rays_per_s=H * W / t.median * 1e3, **kw)
        if counts:
            n_eval = t.last.n_eval.tolist()
            if n_eval[1]:
                r.update(n_eval=n_eval, evaluated_fraction=n_eval[0] / n_eval[1])
        emit(r)

    with torch.no_grad():
        plain = types.SimpleNamespace(perturb=False, is_train=False, N_ins=None, **base)

        def frame():
            return D.FrameRenderer(H, W, K, pose, (mc, mf), 4.0, 15.0, plain, chunk=4096, n_samples=64)
        row("render_frame", frame, launches_per_chunk=2)

        def manip(n, **kw):
            args = types.SimpleNamespace(target_labels=[2 + t for t in range(n)], **base)

            def make():
                torch.manual_seed(7)                                 # the same draws in every run and every row
                return D.ManipulationFrameRenderer(H, W, K, pose, [torch.tensor(T.rigid(t), dtype=torch.float32) for t in range(n)], (mc, mf),
                                                   args, chunk=4096, **kw)
            return make
        for n in a.moves:
            row("manipulate_frame_dense", manip(n), T=n, launches_per_chunk=2 + 4 * n)
        for pct in a.fills:
            labels = T.random_labels(pct, a.dims, NC - 1)
            grid = F.LabelGrid.from_labels(torch.from_numpy(labels).to(dev), *T.BOX, NC)
            fill = float((labels != 255).mean())
            skip = grid.skip_grid(range(NC), outside="empty")
            for n in a.moves:
                row("manipulate_frame_skip", manip(n, skip=skip), True, T=n, fill=fill, launches_per_chunk=2 + 4 * n)
            for E in a.edits:
                trans = [Ed.Remove() if (E >= 3 and e == 2) else Ed.Copy(T.rigid(e)) if (E >= 3 and e == 1) else T.rigid(e) for e in range(E)]
                targets = [e % (NC - 1) for e in range(E)]
                edit = Ed.FieldEdit.from_volume(grid, trans, targets, outside="empty", unowned="empty")
                args = types.SimpleNamespace(target_labels=[], **base)

                def make():
                    torch.manual_seed(7)
                    return D.ManipulationFrameRenderer(H, W, K, pose, [], (mc, mf), args, chunk=4096, field_edit=edit)
                row("field_edit", make, True, E=E, fill=fill, owned=float((edit.source != 255).float().mean()), launches_per_chunk=2)


if __name__ == "__main__":
    main()
