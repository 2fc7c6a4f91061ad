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

``--quality`` (analytic scene only): the training loop of tests/test_gpu_convergence.py (``--steps`` steps of 3072 rays on the
twelve 120 x 160 views of oracle/analytic_scene.py), then ``SkipGrid.from_model`` and ``bake_grid`` over [-8, 8)^3 at 128^3, per
``--sigma-threshold`` value.  On held-out poses: PSNR of ``render_preview``'s ``rgb`` against the dense ``render_frame`` (all pixels,
and the pixels the dense frame gives to an object), and the share of pixels whose label agrees with the dense argmax for
``render_preview`` and for ``preview_frame`` (a pixel without a label counts as the field's "nothing" class).  The same three
numbers for one rigid move of one sphere against ``manipulate_frame``.  One JSON object per line."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_label_trace import time_host  # noqa: E402
from time_manip_skip import clocks, time_frame  # noqa: E402
from time_mark import time_call  # noqa: E402

LO, HI = (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)


def pack_bits(occ):
    words = np.packbits(occ.reshape(-1), bitorder="little")
    return np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)


def timing(a, lines):
    import bench_common as B
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    from oracle import ref_cpu as O
    dev = torch.device("cuda")
    H, W, C, target = 480, 640, 14, 2
    near, far = 4.0, 15.0
    K = O.dmsr_intrinsics(H, W)
    pose = O.pose_spherical(30.0, -65.0, 7.0)
    ang = 0.2
    trans = torch.tensor([[np.cos(ang), -np.sin(ang), 0., 0.3], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]],
                         dtype=torch.float32)
    lines[0].update({"batch": a.batch, "dims": a.dims, "frame": [H, W], "near": near, "far": far, "ins_num": C - 1})
    _, _, mc, mf = B.build_models(dev)
    fr = D.ManipulationFrameRenderer(H, W, K, pose, [trans], None, types.SimpleNamespace(N_importance=0, target_labels=[target]),
                                     ins_num=C - 1, rank=0, world=1)
    rays = {1: fr.ori[None].contiguous(), 2: torch.cat([fr.ori[None], fr.tar], 0)}
    sets = {1: [range(C)], 2: [[l for l in range(C) if l != target], [target]]}
    edits = {1: ((), ()), 2: ([trans], [target])}
    for pct in (0, 5, 25, 100):
        rng = np.random.RandomState(pct)
        shape = (a.dims,) * 3
        set_cells = rng.rand(*shape) < pct / 100.0
        occ = F.SkipGrid.from_bits(pack_bits(set_cells), LO, HI, a.dims)
        with torch.no_grad():
            for split in (None, "f16x2"):
                med, mn = time_call(lambda: F.bake_grid(mf, occ, split=split), a.iters, a.warmup)
                lines.append({"leg": "bake_grid", "set_fraction": float(set_cells.mean()), "split": split or "f32", "bake_ms_median": med,
                              "bake_ms_min": mn})
        vol = rng.randint(0, C, size=shape).astype(np.uint8)
        vol[~set_cells] = F.UNLABELLED
        cells = np.zeros(shape + (4,), np.float32)
        cells[..., :3] = rng.randn(*shape, 3)
        cells[..., 3] = rng.uniform(0.0, 8.0, size=shape)
        cells[~set_cells] = 0.0
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

                med, mn = time_call(batch, a.iters, a.warmup)
                row[name + "_render_ms_median"], row[name + "_render_ms_min"] = med / a.batch, mn / a.batch
                row[name + "_preview_ms_median"], row[name + "_preview_ms_min"] = time_host(
                    lambda: Ed.render_preview(bg, H, W, K, pose, *edits[R], near=near, far=far, stop=stop), a.iters, a.warmup)
            row["hard_preview_ms_median"], row["hard_preview_ms_min"] = time_host(
                lambda: Ed.preview_frame(bg, H, W, K, pose, *edits[R], near=near, far=far), a.iters, a.warmup)
            lines.append(row)
    if not a.no_frame:
        args = types.SimpleNamespace(N_samples=64, N_importance=128, near=near, far=far, N_test=4096, target_labels=[target])

        def renderer():
            torch.manual_seed(7)
            return D.ManipulationFrameRenderer(H, W, K, pose.to(dev), [trans], (mc, mf), args, chunk=4096)

        with torch.no_grad():
            med, mn, _ = time_frame(renderer, 1, 1)
        lines.append({"leg": "manipulate_frame_dense", "runs": 1, "warmup": 1, "ms": med})


def train_analytic(steps, dev):
    """tests/test_gpu_convergence.py's loop (the reference's recipe) on the analytic scene -> the two trained networks."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_convergence as TC
    from dm_nerf_amd import config as Cfg
    from dm_nerf_amd.networks import evaluator as E, helpers as Hh, penalizer as P, render as R
    from oracle import analytic_scene as S
    H, W, views, batch = 120, 160, 12, 3072
    poses, ims, labs, K, _ = TC._setup(H, W, views, dev)
    d_ims, d_labs = ims.to(dev), labs.to(dev)
    torch.manual_seed(0)
    cargs = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, ins_num=TC.INS_NUM, device=dev)
    _, _, mc, mf, _ = Cfg.create_nerf(cargs)
    mc.train(); mf.train()
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
    args = types.SimpleNamespace(perturb=1.0, N_importance=128, is_train=True, N_ins=None, penalize=True, tolerance=0.05, deta_w=0.05,
                                 mfma_split=False)
    z = Hh.z_val_sample(batch, S.NEAR, S.FAR, 64, device=dev)
    np.random.seed(0)
    torch.cuda.manual_seed(0)
    for it in range(1, steps + 1):
        v = np.random.choice(views)
        tc, ti, rays = Hh.get_select_full(d_ims[v], poses[v, :3, :4], K, d_labs[v], batch)
        out = R.dm_nerf(rays, None, None, mc, mf, z, args)
        loss = E.img2mse(out['rgb_fine'], tc) + E.img2mse(out['rgb_coarse'], tc) + E.ins_criterion(out['ins_fine'], ti, TC.INS_NUM)[0] \
            + E.ins_criterion(out['ins_coarse'], ti, TC.INS_NUM)[0] \
            + P.ins_penalizer(out['raw_fine'], out['z_vals_fine'], out['depth_fine'], rays[1], args).sum() \
            + P.ins_penalizer(out['raw_coarse'], out['z_vals_coarse'], out['depth_coarse'], rays[1], args).sum()
        opt.zero_grad(); loss.backward(); opt.step()
        for g in opt.param_groups:
            g['lr'] = 5e-4 * (0.1 ** (it / 500000.0))
    mc.eval(); mf.eval()
    return mc, mf


def quality(a, lines):
    from dm_nerf_amd import distributed as D, editing as Ed, field as F
    from oracle import analytic_scene as S
    dev = torch.device("cuda:0")
    H, W, C = 120, 160, 14
    t0 = time.perf_counter()
    mc, mf = train_analytic(a.steps, dev)
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
    if not torch.cuda.is_available():
        raise SystemExit("time_baked.py measures on the GPU: no device found")
    lines = [{"leg": "device", "name": torch.cuda.get_device_name(0), "clocks": clocks(), "iters": a.iters, "warmup": a.warmup}]
    (quality if a.quality else timing)(a, lines)
    text = "\n".join(json.dumps(l) for l in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
