"""Time one full training step through the occupancy bit grid (``args.train_skip``) against the dense step, by grid occupancy, and
-- with ``--quality`` -- train the analytic scene dense and with ``field.TrainSkip`` and compare what they learn.

    python scripts/time_train_skip.py [--out profiles/train_skip/timing_f32.jsonl]
    python scripts/time_train_skip.py --mfma-split f16x2 [--out profiles/train_skip/timing_f16x2.jsonl]
    python scripts/time_train_skip.py --tree ../parent --label parent --dense-only [--mfma-split f16x2]    (another checkout's dense step)
    python scripts/time_train_skip.py --quality [--steps 3000] [--out profiles/train_skip/quality.jsonl]

Timing: one optimisation step (``distributed.sharded_train_step`` in a world of one: dm_nerf forward with saved activations, img2mse +
object-code loss + emptiness penalizer on both levels, backward, Adam) on one batch of 3072 and of 4096 rays, 64 + 128 samples,
ins_num 13, perturb 1, the benchmark's models and camera.  The grids are synthetic: a 128^3 box round the scene whose cells are set at
random with probability 5, 10, 25, 50 and 100 %, ``outside="empty"``, both levels through the grid.  Per row: HIP-event milliseconds
of the step, median and minimum of ``--iters`` steps after ``--warmup``, and the evaluated fraction per level from
``args.train_skip_counts``.  The ``dense`` row is the same step without ``args.train_skip``; with ``--tree`` the package is imported
from that checkout (its library must be built), which is how the parent commit's dense step is timed in the same session.  The first
line records the device and its clocks as ``rocm-smi`` reports them (read-only).

Quality: tests/test_gpu_convergence.py's loop on the analytic scene (12 views of 120 x 160 + one held out, 3072 rays per step, Adam
5e-4 with the reference's decay), twice with the same seeds: dense, and with a ``TrainSkip`` (its defaults; a 128^3 grid over the box
the rays can reach, ``outside="evaluate"``) at both levels.  Per run and checkpoint: held-out PSNR, label purity, evaluated fraction
per level since the last checkpoint, and wall seconds of the training steps (evaluations excluded).  One JSON object per line."""
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


def timing(a, lines):
    import bench_common as C
    from dm_nerf_amd import distributed as D, field as F
    from dm_nerf_amd.networks import helpers as H
    dev = torch.device("cuda")
    _, _, mc, mf = C.build_models(dev)
    mc.train(); mf.train()
    _, _, K, pose = T.study_view()
    ro, rd = H.get_rays_k(480, 640, K, pose.to(dev))
    pick = torch.from_numpy(np.random.RandomState(0).choice(480 * 640, 4096, replace=False)).to(dev)
    ro, rd = ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous()
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
    start = [p.detach().clone() for p in opt.param_groups[0]["params"]]
    for n in (3072, 4096):
        g = torch.Generator(device=dev).manual_seed(0)
        target, labels = torch.rand(n, 3, device=dev, generator=g), torch.randint(0, 9, (n,), device=dev, generator=g)
        rays = torch.stack([ro[:n], rd[:n]])
        z = H.z_val_sample(n, 4.0, 15.0, 64, device=dev)
        dense_ms = None
        for pct in (None,) + (() if a.dense_only else (5, 10, 25, 50, 100)):
            args = types.SimpleNamespace(perturb=1.0, N_importance=128, is_train=True, N_ins=None, penalize=True, tolerance=0.05, deta_w=0.05,
                                         mfma_split=a.mfma_split or False)
            if pct is not None:
                args.train_skip = F.SkipGrid.from_bits(T.random_bits(pct, a.dims), *T.BOX, a.dims, outside="empty")
                args.train_skip_levels = ("coarse", "fine")
                args.train_skip_counts = {l: torch.zeros(2, dtype=torch.int64, device=dev) for l in ("coarse", "fine")}
            with torch.no_grad():                                    # every row starts from the same weights and optimizer state
                for p, s in zip(opt.param_groups[0]["params"], start):
                    p.copy_(s)
            opt.state.clear()
            torch.manual_seed(0); torch.cuda.manual_seed(0)
            t = T.time_events(lambda: D.sharded_train_step(rays, z, target, labels, (mc, mf), args, opt, C.INS_NUM), a.iters, a.warmup)
            med, mn = t.median, t.min
            row = {"leg": "dense" if pct is None else "skip", "rays": n, "ms_median": med, "ms_min": mn}
            if pct is None:
                dense_ms = med
            else:
                cnt = {l: t.tolist() for l, t in args.train_skip_counts.items()}
                row.update(grid_occupancy=float(args.train_skip.occupancy()), speedup_vs_dense=dense_ms / med,
                           evaluated_fraction={l: c[0] / max(c[1], 1) for l, c in cnt.items()},
                           evaluated_fraction_all=sum(c[0] for c in cnt.values()) / max(sum(c[1] for c in cnt.values()), 1))
                if pct == 100:
                    row["overhead_over_dense_ms"] = med - dense_ms
            lines.append(row)
            print(json.dumps(row), flush=True)


def quality(a, lines):
    from dm_nerf_amd import config as Cfg, field as F
    from dm_nerf_amd.networks import evaluator as E, helpers as Hh, penalizer as P, render as R
    from oracle import analytic_scene as S
    dev = torch.device("cuda:0")
    ins_num, H, W, views, batch = 13, 120, 160, 12, 3072
    thetas = list(np.linspace(0.0, 360.0, views, endpoint=False)) + [17.0]          # the last view is held out
    poses, ims, labs = S.make_views(H, W, thetas, ins_num)
    K = S.dmsr_intrinsics(H, W)
    tro, trd = Hh.get_rays_k(H, W, K, poses[-1, :3, :4])
    test_rays = torch.stack([tro.reshape(-1, 3), trd.reshape(-1, 3)])
    d_ims, d_labs = ims.to(dev), labs.to(dev)
    z = Hh.z_val_sample(batch, S.NEAR, S.FAR, 64, device=dev)
    ze = Hh.z_val_sample(H * W, S.NEAR, S.FAR, 64, device=dev)
    checkpoints = sorted(set(int(c) for c in a.checkpoints.split(",")))

    def evaluate(mc, mf):
        eargs = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, mfma_split=a.mfma_split or False)
        mc.eval(); mf.eval()
        with torch.no_grad():
            out = R.dm_nerf(test_rays, None, None, mc, mf, ze, eargs)
        mc.train(); mf.train()
        pred = out['ins_fine'].cpu().argmax(-1)
        return S.psnr(out['rgb_fine'].cpu(), ims[-1].reshape(-1, 3)), S.purity(pred, labs[-1].reshape(-1))

    for leg in ("dense", "train_skip"):
        torch.manual_seed(0)
        cargs = types.SimpleNamespace(multires=10, multires_views=4, i_embed=0, netdepth=8, netwidth=256, ins_num=ins_num, device=dev)
        _, _, mc, mf, _ = Cfg.create_nerf(cargs)
        mc.train(); mf.train()
        opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
        args = types.SimpleNamespace(perturb=1.0, N_importance=128, is_train=True, N_ins=None, penalize=True, tolerance=0.05, deta_w=0.05,
                                     mfma_split=a.mfma_split or False)
        ts = None
        if leg == "train_skip":
            ts = F.TrainSkip((-12.0,) * 3, (12.0,) * 3, dims=a.dims)              # the defaults under test
            args.train_skip = ts
            args.train_skip_counts = {l: torch.zeros(2, dtype=torch.int64, device=dev) for l in ("coarse", "fine")}
        np.random.seed(0)
        torch.cuda.manual_seed(0)
        psnr0, pur0 = evaluate(mc, mf)
        wall = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(1, a.steps + 1):
            v = np.random.choice(views)
            tc, ti, rays = Hh.get_select_full(d_ims[v], poses[v, :3, :4], K, d_labs[v], batch)
            out = R.dm_nerf(rays, None, None, mc, mf, z, args)
            loss = E.img2mse(out['rgb_fine'], tc) + E.img2mse(out['rgb_coarse'], tc) + E.ins_criterion(out['ins_fine'], ti, ins_num)[0] \
                + E.ins_criterion(out['ins_coarse'], ti, ins_num)[0] \
                + P.ins_penalizer(out['raw_fine'], out['z_vals_fine'], out['depth_fine'], rays[1], args).sum() \
                + P.ins_penalizer(out['raw_coarse'], out['z_vals_coarse'], out['depth_coarse'], rays[1], args).sum()
            opt.zero_grad(); loss.backward(); opt.step()
            for grp in opt.param_groups:
                grp['lr'] = 5e-4 * (0.1 ** (it / 500000.0))
            if ts is not None:
                ts.step(mf)
            if it in checkpoints:
                torch.cuda.synchronize()
                wall += time.perf_counter() - t0
                psnr, pur = evaluate(mc, mf)
                row = {"leg": "quality", "run": leg, "step": it, "psnr_db": psnr, "purity": pur, "psnr_db_untrained": psnr0,
                       "train_wall_s": wall}
                if ts is not None:
                    cnt = {l: t.tolist() for l, t in args.train_skip_counts.items()}
                    row.update(evaluated_fraction_since_last={l: c[0] / max(c[1], 1) for l, c in cnt.items()}, refreshes=ts.refreshes,
                               grid_occupancy=float(ts.grid.occupancy()),
                               train_skip={"every": ts.every, "warmup": ts.warmup, "threshold": ts.threshold, "dilate": ts.dilate,
                                           "dims": a.dims, "outside": ts.grid.outside})
                    for t in args.train_skip_counts.values():
                        t.zero_()
                lines.append(row)
                print(json.dumps(row), flush=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--mfma-split", default=None, choices=["f16x2"], help="train with args.mfma_split (default: the f32 kernels)")
    ap.add_argument("--tree", default=None, help="import the package from this checkout (default: the one this script lies in)")
    ap.add_argument("--label", default=None, help="what to record as the tree instead of its path")
    ap.add_argument("--dense-only", action="store_true", help="time the dense step only (a checkout without args.train_skip)")
    ap.add_argument("--quality", action="store_true", help="the quality leg instead of the timing")
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--checkpoints", default="1000,2000,3000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    tree = os.path.abspath(a.tree) if a.tree else T.ROOT
    sys.path.insert(0, tree)
    import dm_nerf_amd
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, tree=a.label or os.path.relpath(tree),
                           package_in_tree=os.path.relpath(os.path.dirname(os.path.abspath(dm_nerf_amd.__file__)), tree))]
    if a.mfma_split:
        lines[0]["mfma_split"] = a.mfma_split
    print(json.dumps(lines[0]), flush=True)
    (quality if a.quality else timing)(a, lines)
    T.write_jsonl(lines, a.out, echo=False)                          # (every line was printed as it was measured)


if __name__ == "__main__":
    main()
