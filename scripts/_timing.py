"""What the stand-alone timing scripts (scripts/time_*.py) share: the one event timer, the host-clock timer, the device line, the
output tail and the seeded fixtures.  A script's preamble is

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _timing as T

(importing this module puts the repository root on ``sys.path``), and its ``main()`` parses its arguments, calls
``T.require_gpu(__file__)`` and then reads top to bottom.  No script imports another script."""
import collections
import json
import os
import subprocess
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640                                                      # the study frame
BOX = ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))                          # (lo, hi) of the box round the scene
UNLABELLED = 255                                                     # field.UNLABELLED (the package may come from another checkout)

Timing = collections.namedtuple("Timing", "median min max runs last")


def require_gpu(name):
    """A measurement path that finds no GPU fails; it does not fall back."""
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(name)} measures on the GPU: no device found")


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30)
        return json.loads(r.stdout) if r.returncode == 0 else {"error": r.stderr[-200:]}
    except Exception as e:                                           # the tool is optional
        return {"error": repr(e)}


def device_line(**extra):
    """The first JSON line: the device, its clocks as ``rocm-smi --showclocks`` reports them (read-only), and what the script adds."""
    return {"leg": "device", "name": torch.cuda.get_device_name(0), "clocks": clocks(), **extra}


def reduce_ms(runs):
    """A list of milliseconds -> (median, min, max); the median of an even count is the mean of the two middle runs."""
    return float(np.median(runs)), float(np.min(runs)), float(np.max(runs))


def time_events(fn, iters, warmup, setup=None):
    """HIP events round ``fn()``, or round ``fn(setup())`` with ``setup()`` outside the timed window; ``warmup`` untimed iterations
    that run what the timed ones run, a device synchronise after every one.  -> Timing (milliseconds; ``last``: the last ``setup()``)."""
    runs, last = [], None
    for it in range(warmup + iters):
        if setup is not None:
            last = setup()
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        fn() if setup is None else fn(last)
        e.record()
        torch.cuda.synchronize()
        if it >= warmup:
            runs.append(b.elapsed_time(e))
    return Timing(*reduce_ms(runs), runs, last)


def time_host(fn, iters, warmup):
    """A host clock between two device synchronises, for calls whose host work is part of the cost.  -> Timing (milliseconds)."""
    runs = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            runs.append((time.perf_counter() - t0) * 1e3)
    return Timing(*reduce_ms(runs), runs, None)


def render_chunks(fr):
    """Every chunk of a frame renderer: what a frame leg times, with the renderer made by ``setup=``."""
    for i in range(fr.n_chunks):
        fr.step(i)


def write_jsonl(lines, out, echo=True):
    """Print the lines (unless the script printed each as it was measured) and write them to ``out``, creating its directory."""
    text = "\n".join(json.dumps(l) for l in lines)
    if echo:
        print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


# ---- fixtures: every one is seeded, and the same in every script that uses it

def study_view():
    """-> H, W, K, pose of the 640 x 480 study view (the benchmark's camera); the pose is a host tensor."""
    from oracle import ref_cpu as O                                  # (here: a script may have put another checkout first on the path)
    return H, W, O.dmsr_intrinsics(H, W), O.pose_spherical(30.0, -65.0, 7.0)


def pack_bits(cells):
    """A bool array -> the uint32 words of a SkipGrid: cell g is bit g & 31 of word g >> 5."""
    words = np.packbits(cells.reshape(-1), bitorder="little")
    return np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)


def random_bits(pct, dims, seed=None):
    """The words of a dims^3 grid whose cells are set at random with probability ``pct`` per cent (seed: ``pct``)."""
    return pack_bits(np.random.RandomState(pct if seed is None else seed).rand(dims, dims, dims) < pct / 100.0)


def random_labels(pct, dims, C, seed=None):
    """A dims^3 uint8 volume: a label uniform in 0 .. C - 1 with probability ``pct`` per cent, UNLABELLED otherwise (seed: ``pct``)."""
    rng = np.random.RandomState(pct if seed is None else seed)
    vol = rng.randint(0, C, size=(dims,) * 3).astype(np.uint8)
    vol[rng.rand(dims, dims, dims) >= pct / 100.0] = UNLABELLED
    return vol


def random_baked(pct, dims, C):
    """-> (set cells, labels, cells) of a dims^3 baked volume with ``pct`` per cent of the cells set: label uniform in 0 .. C - 1,
    colour logits N(0, 1), density uniform in 0 .. 8; an unset cell is UNLABELLED and zero."""
    rng = np.random.RandomState(pct)
    shape = (dims,) * 3
    set_cells = rng.rand(*shape) < pct / 100.0
    vol = rng.randint(0, C, size=shape).astype(np.uint8)
    vol[~set_cells] = UNLABELLED
    cells = np.zeros(shape + (4,), np.float32)
    cells[..., :3] = rng.randn(*shape, 3)
    cells[..., 3] = rng.uniform(0.0, 8.0, size=shape)
    cells[~set_cells] = 0.0
    return set_cells, vol, cells


def voronoi_labels(dims, n_labels, C, stray_pct=3.0, seed=0):
    """A dims^3 uint8 volume that looks like objects with strays: the Voronoi partition of ``n_labels`` random seed points (label = the
    nearest seed, the lowest on ties; squared distances in int64), then ``stray_pct`` per cent of the cells relabelled uniformly in
    0 .. C - 1 (label C - 1 is "empty": it exists only as strays)."""
    rng = np.random.RandomState(seed)
    points = rng.randint(0, dims, size=(n_labels, 3)).astype(np.int64)
    ax = np.arange(dims, dtype=np.int64)
    vol = np.empty((dims,) * 3, np.uint8)
    for i in range(dims):                                            # plane by plane: [n_labels, dims, dims] int64 at a time
        d2 = (i - points[:, 0, None, None]) ** 2 + (ax[None, :, None] - points[:, 1, None, None]) ** 2 \
            + (ax[None, None, :] - points[:, 2, None, None]) ** 2
        vol[i] = np.argmin(d2, axis=0)
    stray = rng.rand(dims, dims, dims) < stray_pct / 100.0
    vol[stray] = rng.randint(0, C, size=int(stray.sum())).astype(np.uint8)
    return vol


def rigid(e=0, series="frame"):
    """The e-th rigid test move, a rotation about z and a shift, as a 4 x 4 float64 array.  ``rigid()`` is THE move of the frame
    scripts (0.2 rad, shift 0.3 / -0.2 / 0.1); series "frame" goes on with moves of the same size, alternating the shift's side;
    series "volume" starts at 0.1 rad and grows the angle and the shift with e."""
    if series == "volume":
        ang, shift = 0.1 + 0.02 * e, (0.3 + 0.05 * e, -0.2, 0.1 * (e % 5))
    else:
        s = 1.0 if e % 2 == 0 else -1.0
        ang, shift = 0.2 + 0.05 * e, (0.3 * s, -0.2 + 0.02 * e, 0.1 * s)
    return np.array([[np.cos(ang), -np.sin(ang), 0., shift[0]], [np.sin(ang), np.cos(ang), 0., shift[1]], [0., 0., 1., shift[2]],
                     [0., 0., 0., 1.]], dtype=np.float64)


def train_analytic(steps, dev):
    """tests/test_gpu_convergence.py's loop (the reference's recipe) on the analytic scene -> the two trained networks: the field
    of the ``--quality`` legs."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_convergence as TC
    from dm_nerf_amd import config as Cfg
    from dm_nerf_amd.networks import evaluator as E, helpers as Hh, penalizer as P, render as R
    from oracle import analytic_scene as S
    h, w, views, batch = 120, 160, 12, 3072
    poses, ims, labs, K, _ = TC._setup(h, w, views, dev)
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
