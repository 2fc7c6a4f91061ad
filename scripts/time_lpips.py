"""Time LPIPS (VGG16) on the device: ``evaluator.LPIPSVGG`` (csrc/conv3x3.hip, csrc/lpips.hip), the third image score of
``render_test`` (networks/tester.py:43,91), with random weights (tests/_lpips_restate.py's generator).

    python scripts/time_lpips.py                              # 480 x 640: HIP-event ms, median of --iters after --warmup
    python scripts/time_lpips.py --no-torch                   # without the yardstick

One JSON line per measurement:
  pair       one 480 x 640 frame pair (P = 1), the whole metric; ``fraction_of_f32_mfma_peak`` = 375.8 GFLOP (2 frames x 93.95 GMAC of
             the thirteen convolutions) over the median time, against the 157.3 TFLOP/s f32 MFMA peak
  batch      P = 10 in one call, likewise
  step       every launch of a P = 1 call on its own (prologue, each convolution with its GFLOP and fraction of the peak, each pool,
             each tail); conv5_x has 2 x 1200 pixel rows and cannot fill 256 CUs at P = 1
  torch      the same network through ``torch.nn.functional.conv2d`` / ``max_pool2d`` on the device with the same weights -- what a
             caller has to do today.  A yardstick only: no part of the package, and not a target set in advance.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

sys.path.insert(0, os.path.join(T.ROOT, "tests"))

PEAK_F32_MFMA_TFLOPS = 157.3


def conv_gflop(P, H, W):
    """2 x MACs of the thirteen convolutions on 2P frames, per layer (the K = 27 of the first layer, not its padded 32)."""
    import _lpips_restate as RS
    out, h, w = [], H, W
    for i, (idx, sl, cin, cout) in enumerate(RS.CONVS):
        if i > 0 and RS.CONVS[i - 1][1] != sl:
            h, w = h // 2, w // 2
        out.append(2.0 * 2 * P * h * w * 9 * cin * cout / 1e9)
    return out


def steps_of(model, pred, gt):
    """The launches of ``model(pred, gt)`` one by one (the sequence of LPIPSVGG.__call__), as (name, closure) pairs."""
    import torch
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator as E
    lib = _lib.load()
    P, H, W, _ = pred.shape
    ws = model._workspace(P, H, W)
    out = torch.empty(P, dtype=torch.float64, device=pred.device)
    st, N = _lib.stream(), 2 * P
    steps = [("prologue", lambda: _lib.check(lib.dmnerf_lpips_prologue(_lib.ptr(pred), _lib.ptr(gt), P, H, W, 0, _lib.ptr(ws["taps"]),
                                                                       ws["taps"].numel(), st), "prologue"))]
    src, dst, other = ws["taps"], ws["a"], ws["b"]
    h, w, level = H, W, 0
    for i, (idx, sl, cin, cout) in enumerate(E.LPIPS_VGG_CONVS):
        if i > 0 and sl != E.LPIPS_VGG_CONVS[i - 1][1]:
            steps.append((f"pool{sl - 1}", lambda s=src, d=dst, h=h, w=w, c=cin: _lib.check(
                lib.dmnerf_maxpool2(_lib.ptr(s), s.numel(), _lib.ptr(d), d.numel(), N, h, w, c, st), "maxpool2")))
            h, w = h // 2, w // 2
            src, dst = dst, src
        first = i == 0
        steps.append((f"conv{idx}", lambda s=src, d=dst, i=i, h=h, w=w, cin=32 if first else cin, cout=cout, t=1 if first else 9: _lib.check(
            lib.dmnerf_conv3x3(_lib.ptr(s), s.numel(), _lib.ptr(model.packed[i]), model.packed[i].numel(), _lib.ptr(model.bias[i]), _lib.ptr(d),
                               d.numel(), N, h, w, cin, cout, t, 1, st), "conv3x3")))
        src, dst = (dst, other) if first else (dst, src)
        if i + 1 == len(E.LPIPS_VGG_CONVS) or E.LPIPS_VGG_CONVS[i + 1][1] != sl:
            steps.append((f"tail{level}", lambda s=src, h=h, w=w, c=cout, l=level: _lib.check(
                lib.dmnerf_lpips_tail(_lib.ptr(s), s.numel(), _lib.ptr(model.lin[l]), P, h, w, c, 1 if l == 0 else 0, _lib.ptr(ws["part"]),
                                      ws["part"].numel(), _lib.ptr(out), st), "lpips_tail")))
            level += 1
    return steps, out


def torch_lpips(pred, gt, sd):
    import torch
    import torch.nn.functional as F
    import _lpips_restate as RS
    P = pred.shape[0]
    x = torch.cat([pred, gt], 0).permute(0, 3, 1, 2)
    x = (x - torch.tensor(RS.SHIFT, device=x.device).view(1, 3, 1, 1)) / torch.tensor(RS.SCALE, device=x.device).view(1, 3, 1, 1)
    score = torch.zeros(P, dtype=torch.float64, device=x.device)
    k = 0
    for i, (idx, sl, cin, cout) in enumerate(RS.CONVS):
        if i > 0 and RS.CONVS[i - 1][1] != sl:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, sd[f"net.slice{sl}.{idx}.weight"], sd[f"net.slice{sl}.{idx}.bias"], padding=1))
        if i + 1 == len(RS.CONVS) or RS.CONVS[i + 1][1] != sl:
            f0, f1 = x[:P], x[P:]
            n0, n1 = torch.sqrt((f0 ** 2).sum(1, keepdim=True)), torch.sqrt((f1 ** 2).sum(1, keepdim=True))
            d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
            score = score + (d * sd[f"lin{k}.model.1.weight"]).sum(1).double().mean((1, 2))
            k += 1
    return score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    T.require_gpu(__file__)
    if a.iters < 10:
        print("note: fewer than 10 timed runs", file=sys.stderr)

    import torch
    import _lpips_restate as RS
    from dm_nerf_amd.networks import evaluator as E

    H, W = a.height, a.width
    sd = {k: v.cuda() for k, v in RS.random_state_dict(0).items()}
    model = E.LPIPSVGG.from_state_dict(sd)
    base = {"H": H, "W": W, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    frames = {P: tuple(t.cuda() for t in RS.frames(P, H, W, 100 + P)) for P in (1, a.batch)}

    for name, P in (("pair", 1), ("batch", a.batch)):
        pred, gt = frames[P]
        med, mn = T.time_events(lambda: model(pred, gt), a.iters, a.warmup)[:2]
        gf = sum(conv_gflop(P, H, W))
        print(json.dumps({"stage": name, "P": P, **base, "ms_median": med, "ms_min": mn, "ms_per_pair": med / P, "conv_gflop": gf,
                          "achieved_tflops": gf / med, "fraction_of_f32_mfma_peak": gf / med / PEAK_F32_MFMA_TFLOPS,
                          "score": [float(v) for v in model(pred, gt)[:2]]}), flush=True)

    pred, gt = frames[1]
    steps, _ = steps_of(model, pred, gt)
    gfs = iter(conv_gflop(1, H, W))
    for step, fn in steps:                              # (in order: each step reads what the one before it left)
        med, mn = T.time_events(fn, a.iters, a.warmup)[:2]
        rec = {"stage": "step", "step": step, "P": 1, **base, "ms_median": med, "ms_min": mn}
        if step.startswith("conv"):
            gf = next(gfs)
            rec.update(conv_gflop=gf, achieved_tflops=gf / med, fraction_of_f32_mfma_peak=gf / med / PEAK_F32_MFMA_TFLOPS)
        print(json.dumps(rec), flush=True)

    if not a.no_torch:
        for name, P in (("torch_pair", 1), ("torch_batch", a.batch)):
            pred, gt = frames[P]
            with torch.no_grad():
                med, mn = T.time_events(lambda: torch_lpips(pred, gt, sd), a.iters, a.warmup)[:2]
                s = torch_lpips(pred, gt, sd)
            print(json.dumps({"stage": name, "P": P, **base, "ms_median": med, "ms_min": mn, "ms_per_pair": med / P,
                              "score": [float(v) for v in s[:2]]}), flush=True)


if __name__ == "__main__":
    main()
