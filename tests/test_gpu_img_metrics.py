"""SSIM and PSNR of rendered frames on the device (csrc/img_metrics.hip, ``evaluator.img_metrics_device`` / ``ssim`` / ``psnr``,
``render_path(image_metrics=True)``) against the numpy float64 restatement of the reference's two ``skimage.metrics`` calls
(tests/_img_metrics_restate.py, form (a): ``uniform_filter`` + crop; checked on the CPU by tests/test_img_metrics_restate.py).

The bound is |delta SSIM| <= 1e-9 and |delta PSNR| <= 1e-9 dB, derived and not measured: every moment is a sum of 49 float64 terms
of magnitude <= 1, so its absolute error is <= 49 x 2^-53 = 5.4e-15 in any order; the denominators are >= C1 = 1e-4 and >= C2 =
9e-4, so a window's S moves by ~2e-10 at most and the mean by no more; 1e-9 is 5 times that, and 100 times below the smallest
wrong-arithmetic effect the CPU test demonstrates (float32 moments, a counted border: > 1e-7).

Inputs come from oracle/analytic_scene.py and seeded numpy.  Observed on an MI355X: see DESIGN.md section 2."""
import types

import numpy as np
import pytest
import torch

import _gpu
import _img_metrics_restate as RS

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator
    _lib.load()
    return evaluator


@pytest.fixture(scope="module")
def main_cases():
    return RS.main_cases()


def _check_pair(E, name, pred, gt, seen):
    """One frame pair through the private driver (per-channel output included) against restatement (a)."""
    s, p, mse, ch = E._img_metrics_run(torch.from_numpy(pred).cuda()[None], torch.from_numpy(gt).cuda()[None], with_channels=True)
    s, p, mse, ch = float(s[0]), float(p[0]), float(mse[0]), ch[0].cpu().numpy()
    want_ch = RS.ssim_channels_uniform(pred, gt)
    want_s, want_p = RS.ssim_uniform(pred, gt), RS.psnr_restate(pred, gt)
    d_s, d_ch = abs(s - want_s), float(np.abs(ch - want_ch).max())
    d_p = 0.0 if (np.isinf(want_p) and p == want_p) else abs(p - want_p)
    print(f"{name}: ssim {s:.15f} (delta {d_s:.2e}, per channel {d_ch:.2e}), psnr {p:.12f} dB (delta {d_p:.2e})")
    seen["ssim"], seen["psnr"] = max(seen["ssim"], d_s, d_ch), max(seen["psnr"], d_p)
    assert d_s <= TOL and d_ch <= TOL, (name, s, want_s, ch, want_ch)
    assert d_p <= TOL, (name, p, want_p)
    assert abs(mse - RS.mse_restate(pred, gt)) <= 1e-15, (name, mse)
    assert s == RS.channel_mean(ch), name                # the frame's SSIM is the mean of the per-channel output, bit for bit


def test_against_the_restatement(E, main_cases):
    seen = {"ssim": 0.0, "psnr": 0.0}
    for name, (pred, gt) in main_cases.items():
        _check_pair(E, name, pred, gt, seen)
    for shape, (pred, gt) in RS.shape_cases().items():
        _check_pair(E, str(shape), pred, gt, seen)
    print(f"max |delta SSIM| {seen['ssim']:.3e}, max |delta PSNR| {seen['psnr']:.3e} dB (bound {TOL:.0e})")
    pred, gt = main_cases["same"]
    s, p = E.img_metrics_device(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
    assert s.dim() == 0 and s.dtype == torch.float64 and p.dtype == torch.float64
    assert float(s) == 1.0 and float(p) == float("inf")
    a, b = (torch.from_numpy(x).cuda() for x in main_cases["noise"])
    assert abs(E.ssim(a, b) - RS.ssim_uniform(*main_cases["noise"])) <= TOL
    assert abs(E.psnr(a, b) - RS.psnr_restate(*main_cases["noise"])) <= TOL
    assert isinstance(E.ssim(a, b), float) and isinstance(E.psnr(a, b), float)


def _batch(main_cases, P):
    names = ("noise", "shift", "const", "same", "noise")[:P]
    pred = torch.from_numpy(np.stack([main_cases[n][0] for n in names])).cuda()
    gt = torch.from_numpy(np.stack([main_cases[n][1] for n in names])).cuda()
    if P == 5:
        pred[4] = pred[4].flip(0)                        # a fifth pair unlike the first
    return names, pred, gt


def test_batches_of_1_3_5_frames(E, main_cases):
    alone = {}
    for P in (1, 3, 5):
        names, pred, gt = _batch(main_cases, P)
        s, p = E.img_metrics_device(pred, gt)
        s2, p2 = E.img_metrics_device(pred, gt)
        assert s.shape == (P,) and p.shape == (P,) and s.dtype == torch.float64
        assert torch.equal(s, s2) and torch.equal(p, p2)                     # no atomics: the same bits every run
        for i in range(P):
            si, pi = E.img_metrics_device(pred[i], gt[i])
            assert torch.equal(si, s[i]) and torch.equal(pi, p[i]), (P, i)   # a frame's score does not depend on the batch
            want_s = RS.ssim_uniform(pred[i].cpu().numpy(), gt[i].cpu().numpy())
            want_p = RS.psnr_restate(pred[i].cpu().numpy(), gt[i].cpu().numpy())
            assert abs(float(si) - want_s) <= TOL, (P, i)
            assert float(pi) == want_p if np.isinf(want_p) else abs(float(pi) - want_p) <= TOL, (P, i)
            alone.setdefault(names[i] if i < 4 else "flipped", []).append((si, pi))
    for name, vals in alone.items():
        assert all(torch.equal(v[0], vals[0][0]) and torch.equal(v[1], vals[0][1]) for v in vals), name


def test_nan_stays_in_its_frame(E, main_cases):
    _, pred, gt = _batch(main_cases, 3)
    s0, p0 = E.img_metrics_device(pred, gt)
    pred[1, 200, 300, 1] = float("nan")
    s, p = E.img_metrics_device(pred, gt)
    assert torch.isnan(s[1]) and torch.isnan(p[1])
    assert torch.equal(s[[0, 2]], s0[[0, 2]]) and torch.equal(p[[0, 2]], p0[[0, 2]])


def test_views_are_made_contiguous(E, main_cases):
    pred, gt = (torch.from_numpy(x).cuda() for x in main_cases["noise"])
    pv, gv = pred[17:140, 5:82], gt[17:140, 5:82]
    assert not pv.is_contiguous()
    s, p = E.img_metrics_device(pv, gv)
    want = RS.ssim_uniform(pv.cpu().numpy(), gv.cpu().numpy())
    assert abs(float(s) - want) <= TOL
    assert abs(float(p) - RS.psnr_restate(pv.cpu().numpy(), gv.cpu().numpy())) <= TOL


def test_graph_capture_and_replay(E):
    cases = RS.shape_cases()
    pred0, gt0 = cases[(120, 160, 3)]
    pred, gt = torch.from_numpy(pred0).cuda(), torch.from_numpy(gt0).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up outside the capture
        E.img_metrics_device(pred, gt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s, p = E.img_metrics_device(pred, gt)
    rng = np.random.default_rng(11)
    for k in range(3):
        new_pred = np.clip(gt0 + rng.normal(0, 0.01 * (k + 1), gt0.shape), 0, 1).astype(np.float32)
        new_gt = np.ascontiguousarray(np.roll(gt0, k, axis=0))
        pred.copy_(torch.from_numpy(new_pred))
        gt.copy_(torch.from_numpy(new_gt))
        g.replay()
        torch.cuda.synchronize()
        assert abs(float(s) - RS.ssim_uniform(new_pred, new_gt)) <= TOL, k
        assert abs(float(p) - RS.psnr_restate(new_pred, new_gt)) <= TOL, k
        es, ep = E.img_metrics_device(pred, gt)
        assert torch.equal(es, s) and torch.equal(ep, p), k


def _driver_setup():
    """The small models and poses of tests/test_gpu_driver.py (synthetic weights 61 / 62, a 9 x 13 frame, two poses)."""
    from dm_nerf_amd import distributed as D
    from oracle import ref_cpu as O
    mods = _gpu.models(13)
    H, W = 9, 13
    K = np.array([[20.0, 0, W / 2], [0, -20.0, H / 2], [0, 0, -1]])
    poses = torch.stack([O.pose_spherical(30.0, -65.0, 7.0), O.pose_spherical(80.0, -65.0, 7.0)]).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, N_test=50, N_samples=64,
                                 near=4.0, far=15.0, crop_height=7, crop_width=10, ins_num=13)
    return D, mods, (H, W, K), poses, args


def test_render_path_image_metrics(E):
    D, mods, hwk, poses, args = _driver_setup()
    H, W, _ = hwk
    mask = torch.zeros(H, W, dtype=torch.int64)
    mask[1:8, 2:12] = 1                                  # the scored frame is crop_height x crop_width = 7 x 10
    g = torch.Generator().manual_seed(2)
    for crop, (h, w) in ((None, (H, W)), (mask, (7, 10))):
        gt = torch.rand(2, h, w, 3, generator=g).cuda()
        gtl = torch.randint(0, 5, (2, h, w), generator=g)
        for labels_only in (False, True):
            with torch.no_grad():
                base = D.render_path(poses, hwk, mods, args, gt_imgs=gt, crop_mask=crop, labels_only=labels_only, gt_labels=gtl)
                out = D.render_path(poses, hwk, mods, args, gt_imgs=gt, crop_mask=crop, labels_only=labels_only, gt_labels=gtl,
                                    image_metrics=True)
            want_keys = {"rgb", "depth", "psnr", "ap", "matched", "gt_num"} | ({"label", "conf"} if labels_only else {"ins"})
            assert set(base) == want_keys                                     # image_metrics=False: the keys of today
            assert set(out) == want_keys | {"ssim", "psnr_f64"}
            for k in base:
                assert out[k].dtype == base[k].dtype and torch.equal(out[k], base[k]), k
            assert out["ssim"].shape == (2,) and out["ssim"].dtype == torch.float64 and out["psnr_f64"].dtype == torch.float64
            assert out["psnr"].dtype == torch.float32
            for i in range(2):
                rgb, gi = out["rgb"][i].cpu().numpy(), gt[i].cpu().numpy()
                assert abs(float(out["ssim"][i]) - RS.ssim_uniform(rgb, gi)) <= TOL, (crop is not None, i)
                assert abs(float(out["psnr_f64"][i]) - RS.psnr_restate(rgb, gi)) <= TOL, (crop is not None, i)
                assert abs(float(out["psnr_f64"][i]) - float(out["psnr"][i])) < 1e-3
            table = D.results_table(out)
            assert table.shape == (3, 9) and np.isnan(table[:, 2]).all()
            assert np.array_equal(table[:2, 0], out["psnr_f64"].cpu().numpy()) and np.array_equal(table[:2, 1], out["ssim"].cpu().numpy())
            assert np.array_equal(table[:2, 3:], out["ap"].double().cpu().numpy())
    with torch.no_grad():                                # without ground-truth images there is nothing to score
        plain = D.render_path(poses[:1], hwk, mods, args, image_metrics=True)
    assert set(plain) == {"rgb", "ins", "depth"}


def test_error_paths(E):
    ok = torch.rand(8, 640, 3, device="cuda")
    with pytest.raises(ValueError, match="win_size"):
        E.img_metrics_device(torch.rand(6, 640, 3, device="cuda"), torch.rand(6, 640, 3, device="cuda"))
    with pytest.raises(ValueError, match="win_size"):
        E.ssim(torch.rand(640, 6, 3, device="cuda"), torch.rand(640, 6, 3, device="cuda"))
    with pytest.raises(ValueError, match="device"):
        E.img_metrics_device(ok.cpu(), ok)
    with pytest.raises(ValueError, match="device"):
        E.psnr(ok, ok.cpu())
    with pytest.raises(ValueError, match="float32"):
        E.img_metrics_device(ok.half(), ok.half())
    with pytest.raises(ValueError, match="float32"):
        E.img_metrics_device(ok, ok.double())
    with pytest.raises(ValueError, match="shape"):
        E.img_metrics_device(ok, ok[:, :639])
    with pytest.raises(ValueError, match="shape"):
        E.img_metrics_device(ok[None], ok)
    with pytest.raises(ValueError, match="unsupported"):
        E.img_metrics_device(torch.rand(8, 8, 5, device="cuda"), torch.rand(8, 8, 5, device="cuda"))
    s, p = E.img_metrics_device(torch.empty(0, 8, 8, 3, device="cuda"), torch.empty(0, 8, 8, 3, device="cuda"))
    assert s.shape == (0,) and p.shape == (0,)
