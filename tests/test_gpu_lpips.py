"""LPIPS (VGG16) on the device -- csrc/conv3x3.hip, csrc/lpips.hip, ``evaluator.LPIPSVGG``, ``render_path(lpips=)`` -- against the
float64 restatement tests/_lpips_restate.py (held against hand-computable cases by tests/test_lpips_restate.py), with random
weights: the pretrained ones can be neither shipped nor fetched.

Tolerances.  The device sums f32 chains of up to 4608 terms; how close f32 can be to the float64 referee is measured, not guessed:
the restatement is run in float32 on the CPU on the same cases, and per compared quantity the worst deviation from float64 over
all cases is taken -- the relative error of the score; for a feature map max |error| / max |value|.  The device must be within
4 x that worst case (a differently ordered f32 sum of the same length is the same class of arithmetic, not the same rounding, and
a single number's error fluctuates by a small factor between orders).  The constants below are those CPU measurements (x86-64,
torch 2.x, seed and cases of _lpips_restate.METRIC_CASES / conv_cases()); none comes from the kernels' output.  A border, tap-order
or pooling mistake is an O(1) error."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gpu
import _lpips_restate as RS

pytestmark = pytest.mark.gpu

# float32 restatement vs float64, worst over METRIC_CASES (measured on the CPU):
F32_SCORE_REL = 1.18e-6                # relative error of the score
F32_FEAT_REL = (1.03e-6, 1.41e-6, 1.78e-6, 2.33e-6, 2.64e-6)               # per tap: max abs error / max abs value
# float32 F.conv2d vs float64, worst over conv_cases(): max abs error / max abs value of the output
F32_CONV_REL = 2.46e-6
FACTOR = 4.0
TOL_SCORE = FACTOR * F32_SCORE_REL
TOL_FEAT = tuple(FACTOR * v for v in F32_FEAT_REL)
TOL_CONV = FACTOR * F32_CONV_REL

CONV_CHANNELS = ((32, 32), (64, 128), (256, 320), (512, 512))
CONV_IMAGES = ((1, 1, 1), (1, 5, 7), (3, 11, 13))       # (batch, H, W): all border but the centre tap | odd | M % 128 != 0, odd row length, images sharing a tile


def conv_cases():
    g = torch.Generator().manual_seed(7)
    cases = []
    for cin, cout in CONV_CHANNELS:
        for n, h, w in CONV_IMAGES:
            cases.append(dict(name=f"{cin}->{cout} {n}x{h}x{w}", x=torch.randn(n, h, w, cin, generator=g),
                              w=torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin)), b=0.05 * torch.randn(cout, generator=g)))
    return cases


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator
    _lib.load()
    return evaluator


@pytest.fixture(scope="module")
def sd():
    return RS.random_state_dict(0)


@pytest.fixture(scope="module")
def model(E, sd):
    return E.LPIPSVGG.from_state_dict({k: v.cuda() for k, v in sd.items()})


@pytest.fixture(scope="module")
def metric_refs(sd):
    """Per case: frames and the float64 restatement's (feature maps, score); computed once, never modified."""
    refs = []
    for P, H, W, seed in RS.METRIC_CASES:
        pred, gt = RS.frames(P, H, W, seed)
        feats, score = RS.lpips_restate(pred, gt, sd, torch.float64)
        refs.append((pred, gt, feats, score))
    return refs


def test_conv3x3_against_float64(E):
    worst = 0.0
    for case in conv_cases():
        x, w, b = case["x"], case["w"], case["b"]
        n, h, wd, cin = x.shape
        cout = w.shape[0]
        want = F.relu(F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)).permute(0, 2, 3, 1)
        xin = E.padded_flat(x.cuda())
        out = torch.full((xin.shape[0], cout), float("nan"), device="cuda")      # every row must be written
        E.conv3x3(xin, E.conv3x3_pack(w.cuda()), b.cuda(), n, h, wd, out=out)
        out = out.cpu()
        img = E.padded_flat_images(out, n, h, wd)
        err = RS.rel_feature_error(img[:, 1:-1, 1:-1], want)
        worst = max(worst, err)
        print(f"conv {case['name']}: max abs err / max abs {err:.3e} (bound {TOL_CONV:.3e})")
        assert err <= TOL_CONV, case["name"]
        # the zero border and the guard rows: exactly 0.0
        border = img.clone()
        border[:, 1:-1, 1:-1] = 0
        assert torch.equal(border, torch.zeros_like(border)), case["name"]
        g = wd + 3
        assert torch.equal(out[:g], torch.zeros(g, cout)) and torch.equal(out[-g:], torch.zeros(g, cout)), case["name"]
    print(f"conv worst {worst:.3e}")


def test_conv3x3_border_by_select(E):
    """A NaN pixel reaches its 3 x 3 neighbourhood and nothing else; border rows that accumulated it are still exact zeros."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 5, 7, 32, generator=g)
    w, b = torch.randn(64, 32, 3, 3, generator=g) * 0.1, torch.zeros(64)
    clean = E.conv3x3(E.padded_flat(x.cuda()), E.conv3x3_pack(w.cuda()), b.cuda(), 2, 5, 7, relu=False).cpu()
    x[0, 0, 6, 3] = float("nan")                          # a corner pixel of image 0: its neighbours include border positions
    out = E.conv3x3(E.padded_flat(x.cuda()), E.conv3x3_pack(w.cuda()), b.cuda(), 2, 5, 7, relu=False).cpu()
    img, ref = E.padded_flat_images(out, 2, 5, 7), E.padded_flat_images(clean, 2, 5, 7)
    hit = torch.zeros(2, 7, 9, dtype=torch.bool)
    hit[0, 1:3, 6:8] = True                               # pixels (0..1, 5..6) in padded coordinates
    assert bool(torch.isnan(img[hit]).all())
    assert torch.equal(img[~hit], ref[~hit])


def test_maxpool2(E):
    g = torch.Generator().manual_seed(3)
    for n, h, w, c in ((2, 5, 7, 64), (1, 6, 6, 32)):
        x = torch.randn(n, h, w, c, generator=g)
        out = E.maxpool2(E.padded_flat(x.cuda()), n, h, w).cpu()
        img = E.padded_flat_images(out, n, h // 2, w // 2)
        want = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(img[:, 1:-1, 1:-1], want), (h, w)
        ref = E.padded_flat(want)
        assert torch.equal(out, ref), (h, w)                # borders and guards exactly zero


def test_metric_against_float64(model, metric_refs):
    for (P, H, W, seed), (pred, gt, feats, score) in zip(RS.METRIC_CASES, metric_refs):
        got_f = []
        got = model(pred.cuda(), gt.cuda(), features=got_f)
        assert got.shape == (P,) and got.dtype == torch.float64 and len(got_f) == 5
        for k in range(5):
            assert got_f[k].shape == feats[k].shape, (H, W, k)
            err = RS.rel_feature_error(got_f[k].cpu(), feats[k])
            print(f"{H}x{W} tap {k}: max abs err / max abs {err:.3e} (bound {TOL_FEAT[k]:.3e})")
            assert err <= TOL_FEAT[k], (H, W, k)
        rel = float(((got.cpu() - score).abs() / score.abs()).max())
        print(f"{H}x{W} score {got.tolist()} want {score.tolist()}: rel err {rel:.3e} (bound {TOL_SCORE:.3e})")
        assert rel <= TOL_SCORE, (H, W)


def test_normalize_flag_and_single_frame(E, model, sd):
    pred, gt = RS.frames(1, 16, 20, 21)
    _, want = RS.lpips_restate(pred[0], gt[0], sd, torch.float64, normalize=True)
    got = model(pred[0].cuda(), gt[0].cuda(), normalize=True)
    assert got.dim() == 0 and abs(float(got) - float(want)) <= TOL_SCORE * float(want)
    _, want0 = RS.lpips_restate(pred[0], gt[0], sd, torch.float64)
    assert abs(E.lpips(model, pred[0].cuda(), gt[0].cuda()) - float(want0)) <= TOL_SCORE * float(want0)


def test_independence_and_determinism(model):
    pred, gt = RS.frames(3, 21, 18, 31)
    pred, gt = pred.cuda(), gt.cuda()
    a = model(pred, gt)
    b = model(pred, gt)
    assert torch.equal(a, b)                              # two runs: bit-identical
    for i in range(3):                                    # P = 3 equals three P = 1 calls bit for bit
        assert torch.equal(model(pred[i:i + 1], gt[i:i + 1])[0], a[i]), i
    bad = pred.clone()
    bad[1, 7, 5, 1] = float("nan")
    c = model(bad, gt)
    assert bool(torch.isnan(c[1])) and torch.equal(c[0], a[0]) and torch.equal(c[2], a[2])
    z = model(pred, pred.clone())
    assert torch.equal(z, torch.zeros(3, dtype=torch.float64, device="cuda"))      # identical frames: exactly 0


def _driver_setup():
    """The small models of tests/test_gpu_img_metrics.py's driver test, a 17 x 19 frame, two poses."""
    from dm_nerf_amd import distributed as D
    from oracle import ref_cpu as O
    mods = _gpu.models(13)
    H, W = 17, 19
    K = np.array([[20.0, 0, W / 2], [0, -20.0, H / 2], [0, 0, -1]])
    poses = torch.stack([O.pose_spherical(30.0, -65.0, 7.0), O.pose_spherical(80.0, -65.0, 7.0)]).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, N_test=100, N_samples=64,
                                 near=4.0, far=15.0, crop_height=16, crop_width=16, ins_num=13)
    return D, mods, (H, W, K), poses, args


def test_render_path_plumbing(model):
    D, mods, hwk, poses, args = _driver_setup()
    H, W, _ = hwk
    mask = torch.zeros(H, W, dtype=torch.int64)
    mask[1:17, 2:18] = 1                                  # the scored frame is 16 x 16
    g = torch.Generator().manual_seed(2)
    for crop, (h, w) in ((None, (H, W)), (mask, (16, 16))):
        gt = torch.rand(2, h, w, 3, generator=g).cuda()
        gtl = torch.randint(0, 5, (2, h, w), generator=g)
        with torch.no_grad():
            base = D.render_path(poses, hwk, mods, args, gt_imgs=gt, crop_mask=crop, labels_only=True, gt_labels=gtl, image_metrics=True)
            out = D.render_path(poses, hwk, mods, args, gt_imgs=gt, crop_mask=crop, labels_only=True, gt_labels=gtl, image_metrics=True,
                                lpips=model)
        assert "lpips" not in base and set(out) == set(base) | {"lpips"}
        for k in base:                                    # without lpips=: what the call returns today
            assert out[k].dtype == base[k].dtype and torch.equal(out[k], base[k]), k
        assert out["lpips"].shape == (2,) and out["lpips"].dtype == torch.float64
        assert torch.equal(out["lpips"], model(out["rgb"], gt))       # the frame ssim scores
        table = D.results_table(out)
        assert table.shape == (3, 9)
        assert np.array_equal(table[:2, 2], out["lpips"].cpu().numpy()) and table[2, 2] == table[:2, 2].mean()
        assert np.array_equal(table[:2, 1], out["ssim"].cpu().numpy()) and np.array_equal(table[:2, 3:], out["ap"].double().cpu().numpy())
        assert np.isnan(D.results_table(base)[:, 2]).all()                               # no model: the nan column of today
        assert np.array_equal(D.results_table(out, lpips=[1.0, 2.0])[:, 2], [1.0, 2.0, 1.5])      # an explicit lpips= still wins
    with torch.no_grad():                                 # without ground-truth images there is nothing to score
        plain = D.render_path(poses[:1], hwk, mods, args, lpips=model)
    assert set(plain) == {"rgb", "ins", "depth"}


def test_manipulate_eval_path_plumbing(model):
    from dm_nerf_amd import distributed as D, editing as ED
    from oracle import ref_cpu as O
    H, W, INS = 16, 18, 7
    mods = _gpu.models(INS, seeds=(721, 722))
    K = O.dmsr_intrinsics(H, W)
    poses = [O.pose_spherical(75.0, -65.0, 7.0), O.pose_spherical(60.0, -60.0, 7.0)]
    trans = torch.tensor([[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])
    gen = torch.Generator().manual_seed(4)
    gt_rgbs = torch.rand(2, H, W, 3, generator=gen)
    gt_labels = torch.tensor([0, 2, 5])[torch.randint(0, 3, (2, H, W), generator=gen)]
    a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=64, target_label=2, ins_num=INS)
    outs = []
    for kw in ({}, {"lpips": model}):
        torch.manual_seed(3); torch.cuda.manual_seed(3)
        with torch.no_grad():
            outs.append(ED.manipulate_eval_path(poses, (H, W, K), tuple(mods), a, trans, gt_rgbs=gt_rgbs, gt_labels=gt_labels, keep_maps=True, **kw))
    base, out = outs
    assert "lpips" not in base and set(out) == set(base) | {"lpips"}
    for k in base:
        assert torch.equal(out[k], base[k]), k
    assert torch.equal(out["lpips"], model(out["rgb"], gt_rgbs.cuda()))
    table = D.results_table(out)
    assert np.array_equal(table[:2, 2], out["lpips"].cpu().numpy()) and np.isnan(D.results_table(base)[:, 2]).all()
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    with torch.no_grad():                                 # scored without image_metrics, frames not kept
        only = ED.manipulate_eval_path(poses, (H, W, K), tuple(mods), a, trans, gt_rgbs=gt_rgbs, image_metrics=False, lpips=model)
    assert sorted(only) == ["lpips", "psnr", "rgb8", "tar_rgb8"] and torch.equal(only["lpips"], out["lpips"])


def test_capturable(model):
    pred, gt = RS.frames(2, 16, 24, 41)
    pred, gt = pred.cuda(), gt.cuda()
    want = model(pred, gt)                                # (allocates the workspace of this shape)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = model(pred, gt)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    pred2, gt2 = RS.frames(2, 16, 24, 42)
    want2 = model(pred2.cuda(), gt2.cuda()).clone()
    pred.copy_(pred2.cuda()); gt.copy_(gt2.cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want2)


def test_argument_errors(E, model, sd):
    ok = torch.rand(16, 16, 3, device="cuda")
    with pytest.raises(ValueError, match="16 x 16"):
        model(torch.rand(15, 40, 3, device="cuda"), torch.rand(15, 40, 3, device="cuda"))
    with pytest.raises(ValueError, match="16 x 16"):
        model(torch.rand(2, 40, 12, 3, device="cuda"), torch.rand(2, 40, 12, 3, device="cuda"))
    with pytest.raises(ValueError, match="device"):
        model(ok.cpu(), ok)
    with pytest.raises(ValueError, match="device"):
        model(ok, ok.cpu())
    with pytest.raises(ValueError, match="shape"):
        model(torch.rand(16, 16, 4, device="cuda"), torch.rand(16, 16, 4, device="cuda"))
    with pytest.raises(ValueError, match="float32"):
        model(ok.double(), ok.double())
    dev = {k: v.cuda() for k, v in sd.items()}
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        E.LPIPSVGG.from_state_dict({k: v for k, v in dev.items() if k != "lin3.model.1.weight"})
    with pytest.raises(ValueError, match=r"net\.slice2\.5\.bias.*device"):
        E.LPIPSVGG.from_state_dict(dict(dev, **{"net.slice2.5.bias": sd["net.slice2.5.bias"]}))
    # the C entries report bad sizes before anything touches the device; P == 0 is a no-op
    from dm_nerf_amd import _lib
    lib = _lib.load()
    assert lib.dmnerf_lpips_work_bytes(1, 15, 64) == -1 and lib.dmnerf_lpips_work_bytes(1, 64, 5000) == -1 and lib.dmnerf_lpips_work_bytes(0, 64, 64) == 0
    assert lib.dmnerf_conv3x3(None, 0, None, 0, None, None, 0, 1, 4, 4, 48, 64, 9, 1, None) == -1
    assert lib.dmnerf_conv3x3(None, 0, None, 0, None, None, 0, 0, 4, 4, 64, 64, 9, 1, None) == 0
    assert lib.dmnerf_maxpool2(None, 0, None, 0, 1, 1, 4, 64, None) == -1 and lib.dmnerf_maxpool2(None, 0, None, 0, 0, 4, 4, 64, None) == 0
    assert lib.dmnerf_lpips_prologue(None, None, -1, 16, 16, 0, None, 0, None) == -1 and lib.dmnerf_lpips_prologue(None, None, 0, 16, 16, 0, None, 0, None) == 0
    assert lib.dmnerf_lpips_tail(None, 0, None, 1, 4, 4, 48, 1, None, 0, None, None) == -1 and lib.dmnerf_lpips_tail(None, 0, None, 0, 4, 4, 64, 1, None, 0, None, None) == 0
    assert lib.dmnerf_conv3x3_pack(None, 64, 5, None, 64, None) == -1
    assert model(torch.rand(0, 16, 16, 3, device="cuda"), torch.rand(0, 16, 16, 3, device="cuda")).shape == (0,)
