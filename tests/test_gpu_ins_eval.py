"""Instance AP on the device (csrc/ins_eval.hip, ``evaluator.ins_eval`` / ``ins_eval_device``, ``render_path(gt_labels=)``):

* the reference fixtures (tests/golden/ins_eval.npz): ``pred_label`` and ``return_labels`` equal, ``ap`` within 2e-7;
* random 480 x 640 frames at ins_num 13 / 59 / 93 with and without a mask against the count-based restatement
  (tests/_ins_eval_restate.py, itself pinned to the reference on the CPU): labels and per-label medians equal; the matched labels
  and APs equal wherever the optimal assignment is unique by more than 1e-5, else the device's total cost is optimal within 1e-5;
* a label covering most of a frame and a single-pixel label; render_path with gt_labels and a crop; HIP-graph replay; errors."""
import types

import numpy as np
import pytest
import torch

import _gpu
import _ins_eval_restate as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from dm_nerf_amd import _lib
    from dm_nerf_amd.networks import evaluator
    _lib.load()
    return evaluator


def _medians(E, label, conf, gt_label, rows, ins_num, mask=None):
    """Device run through the private driver, returning the per-label medians from the work buffer as well."""
    from dm_nerf_amd import _lib
    lab = label.reshape(-1).contiguous()
    N = lab.shape[0]
    m = None if mask is None else mask.reshape(-1).float().contiguous()
    gl = gt_label.reshape(-1).contiguous()
    out = E._ins_eval_run(N, ins_num, rows.shape[0], m is not None, lab.device,
                          lambda o: (None, 0, _lib.ptr(lab), _lib.ptr(conf.reshape(-1)), _lib.ptr(o), _lib.ptr(m), None, 0,
                                     _lib.ptr(gl), _lib.ptr(rows)))
    off = _lib.load().dmnerf_ins_eval_median_offset(N, ins_num)
    med = out[3][off:off + 4 * ins_num].view(torch.float32)
    return out[0], out[1], out[2], med


def test_reference_fixtures(E):
    exact = 0
    for name, z in RS.load_fixtures().items():
        ins_num, gt_num = int(z["ins_num"]), int(z["gt_num"])
        mask = torch.from_numpy(z["mask"]).cuda() if int(z["has_mask"]) else None
        pred = torch.from_numpy(z["pred_ins"]).cuda()
        gt = torch.from_numpy(z["gt_ins"]).float().cuda()
        label, ap, ret = E.ins_eval(pred, gt, gt_num, ins_num, mask, check=True)
        assert torch.equal(label.cpu(), torch.from_numpy(z["pred_label"])), name
        assert np.array_equal(ret, z["return_labels"]), (name, ret, z["return_labels"])
        d = np.abs(np.asarray(ap) - z["ap"]).max()
        assert d <= 2e-7, (name, ap, z["ap"])
        exact += int(d == 0)
        # the same frame through ins_eval_device: labels / confidences and gt rows as ids (row g = label g)
        lab, conf = E.ins_label_conf(pred)
        rows_px = torch.from_numpy(RS.gt_rows_from_onehot(z["gt_ins"], gt_num)).cuda()
        l2, ap2, m2 = E.ins_eval_device(lab, conf, rows_px.reshape(lab.shape), torch.arange(gt_num, device="cuda"), ins_num, mask)
        assert torch.equal(l2, label) and torch.equal(ap2.cpu().double(), torch.tensor(ap, dtype=torch.float64)), name
        assert np.array_equal(m2.cpu().numpy()[:gt_num], ret) and bool((m2[gt_num:] == -1).all()), name
    print(f"ins_eval fixtures: ap bit-equal to the reference in {exact} of {len(RS.load_fixtures())} cases")


def _frame(rng, H, W, ins_num, n_gt, big=None, single=False):
    """Blocky gt labels, predictions = a relabelled, shifted, noisy copy; confidences from a few levels plus noise."""
    bs = 40
    small = rng.choice(n_gt, size=(-(-H // bs), -(-W // bs)))
    gt = np.kron(small, np.ones((bs, bs), dtype=np.int64))[:H, :W]
    if big is not None:
        gt[:, : int(W * big)] = 0
    flip = rng.random((H, W)) < 0.03
    gt[flip] = rng.integers(0, n_gt, size=int(flip.sum()))
    perm = rng.permutation(ins_num)
    pl = np.roll(perm[gt], shift=(3, 5), axis=(0, 1))
    flip = rng.random((H, W)) < 0.05
    pl[flip] = rng.integers(0, ins_num, size=int(flip.sum()))
    if single:                                       # one label with a single pixel
        lone = int(perm[-1])
        pl[pl == lone] = int(perm[0])
        pl[H // 2, W // 2] = lone
    conf = (rng.choice(np.float32([0.5, 0.625, 0.75, 0.875]), size=(H, W))
            + rng.integers(0, 64, size=(H, W)).astype(np.float32) / np.float32(4096)).astype(np.float32)
    return pl, conf, gt


def _check_frame(E, pl, conf, gt, ins_num, mask, tag):
    rows = np.unique(gt)
    rows_t = torch.from_numpy(rows).cuda()
    lab_d, ap_d, m_d, med_d = _medians(E, torch.from_numpy(pl).cuda(), torch.from_numpy(conf).cuda(), torch.from_numpy(gt).cuda(),
                                       rows_t, ins_num, None if mask is None else torch.from_numpy(mask).cuda())
    g_row = np.searchsorted(rows, gt)
    lab, ap, ret, det = RS.ins_eval(pl, conf, g_row, len(rows), ins_num, mask, details=True)
    assert np.array_equal(lab_d.cpu().numpy().reshape(-1), lab), tag
    med_all = med_d.cpu().numpy()
    assert np.array_equal(med_all[det["valid"][det["valid"] < ins_num]], det["medians"][det["valid"] < ins_num]), tag
    gt_num = len(rows)
    m_d = m_d.cpu().numpy()[:gt_num]
    margin = RS.assignment_margin(det["cost"], det["cols"])
    if margin > 1e-5:
        assert np.array_equal(m_d, ret), (tag, margin)
        assert np.array_equal(ap_d.cpu().numpy().astype(np.float64), np.asarray(ap, dtype=np.float64)), (tag, ap_d, ap)
    else:                                            # a (near-)tie: the device's assignment is optimal on the restatement's matrix
        valid = list(det["valid"])
        cols_d = np.array([valid.index(l) if l >= 0 else -1 for l in m_d])
        free = [c for c in range(ins_num) if c not in set(cols_d[cols_d >= 0]) and c >= len(valid)]
        cols_d[cols_d < 0] = free[:int((cols_d < 0).sum())]
        tot_d = det["cost"][np.arange(gt_num), cols_d].astype(np.float64).sum()
        tot = det["cost"][np.arange(gt_num), det["cols"]].astype(np.float64).sum()
        assert abs(tot_d - tot) <= 1e-5, (tag, tot_d, tot)
    return margin


@pytest.mark.parametrize("ins_num,n_gt", [(13, 11), (59, 50), (93, 80)])
def test_random_frames_vs_restatement(E, ins_num, n_gt):
    rng = np.random.default_rng(ins_num)
    H, W = 480, 640
    pl, conf, gt = _frame(rng, H, W, ins_num, n_gt)
    _check_frame(E, pl, conf, gt, ins_num, None, f"{ins_num} no mask")
    mask = (rng.random((H, W)) > 0.1).astype(np.float32)
    mask[:40] = 0
    _check_frame(E, pl, conf, gt, ins_num, mask, f"{ins_num} mask")


def test_large_and_single_pixel_labels(E):
    rng = np.random.default_rng(7)
    pl, conf, gt = _frame(rng, 480, 640, 59, 20, big=0.9, single=True)
    counts = np.bincount(pl.reshape(-1), minlength=59)
    assert counts.max() > 0.8 * pl.size and (counts == 1).any()
    _check_frame(E, pl, conf, gt, 59, None, "big + single")


def test_ins_eval_device_graph_replay(E):
    rng = np.random.default_rng(11)
    frames = [_frame(rng, 120, 160, 59, 30) for _ in range(3)]
    rows = torch.arange(30, device="cuda")
    st = [torch.from_numpy(x).cuda() for x in frames[0]]
    mask = torch.ones(120, 160, device="cuda")
    eager = []
    for pl, conf, gt in frames[1:]:
        eager.append([t.clone() for t in E.ins_eval_device(torch.from_numpy(pl).cuda(), torch.from_numpy(conf).cuda(),
                                                           torch.from_numpy(gt).cuda(), rows, 59, mask)])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        E.ins_eval_device(st[0], st[1], st[2], rows, 59, mask)           # warm-up (attributes, allocator)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = E.ins_eval_device(st[0], st[1], st[2], rows, 59, mask)
    for (pl, conf, gt), want in zip(frames[1:], eager):
        for dst, src in zip(st, (pl, conf, gt)):
            dst.copy_(torch.from_numpy(src))
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)


def test_render_path_gt_labels_crop(E):
    from dm_nerf_amd import distributed as D
    from oracle import ref_cpu as O
    ins_num = 13
    mods = _gpu.models(ins_num, seeds=(1, 2))
    H, W = 24, 32
    K = O.dmsr_intrinsics(H, W)
    poses = torch.stack([O.pose_spherical(30.0, -65.0, 7.0), O.pose_spherical(90.0, -50.0, 7.0)]).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=64, is_train=False, N_ins=None, N_test=256, N_samples=32, near=4.0,
                                 far=15.0, crop_height=20, crop_width=26, ins_num=ins_num)
    crop = torch.zeros(H, W, dtype=torch.int64)
    crop[2:22, 3:29] = 1
    rng = np.random.default_rng(3)
    gtl = np.kron(rng.integers(0, 9, size=(2, 4, 6)), np.ones((1, 5, 5), dtype=np.int64))[:, :20, :26].copy()
    gtl[0, :3] = 200                                 # labels >= ins_num: masked by the crop branch
    gtl[:, :, -1] = 255
    with torch.no_grad():
        out = D.render_path(poses, (H, W, K), mods, args, crop_mask=crop, labels_only=True, gt_labels=torch.from_numpy(gtl))
        full = D.render_path(poses, (H, W, K), mods, args, crop_mask=crop)
    assert out["ap"].shape == (2, 6) and out["matched"].shape == (2, ins_num) and out["gt_num"].shape == (2,)
    for i in range(2):
        lab, conf = RS.label_conf(full["ins"][i].cpu().numpy())
        g = gtl[i]
        rows = np.unique(g)[:-1]                     # tester.py:99-106
        g_row = np.where(np.isin(g, rows), np.searchsorted(rows, g), -1)
        _, ap, ret = RS.ins_eval(lab, conf, g_row, len(rows), ins_num, (g < ins_num).astype(np.float32))
        assert int(out["gt_num"][i]) == len(rows)
        assert np.array_equal(out["matched"][i].cpu().numpy()[:len(rows)], ret), i
        assert np.array_equal(out["ap"][i].cpu().numpy().astype(np.float64), np.asarray(ap)), i
    # a pose without gt rows: six APs of 1.0 (the reference's tensor([1.0]))
    empty = D.render_path(poses[:1], (H, W, K), mods, args, crop_mask=crop, labels_only=True,
                          gt_labels=torch.full((1, 20, 26), 255, dtype=torch.int64))
    assert torch.equal(empty["ap"][0].cpu(), torch.ones(6)) and int(empty["gt_num"][0]) == 0


def test_error_paths(E):
    pred = torch.rand(8, 8, 13, device="cuda")
    gt = torch.zeros(8, 8, 13, device="cuda")
    gt[..., 0] = 1
    gt[0, 0, 1] = 1                                  # two ones in one pixel
    with pytest.raises(ValueError, match="one-hot"):
        E.ins_eval(pred, gt, 3, 13, check=True)
    gt[0, 0, 1] = 0.5
    with pytest.raises(ValueError, match="one-hot"):
        E.ins_eval(pred, gt, 3, 13, check=True)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.ins_eval(pred.cpu(), gt, 3, 13)
    with pytest.raises(ValueError, match="gt_num=14"):
        E.ins_eval(pred, torch.zeros(8, 8, 14, device="cuda"), 14, 13)
    # a channel slice of a wider tensor needs no copy: ins[..., :-1] of manipulator_eval
    wide = torch.rand(8, 8, 14, device="cuda")
    gt[0, 0, 1] = 0
    a = E.ins_eval(wide[..., :-1], gt, 3, 13)
    b = E.ins_eval(wide[..., :-1].contiguous(), gt, 3, 13)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
