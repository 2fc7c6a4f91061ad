"""CPU checks of the instance-AP feature (no GPU): the count-based restatement ``tests/_ins_eval_restate.py`` reproduces the
reference's ``ins_eval`` on every committed fixture (``tests/golden/ins_eval.npz``, made by ``make_golden_ins_eval.py``), so the
GPU tests can use it on frames too large for the reference; and the new C entry points reject bad arguments before anything
reaches a device."""
import numpy as np
import pytest

import _ins_eval_restate as RS


def test_restatement_reproduces_the_reference_fixtures():
    fx = RS.load_fixtures()
    assert len(fx) >= 10
    for name, z in fx.items():
        f = z.__getitem__
        pred = f("pred_ins")
        ins_num, gt_num = int(f("ins_num")), int(f("gt_num"))
        mask = f("mask") if int(f("has_mask")) else None
        label, conf = RS.label_conf(pred)
        rows = RS.gt_rows_from_onehot(f("gt_ins"), gt_num)
        lab, ap, ret = RS.ins_eval(label, conf, rows, gt_num, ins_num, mask)
        assert np.array_equal(lab.reshape(pred.shape[:2]), f("pred_label")), name
        assert np.array_equal(ret, f("return_labels")), name
        assert np.asarray(ap, dtype=np.float64).tobytes() == f("ap").tobytes(), (name, ap, f("ap"))


def test_fixtures_cover_the_reference_branches():
    seen = set()
    for name, z in RS.load_fixtures().items():
        f = z.__getitem__
        ins_num, gt_num = int(f("ins_num")), int(f("gt_num"))
        mask = f("mask") if int(f("has_mask")) else None
        label, conf = RS.label_conf(f("pred_ins"))
        rows = RS.gt_rows_from_onehot(f("gt_ins"), gt_num)
        lab, _, ret, d = RS.ins_eval(label, conf, rows, gt_num, ins_num, mask, details=True)
        seen.add(ins_num)
        counts = np.bincount(lab, minlength=ins_num + 1)[d["valid"]]
        if (counts % 2 == 0).any() and (counts % 2 == 1).any():
            seen.add("even+odd")
        if mask is not None and (mask != 0).all():
            seen.add("mask quirk")
        if mask is not None and (mask == 0).any():
            seen.add("crop")
        if len(d["valid"]) < gt_num:
            seen.add("V < gt_num")
        if len(d["valid"]) == 0:
            seen.add("V = 0")
        if (ret == -1).any():
            seen.add("unmatched row")
        if len(set(d["confidence"][d["cols"] < len(d["valid"])].tolist())) < int((d["cols"] < len(d["valid"])).sum()):
            seen.add("tied medians")
        if int(f("reference_raises")):
            seen.add("reference raises")
    for want in (13, 59, 93, "even+odd", "mask quirk", "crop", "V < gt_num", "V = 0", "unmatched row", "tied medians", "reference raises"):
        assert want in seen, want


def test_median_and_sum_order_helpers():
    import torch
    rng = np.random.default_rng(5)
    for n in (1, 3, 7, 8, 9, 31, 64, 95, 130):
        x = (rng.random(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype(np.float32)
        assert RS.ata_sum_f32(x) == torch.from_numpy(x).sum().numpy(), n
    a = np.float32([0.1, 0.7, 0.3, 0.9])
    assert np.median(a) == np.float32((np.float32(0.3) + np.float32(0.7)) / np.float32(2))


def test_ins_eval_entry_points_validate_before_the_device():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    assert lib.dmnerf_ins_eval_work_bytes(100, 129) == -1 and lib.dmnerf_ins_eval_work_bytes(0, 13) == -1
    nb = lib.dmnerf_ins_eval_work_bytes(640 * 480, 93)
    assert 0 < nb < 8 << 20
    assert lib.dmnerf_ins_eval_flags_offset(10, 13) == 0
    # null work / label, bad gt_num, no prediction, no ground truth, short work buffer: DMNERF_E_ARG with a message
    rc = lib.dmnerf_ins_eval_prep(None, 0, None, None, None, None, None, 0, None, None, 3, 100, 13, None, 0, None)
    assert rc == -1 and "null" in _lib.last_error()
    fake = 1 << 20                                           # never dereferenced: validation fails first
    rc = lib.dmnerf_ins_eval_prep(fake, 13, None, None, fake, None, fake, 13, None, None, 14, 100, 13, fake, nb, None)
    assert rc == -1 and "gt_num" in _lib.last_error()
    rc = lib.dmnerf_ins_eval_prep(fake, 12, None, None, fake, None, fake, 13, None, None, 3, 100, 13, fake, nb, None)
    assert rc == -1 and "pred_ins" in _lib.last_error()
    rc = lib.dmnerf_ins_eval_prep(fake, 13, None, None, fake, None, None, 0, fake, None, 3, 100, 13, fake, nb, None)
    assert rc == -1 and "gt" in _lib.last_error()
    rc = lib.dmnerf_ins_eval_prep(fake, 13, None, None, fake, None, fake, 13, None, None, 3, 100, 13, fake, 16, None)
    assert rc == -1 and "too small" in _lib.last_error()
    rc = lib.dmnerf_ins_eval(100, 13, 3, 0, None, nb, None, None, None)
    assert rc == -1 and "null" in _lib.last_error()
    rc = lib.dmnerf_ins_eval(100, 13, 3, 0, fake, 8, fake, fake, None)
    assert rc == -1 and "too small" in _lib.last_error()


def test_cpu_tensors_are_refused():
    import torch
    from dm_nerf_amd.networks import evaluator as E
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.ins_eval(torch.rand(4, 5, 13), torch.zeros(4, 5, 13), 2, 13)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        E.ins_eval_device(torch.zeros(4, 5, dtype=torch.int64), torch.rand(4, 5), torch.zeros(4, 5, dtype=torch.int64),
                          torch.tensor([0]), 13)
