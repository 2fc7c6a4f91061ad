"""Generate ``tests/golden/ins_eval.npz`` by RUNNING THE REFERENCE's ``ins_eval`` (build container only).

    DMNERF_REFERENCE=<reference checkout> python tests/golden/make_golden_ins_eval.py      # writes tests/golden/ins_eval.npz

Each case is one small synthetic frame: ``pred_ins [H, W, ins_num]`` (a low background plus one winning channel per pixel, some
pixels with two equal maxima), the one-hot ``gt_ins [H, W, ins_num]`` the reference's tester builds from a blocky label map
(networks/tester.py:97-118, both branches), and the mask of the crop branch.  The reference's ``networks/evaluator.py`` runs on
them unmodified; its outputs (``pred_label``, the six APs, ``return_labels``) are stored next to the inputs, and the count-based
restatement ``tests/_ins_eval_restate.py`` must reproduce every one of them exactly before anything is written.

The fixtures are data only (inputs and expected outputs); no reference source travels.
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("DMNERF_REFERENCE")
if not REF:
    sys.exit("set DMNERF_REFERENCE to a checkout of the reference (its networks/evaluator.py is what runs)")
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import _ins_eval_restate as RS  # noqa: E402

import networks.evaluator as R_eval  # noqa: E402  (reference)

torch.autograd.set_detect_anomaly(False)
torch.set_num_threads(1)
OUT = os.environ.get("DMNERF_GOLDEN_OUT", HERE)


def blocky(rng, H, W, labels, block, noise):
    """A label map of ``block``-sized tiles drawn from ``labels``, ``noise`` of the pixels redrawn."""
    hb, wb = -(-H // block), -(-W // block)
    small = rng.choice(labels, size=(hb, wb))
    lab = np.kron(small, np.ones((block, block), dtype=np.int64))[:H, :W]
    flip = rng.random((H, W)) < noise
    lab[flip] = rng.choice(labels, size=int(flip.sum()))
    return lab


def pred_from_labels(rng, lab, ins_num, levels=None, ties=0.02):
    """``pred_ins [H, W, ins_num]``: background 0.01 k (k in 0..3), the pixel's label channel raised to a random value in (0.3, 1)
    (or one of ``levels``); ``ties`` of the pixels get a second channel equal to the maximum (first maximum wins)."""
    H, W = lab.shape
    x = (0.01 * rng.integers(0, 4, size=(H, W, ins_num))).astype(np.float32)
    if levels is None:
        top = rng.uniform(0.3, 1.0, size=(H, W)).astype(np.float32)
    else:
        top = rng.choice(np.asarray(levels, dtype=np.float32), size=(H, W))
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x[ii, jj, lab] = top
    tie = rng.random((H, W)) < ties
    other = rng.integers(0, ins_num, size=(H, W))
    x[ii[tie], jj[tie], other[tie]] = top[tie]
    return x


def gt_onehot(gt_label, ins_num, crop):
    """tester.py:97-118: rows = unique(gt_label) (crop: without its largest value), gt_ins[..., :rows] = one_hot[..., rows]."""
    g = torch.from_numpy(gt_label)
    rows = torch.unique(g)[:-1] if crop else torch.unique(g)
    gt_ins = torch.zeros(gt_label.shape + (ins_num,))
    gt_ins[..., :len(rows)] = F.one_hot(g.long())[..., rows.long()].float()
    mask = (g < ins_num).float() if crop else None
    return gt_ins, len(rows), mask


def case(rng, ins_num, H, W, n_gt, n_pred=None, crop=False, mask_ones=False, mask_zeros=False, levels=None, block=8, noise=0.03, shift=(0, 1), ties=0.02):
    gt_labels = np.sort(rng.choice(ins_num, size=n_gt, replace=False))
    gt = blocky(rng, H, W, gt_labels, block, noise)
    if crop:                                              # a border of the crop label 255, as ScanNet's crops leave
        gt[:2, :] = 255
        gt[:, -3:] = 255
    # predictions: the gt tiles under a random relabelling, a shifted copy, more noise; n_pred limits the labels used
    perm = rng.permutation(ins_num)
    plab = perm[np.clip(gt, 0, ins_num - 1)]
    plab = np.roll(plab, shift=shift, axis=(0, 1))
    if n_pred is not None:
        pool = rng.choice(ins_num, size=n_pred, replace=False)
        plab = pool[plab % n_pred]
    flip = rng.random((H, W)) < noise
    plab[flip] = rng.integers(0, ins_num, size=int(flip.sum()))
    pred = pred_from_labels(rng, plab, ins_num, levels=levels, ties=ties)
    gt_ins, gt_num, mask = gt_onehot(gt, ins_num, crop)
    if mask_ones:
        mask = torch.ones(H, W)
    if mask_zeros:
        mask = torch.zeros(H, W)
    return pred, gt_ins, gt_num, mask


def main():
    rng = np.random.default_rng(20261016)
    specs = {
        "c13": dict(ins_num=13, H=24, W=32, n_gt=10, shift=(0, 0), noise=0.02),
        "c59": dict(ins_num=59, H=32, W=48, n_gt=20, noise=0.06),
        "c93": dict(ins_num=93, H=48, W=64, n_gt=60, block=6, shift=(0, 0), noise=0.04),
        "crop59": dict(ins_num=59, H=32, W=40, n_gt=30, crop=True),
        "mask_ones13": dict(ins_num=13, H=24, W=32, n_gt=8, mask_ones=True, block=6),
        "tied13": dict(ins_num=13, H=24, W=32, n_gt=10, levels=(0.5, 0.625, 0.75)),
        "tied59": dict(ins_num=59, H=32, W=48, n_gt=14, levels=(0.5, 0.75), shift=(0, 0)),
        "few_pred13": dict(ins_num=13, H=24, W=32, n_gt=10, n_pred=3, noise=0.0),
        "few_pred_crop59": dict(ins_num=59, H=32, W=40, n_gt=20, n_pred=5, crop=True, noise=0.0),
        "v0_single13": dict(ins_num=13, H=16, W=16, n_gt=4, n_pred=1, mask_ones=True, noise=0.0, ties=0.0),
        "v0_masked13": dict(ins_num=13, H=16, W=16, n_gt=4, mask_zeros=True),
        "small_even_odd13": dict(ins_num=13, H=8, W=12, n_gt=6, block=3, noise=0.1),
    }
    arrays = {"cases": np.array(list(specs))}
    for name, spec in specs.items():
        pred, gt_ins, gt_num, mask = case(rng, **spec)
        ins_num = spec["ins_num"]
        p = torch.from_numpy(pred)
        plab, pconf = RS.label_conf(pred)
        rows = RS.gt_rows_from_onehot(gt_ins.numpy(), gt_num)
        try:
            label, ap, ret = R_eval.ins_eval(p.clone(), gt_ins.clone(), gt_num, ins_num, None if mask is None else mask.clone())
            raises = False
        except IndexError:
            # no valid predicted label: the reference indexes an empty label list (:172) and raises; what is stored is the
            # restatement's answer for it (every row unmatched: labels -1, all six APs 0)
            raises = True
            label, ap, ret = RS.ins_eval(plab, pconf, rows, gt_num, ins_num, None if mask is None else mask.numpy())
            assert (ret == -1).all() and not any(ap), name
            label = torch.from_numpy(label.reshape(pred.shape[:2]))
        label = label.numpy().astype(np.int64)
        ap = np.asarray(ap, dtype=np.float64)
        ret = np.asarray(ret, dtype=np.int64)
        # the restatement reproduces the reference exactly (a case whose assignment a last-bit difference of cost_ce -- ATen's
        # summation order -- flips would stop here)
        r_label, r_ap, r_ret, det = RS.ins_eval(plab, pconf, rows, gt_num, ins_num, None if mask is None else mask.numpy(), details=True)
        assert np.array_equal(r_label.reshape(label.shape), label), name
        assert np.array_equal(np.asarray(r_ap), ap), (name, r_ap, ap)
        assert np.array_equal(r_ret, ret), (name, r_ret, ret)
        counts = np.bincount(r_label, minlength=ins_num + 1)[:ins_num]
        print(f"{name}: ins_num {ins_num}, {pred.shape[0]}x{pred.shape[1]}, gt_num {gt_num}, valid labels "
              f"{int((counts > 0).sum())} ({int(((counts > 0) & (counts % 2 == 0)).sum())} even counts), ap {np.round(ap, 4).tolist()}")
        arrays[name + "/pred_ins"] = pred
        arrays[name + "/gt_ins"] = gt_ins.numpy().astype(np.uint8)
        arrays[name + "/gt_num"] = np.int64(gt_num)
        arrays[name + "/ins_num"] = np.int64(ins_num)
        arrays[name + "/mask"] = (np.zeros(0, np.float32) if mask is None else mask.numpy().astype(np.float32))
        arrays[name + "/has_mask"] = np.int64(mask is not None)
        arrays[name + "/pred_label"] = label
        arrays[name + "/ap"] = ap
        arrays[name + "/return_labels"] = ret
        arrays[name + "/reference_raises"] = np.int64(raises)
    # torch.argsort(descending=True) on the CPU keeps tied entries in index order for up to 16 entries (calculate_ap's ordering,
    # :104); from 17 entries on its order among ties is its sort's own, so the cases with tied medians have at most 16 gt rows
    for n in (2, 6, 11, 16):
        for seed in range(20):
            c = torch.from_numpy(np.random.default_rng(seed).choice(np.float32([0.0, 0.5, 0.75, 0.9]), size=n))
            assert torch.equal(torch.argsort(c, descending=True), torch.from_numpy(np.argsort(-c.numpy(), kind="stable"))), (n, seed)
    path = os.path.join(OUT, "ins_eval.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
