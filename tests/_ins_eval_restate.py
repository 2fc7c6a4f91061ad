"""Count-based restatement of ``ins_eval`` / ``calculate_ap`` (networks/evaluator.py:77-175) in numpy + scipy.

The reference builds one-hot predictions and broadcasts them against the one-hot ground truth into ``[ins_num, ins_num, H*W]``
tensors.  With 0/1 inputs every quantity it forms is a function of three integer counts per (row, channel) pair -- the row's
pixel count, the channel's pixel count and their overlap -- so this module computes the confusion matrix with ``np.bincount``
and evaluates the reference's formulas on it in the reference's f32 order.  ``tests/test_ins_eval_restate.py`` proves it
reproduces the reference's own outputs on the committed fixtures (``tests/golden/ins_eval.npz``); the GPU tests then use it on
frames too large for the reference.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

F32 = np.float32
THRESHOLDS = (0.5, 0.75, 0.8, 0.85, 0.9, 0.95)          # evaluator.py:10
CE_UNIT = np.frombuffer(bytes.fromhex("8e5d9341"), dtype=F32)[0]   # -log(f32(1e-8)) in torch f32 = 18.420681


def label_conf(pred_ins):
    """argmax (first maximum) and max over the last axis of ``pred_ins [..., C]`` (evaluator.py:127-137)."""
    x = np.asarray(pred_ins, dtype=F32)
    return x.argmax(-1).astype(np.int64), x.max(-1).astype(F32)


def gt_rows_from_onehot(gt_ins, gt_num):
    """Per-pixel ground-truth row of a one-hot ``gt_ins [..., C]`` (columns < gt_num), -1 where the pixel has none."""
    g = np.asarray(gt_ins).reshape(-1, np.asarray(gt_ins).shape[-1])[:, :gt_num]
    row = np.full(g.shape[0], -1, dtype=np.int64)
    hit = g.sum(1) > 0
    row[hit] = g[hit].argmax(1)
    return row


def ata_sum_f32(x):
    """``torch.sum`` of a short contiguous f32 vector on the CPU, in ATen's order: 8-lane vectors summed by four accumulators
    (``row_sum`` with ilp 4), the scalar tail first, then the lanes; below 8 elements four scalar accumulators.  The device's
    AP integral adds its terms in this order."""
    x = np.asarray(x, dtype=F32)
    n = len(x)

    def four_acc(vals):                                 # vals: 8-lane vectors or scalars; four accumulators, stride 4
        acc = [vals[0] * F32(0) for _ in range(4)]
        m = len(vals)
        for i in range(m // 4):
            for k in range(4):
                acc[k] = (acc[k] + vals[4 * i + k]).astype(F32)
        for i in range((m // 4) * 4, m):
            acc[0] = (acc[0] + vals[i]).astype(F32)
        for k in range(1, 4):
            acc[0] = (acc[0] + acc[k]).astype(F32)
        return acc[0]

    if n == 0:
        return F32(0)
    if n < 8:
        return F32(four_acc([F32(v) for v in x]))
    nv = n // 8
    lanes = four_acc([x[8 * m:8 * m + 8].copy() for m in range(nv)])
    s = F32(0)
    for k in range(nv * 8, n):
        s = F32(s + x[k])
    for v in lanes:
        s = F32(s + v)
    return s


def calculate_ap(ious, gt_number, confidence):
    """``calculate_ap(..., confidence, 'integral')`` (evaluator.py:77-122): six APs as Python floats."""
    ious = np.asarray(ious, dtype=F32)
    order = np.argsort(-np.asarray(confidence, dtype=F32), kind="stable")      # torch.argsort(descending): ties in index order
    v = ious[order]
    n = len(v)
    out = []
    for t in THRESHOLDS:
        cum = np.cumsum(v > F32(t)).astype(np.int64)
        prec = (cum.astype(F32) / np.arange(1, n + 1).astype(F32)).astype(F32)
        rec = (cum.astype(F32) / F32(gt_number)).astype(F32) if n else np.zeros(0, F32)
        mrec = np.concatenate([[F32(0)], rec, [F32(1)]]).astype(F32)
        mprec = np.concatenate([[F32(0)], prec, [F32(0)]]).astype(F32)
        for i in range(len(mprec) - 1, 0, -1):
            mprec[i - 1] = max(mprec[i - 1], mprec[i])
        idx = np.nonzero(mrec[1:] != mrec[:-1])[0]
        terms = ((mrec[idx + 1] - mrec[idx]).astype(F32) * mprec[idx + 1]).astype(F32)
        out.append(float(ata_sum_f32(terms)))
    return out


def ins_eval(pred_label, conf, gt_row, gt_num, ins_num, mask=None, details=False):
    """``ins_eval`` (evaluator.py:125-175) from per-pixel ``pred_label`` (argmax), ``conf`` (max over all channels) and
    ``gt_row`` (-1 = no row).  Returns ``(pred_label with the mask rule, ap [6], return_labels [gt_num])``; with
    ``details=True`` also a dict of the intermediates (valid labels, medians, cost matrix, assignment)."""
    lab = np.asarray(pred_label, dtype=np.int64).reshape(-1).copy()
    conf = np.asarray(conf, dtype=F32).reshape(-1)
    gt_row = np.asarray(gt_row, dtype=np.int64).reshape(-1)
    N, C = lab.shape[0], int(ins_num)
    if mask is not None:
        lab[np.asarray(mask).reshape(-1) == 0] = C
        valid = np.unique(lab)[:-1]                      # drops the LARGEST value, masked or not (:133)
    else:
        valid = np.unique(lab)
    V = len(valid)
    medians = np.array([np.median(conf[lab == l]) for l in valid], dtype=F32)
    cnt = np.bincount(lab, minlength=C + 1)
    has = gt_row >= 0
    joint = np.bincount(gt_row[has] * (C + 1) + lab[has], minlength=gt_num * (C + 1)).reshape(gt_num, C + 1)
    n_g = joint.sum(1)
    TP = np.zeros((gt_num, C), dtype=np.int64)
    n_p = np.zeros(C, dtype=np.int64)
    TP[:, :V] = joint[:, valid]
    n_p[:V] = cnt[valid]
    # cost_ce: every term of the mean is 0 or CE_UNIT, so the entry is CE_UNIT * (pixels where the two one-hots differ) / N
    ce = (np.float64(CE_UNIT) * (n_g[:, None] + n_p[None, :] - 2 * TP) / N).astype(F32)
    tpf = TP.astype(F32)
    fp = (n_p[None, :].astype(F32) - tpf).astype(F32)
    fn = (n_g[:, None].astype(F32) - tpf).astype(F32)
    den = ((((tpf + fp).astype(F32) + fn).astype(F32)) + F32(1e-6)).astype(F32)
    siou = (F32(1.0) - (tpf / den).astype(F32)).astype(F32)
    cost = (ce + siou).astype(F32)
    _, cols = linear_sum_assignment(cost)
    ious = (F32(1.0) - siou[np.arange(gt_num), cols]).astype(F32)
    confidence = np.zeros(gt_num, dtype=F32)
    inv = cols >= V
    confidence[~inv] = medians[cols[~inv]]
    ap = calculate_ap(ious, gt_num, confidence)
    ret = np.full(gt_num, -1, dtype=np.int64)
    ret[~inv] = valid[cols[~inv]]
    if not details:
        return lab, ap, ret
    return lab, ap, ret, dict(valid=valid, medians=medians, cost=cost, cols=cols, ious=ious, confidence=confidence)


def assignment_margin(cost, cols):
    """Smallest increase of the optimal total when one chosen pair of ``cols`` (row i -> cols[i]) is forbidden: the margin by
    which the optimum is unique (0 for a tie; inf when no alternative exists)."""
    c = np.asarray(cost, dtype=np.float64)
    best = c[np.arange(len(cols)), cols].sum()
    margin = np.inf
    for i, j in enumerate(cols):
        c2 = c.copy()
        c2[i, j] = 1e30
        r2, k2 = linear_sum_assignment(c2)
        alt = c2[r2, k2].sum()
        if alt < 1e29:
            margin = min(margin, alt - best)
    return margin


def load_fixtures():
    """``tests/golden/ins_eval.npz`` as {case: {key: numpy array}} (scalars as 0-d arrays), in the order it was written."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ins_eval.npz")
    with np.load(path) as z:
        cases = [str(c) for c in z["cases"]]
        return {c: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(c + "/")} for c in cases}
