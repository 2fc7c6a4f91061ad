"""The float64 restatement of the object-code loss (tests/_criterion_restate.py) that tests/test_gpu_criterion_edges.py compares
csrc/criterion.hip against, held on the CPU to the committed fixtures of the reference and to the oracle (oracle/ref_cpu.py); then,
for every case the GPU test runs: the margin condition that makes "the same assignment as scipy" a fair demand, margin 0 on the
tied cases, the decoding of an assignment from a gradient, and the oracle's own float32 error against float64 -- the yardstick of
the GPU test's tolerance.

Bounds used here.  A mean of N float32 terms summed pairwise is within (log2 N + 3) 2^-24 of the terms' scale of the float64 mean
(log2 N roundings of the tree, one of each logarithm, one of the division, one to spare): the reference's cost entries and its four
outputs are held to that, relative to the largest entry of the matrix (outputs: to the loss, and to 1 at least: a soft-IoU cost is formed as 1 - ratio).  The fixtures' gradient is held
element by element to ``f32_grad_ulps``; the oracle's on the generated cases (whose saturated entries are not well conditioned) to
2e-5 of its largest entry, and its exact error is what the GPU file's rule is built from."""
import math

import numpy as np
import pytest
import torch

import _criterion_restate as CR
from oracle import ref_cpu as O

UNTIED = CR.case_names(lambda c: not c.tied)
TIED = CR.case_names(lambda c: c.tied)
ORACLE = CR.case_names(CR.oracle_runs)


def f32_sum_bound(N, scale):
    return (math.log2(max(N, 2)) + 3) * 2.0 ** -24 * scale


def f32_grad_ulps(N):
    """An element of the float32 gradient is a cross-entropy term (a sum, two divisions: 1.5 ulp) plus a soft-IoU term TP / D^2 / V
    or 1 / D / V, whose TP and D are pairwise float32 sums of N terms ((log2 N + 3) / 2 ulp each, D twice) with three more
    roundings, and one for the sum of the two: 1.5 (log2 N + 3) + 5.5 ulp, against the elementwise scale of compare_grad."""
    return 1.5 * (math.log2(max(N, 2)) + 3) + 5.5


def grad_ulps(want, got):
    """Largest elementwise |got - want| in float32 ulp of max(|want_e|, 1e-3 median |want| of the column) (compare_grad's scale)."""
    want, got = want.double(), got.double()
    scale = torch.maximum(want.abs(), 1e-3 * want.abs().median(0).values[None, :])
    return float(((got - want).abs() / CR.ulp32(scale)).max())


@pytest.mark.parametrize("name", ["all", "some", "wide"])
def test_fixture(golden, name):
    g = golden("ins_criterion")
    C = int(g[f"{name}_ins_num"])
    pred, lab = g[f"{name}_pred"], g[f"{name}_lab"].numpy()
    N = pred.shape[0]
    ce, siou, rows = CR.cost_matrices64(pred, lab, C)
    V = len(rows)
    gce, gsi = g[f"{name}_cost_ce"].double().numpy(), g[f"{name}_cost_siou"].double().numpy()
    assert gce.shape[0] == V and np.array_equal(rows, np.unique(lab))
    assert np.abs(ce - gce[:V]).max() <= f32_sum_bound(N, np.abs(ce).max()), (name, np.abs(ce - gce[:V]).max())
    assert np.abs(siou - gsi[:V]).max() <= f32_sum_bound(N, 1.0), (name, np.abs(siou - gsi[:V]).max())
    cols = g[f"{name}_cols"].numpy()
    ref_cols = CR.linear_sum_assignment(ce + siou)[1]
    assert np.array_equal(ref_cols, cols[:V]), name
    assert CR.assignment_margin(ce + siou, ref_cols) >= CR.margin_bound(ce + siou)
    out, (grad,) = CR.evaluate64(pred, lab, C, ref_cols, gouts=(CR.WEIGHTS[0],))
    want = g[f"{name}_out"].double().reshape(-1)
    assert float((out - want).abs().max()) <= f32_sum_bound(N, max(1.0, float(out[0]))), (name, out.tolist(), want.tolist())
    gw = g[f"{name}_grad"].double()
    ulps = grad_ulps(grad, gw)
    print(f"{name}: the reference's float32 gradient is within {ulps:.2f} ulp of the float64 one, element by element")
    assert ulps <= f32_grad_ulps(N), (name, ulps, f32_grad_ulps(N))
    assert np.array_equal(CR.decode_assignment(g[f"{name}_grad"], lab), ref_cols), name
    y_out, (y_grad,) = CR.evaluate32(pred, lab, C, ref_cols, gouts=(CR.WEIGHTS[0],))
    assert float((y_out - want).abs().max()) <= 4 * 2.0 ** -24 * max(1.0, float(out[0])), (name, "float32 yardstick vs the reference's floats")
    assert grad_ulps(grad, y_grad) <= f32_grad_ulps(N), name


@pytest.mark.parametrize("name", ORACLE)
def test_restatement_reproduces_oracle(name):
    """Outputs and gradients for every weight vector, at scipy's assignment on the float64 cost; the assignment is decoded from the
    oracle's gradient; the oracle's float32 error is recorded (the GPU file recomputes it); the float32 yardstick that stands in for
    the oracle elsewhere is as close to float64 as the oracle is."""
    c, ref = CR.case(name), CR.reference(name)
    o_out, o_grads, o_cols = CR._oracle_of(name, O)
    if not c.tied:
        assert np.array_equal(o_cols, ref.cols), (name, "decode_assignment(oracle gradient) != scipy on the float64 cost")
    else:
        assert abs(float(ref.cost[np.arange(ref.V), o_cols].sum()) - ref.total) <= ref.bound
    want_out, want_grads = CR.evaluate64(c.pred, c.labels.numpy(), c.C, o_cols)
    y_out, y_grads = CR.evaluate32(c.pred, c.labels.numpy(), c.C, o_cols)
    assert bool(torch.isfinite(want_out).all()) and bool(torch.isfinite(o_out).all())
    err_o, err_y = (o_out - want_out).abs(), (y_out - want_out).abs()
    bound = f32_sum_bound(c.N, max(1.0, float(want_out[0])))
    assert float(err_o.max()) <= bound and float(err_y.max()) <= bound, (name, err_o.tolist(), err_y.tolist(), bound)
    if ref.U == 0:
        assert float(o_out[2]) == 0.0 == float(want_out[2]) == float(y_out[2])
    worst = 0.0
    for w, wg, og, yg in zip(CR.WEIGHTS, want_grads, o_grads, y_grads):
        assert bool(torch.isfinite(wg).all()) and bool(torch.isfinite(og).all()), (name, w)
        scale = float(wg.abs().max())
        e_o, e_y = float((og - wg).abs().max()), float((yg - wg).abs().max())
        assert e_o <= 2e-5 * scale and e_y <= 2e-5 * scale, (name, w, e_o, e_y, scale)
        assert bool((og[wg == 0] == 0).all()) and bool((yg[wg == 0] == 0).all()), (name, w, "exact zeros")
        worst = max(worst, e_o / scale) if scale > 0 else worst
    print(f"{name}: oracle float32 error " + ", ".join(f"{n} {float(e):.2e}" for n, e in zip(CR.OUT, err_o))
          + f"; gradient {worst:.2e} of its largest entry; yardstick " + ", ".join(f"{float(e):.2e}" for e in err_y))


@pytest.mark.parametrize("name", UNTIED)
def test_margin_condition(name):
    """A condition on the generator, not a measurement: scipy's assignment on the float64 cost is the unique optimum by at least
    8 V 2^-23 max|cost|, so a solver that sees every entry within 4 float32 ulp of it has no other optimum."""
    ref = CR.reference(name)
    m = CR.margin(name)
    print(f"{name}: V {ref.V}, U {ref.U}, margin {m:.3e}, bound {ref.bound:.3e}")
    assert m >= ref.bound, (name, m, ref.bound)
    c = CR.case(name)
    if c.family in ("trained", "converged", "saturated") and ref.V > 1:
        assert not np.array_equal(ref.cols, np.arange(ref.V)), (name, "the assignment was meant not to be the identity")


@pytest.mark.parametrize("name", TIED)
def test_tied_cases_are_tied(name):
    ref = CR.reference(name)
    assert CR.margin(name) <= 1e-12 * ref.total, (name, CR.margin(name))
    if CR.case(name).identity:
        assert np.array_equal(ref.cols, np.arange(ref.V)), name
        assert float(np.abs(ref.cost - ref.cost[:, :1]).max()) == 0.0, (name, "every row is one constant")


def test_bad_label_semantics():
    """The stated semantics on the three cases the reference raises on: which rows form, and that out-of-range rays still count in
    N, in the per-channel sums and in invalid_ce."""
    c = CR.case("bad_range")
    lab = c.labels.numpy()
    assert lab[17] == -1 and lab[64] == c.C + 1
    assert CR.rows_of(lab, c.C).tolist() == [0, 1, 3, 5]
    ce, siou, rows = CR.cost_matrices64(c.pred, lab, c.C)
    keep = (lab >= 0) & (lab <= c.C)
    P = c.pred.double().numpy()
    lb = np.log(((1 - c.pred) + 1e-8).double().numpy())
    la = np.log((c.pred + 1e-8).double().numpy())
    own = lab == 3
    assert abs(ce[2, 1] - (-(la[own, 1].sum()) - lb[~own, 1].sum()) / c.N) <= 1e-14       # the two bad rays are "other" rays of every row
    TP = P[own, 1].sum()
    assert abs(siou[2, 1] - (1 - TP / (P[:, 1].sum() + own.sum() - TP + 1e-6))) <= 1e-14
    assert (~keep).sum() == 2
    ref = CR.reference("bad_range")
    out, _ = CR.evaluate64(c.pred, lab, c.C, ref.cols)
    un = sorted(set(range(c.C)) - set(ref.cols.tolist()))
    assert abs(float(out[2]) - P[:, un].mean()) <= 1e-15
    c = CR.case("bad_many")
    assert sorted(set(c.labels.tolist())) == list(range(c.C + 1)) and CR.reference("bad_many").rows.tolist() == list(range(c.C))
    c = CR.case("bad_none")
    ref = CR.reference("bad_none")
    assert ref.V == 0 and ref.U == c.C
    out, grads = CR.evaluate64(c.pred, c.labels.numpy(), c.C, ref.cols)
    assert float(out[1]) == 0.0 == float(out[3]) and abs(float(out[2]) - float(c.pred.double().mean())) <= 1e-15
    assert bool((grads[0] == 1.0 / (c.N * c.C)).all())
    with pytest.raises(Exception):
        O.ins_criterion(c.pred, c.labels, c.C)
    with pytest.raises(Exception):
        O.ins_criterion(CR.case("bad_many").pred, CR.case("bad_many").labels, 5)


def test_decode_refuses_what_is_not_an_assignment():
    c = CR.case("trained_64_13_V9")
    _, grads, cols = CR._oracle_of(c.name, O)
    lab = c.labels.numpy()
    assert np.array_equal(CR.decode_assignment(grads[0], lab), cols)
    for spoil in ("sign", "constant", "double"):
        g = grads[0].clone()
        un = sorted(set(range(c.C)) - set(cols.tolist()))
        if spoil == "sign":                                     # one ray of another label turns negative
            n = int(np.nonzero(lab != CR.rows_of(lab, c.C)[0])[0][0])
            g[n, cols[0]] = -g[n, cols[0]].abs()
        elif spoil == "constant":                               # an unmatched channel is no longer one value
            g[3, un[0]] = g[3, un[0]] * (1 + 2.0 ** -20)
        else:                                                   # two channels claim one label
            g[:, un[0]] = g[:, cols[0]]
        with pytest.raises(AssertionError):
            CR.decode_assignment(g, lab)


def test_planted_values_are_where_the_case_says():
    """The saturated family under each case's own assignment: every existing chunk kind (first, last full, ragged) of every case
    holds planted values on a matched channel's own ray, on another ray of a matched channel and (U > 0) on an unmatched channel;
    over the family each of the four values occurs in each of the three places, and each place in each chunk kind."""
    seen = set()
    for name in CR.case_names(lambda c: c.family == "saturated"):
        need = {"own", "other", "unmatched"} if CR.reference(name).U else {"own", "other"}
        for where, spots in CR.planted_census(name).items():
            assert {place for place, _ in spots} >= need, (name, where, sorted(spots))
            seen |= {(where, place, v) for place, v in spots}
    # planting 0 on a label's own ray costs that pair 18.4 / N: scipy may then move the label, so not every (chunk, place, value)
    # triple survives under the final assignment; every (place, value) and every (chunk, place) pair does
    places = ("own", "other", "unmatched")
    assert {(k, v) for _, k, v in seen} == {(k, v) for k in places for v in CR.PLANTED}, sorted(seen)
    assert {(w, k) for w, k, _ in seen} == {(w, k) for w in ("first", "last full", "ragged") for k in places}, sorted(seen)
