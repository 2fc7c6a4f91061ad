"""GPU tests (-m gpu) of the object-code loss of csrc/criterion.hip (with the assignment solver of csrc/lsa_wave.h) against the
float64 restatement of tests/_criterion_restate.py, at the shape and value edges of its four kernels.

Cases (generated in tests/_criterion_restate.py; tests/test_criterion_restate.py holds the same tensors to the float32 oracle and
to the margin condition on the CPU): N in {1, 63, 64, 65, 129, 1025} -- a ragged only chunk, a ragged last chunk, 17 chunks for the
16 lanes per entry of the chunk sum -- x C in {1, 2, 5, 13, 63, 64, 65, 127, 128} with V = C, V = C - 1 and V < C on both sides of
the solver's second column (C > 64) and second row (V > 64) per lane, label value ins_num among the rows; predictions of a trained
field, of a converged one (logits +-7: the cross-entropy sums nearly cancel) and with 0, 1, 1 - 2^-24 and 2^-30 planted in the
first, the last full and the ragged chunk; labels the reference raises on; tied costs (all predictions 0.5, one channel copied bit
for bit into another); five upstream weight vectors.  Every case goes through ``E.ins_criterion`` and autograd.

Checked per case: the assignment, decoded from the gradient of out[0], equals scipy's on the float64 cost (tied cases: injective,
covers every row, float64 total within the margin-condition bound of the optimum; identity where every row is constant); the four
outputs and every element of the gradient for every weight vector against float64 AT THE KERNEL'S OWN ASSIGNMENT, within 4 x the
float32 oracle's error + 8 float32 ulp (the rule of tests/_criterion_restate.py; no ray or channel left out); unmatched columns one
bit-identical constant; exact zeros kept; ``invalid_ce`` exactly 0 when every channel is matched.

OBSERVED on an MI355X, per case family (the module prints these figures when it finishes): the largest kernel error in float32
ulp of the scale, and the largest multiple of the oracle's error that an output / an element needed on top of the 8 ulp (the rule
allows 4).
  trained      values 12.4 ulp, 0.36 x      gradient 6.2 ulp, within the 8 ulp alone
  converged    values 962 ulp, 3.00 x       gradient 6.3 ulp, within the 8 ulp alone
  saturated    values 2.0 ulp               gradient 5.2 ulp
  bad labels   values 1.2 ulp               gradient 6.1 ulp
  tied         values 0.8 ulp               gradient 3.8 ulp
Every case passes.  The large figures are all ``valid_siou``, which the reference and the kernel both form in float32 as 1 - ratio:
near convergence the result is ~1e-3 and carries the rounding of 1 (converged_63_2_l02: 1.12e-7 on 1.85e-3 where the oracle is 3.7e-8
off, the 3.00 x; converged_1_1_l0: 4.54e-8 on 9.6e-4, the oracle's own error to three digits).  ``valid_ce`` is within 4.2e-11 of
float64 on the converged cases (the oracle: 1.7e-11 ... 4.2e-11), ``invalid_ce`` within 1 ulp everywhere.
BEFORE csrc/criterion.hip was changed (same shapes and families, earlier seeds), 14 of the 47 cases failed, 12 of them on ``valid_ce`` (every converged case below N = 1025
that reached the comparison, and the one-ray case trained_1_1_l0): converged values 11176 ulp, 382792 x the oracle's error (e.g.
converged_63_2_l02: valid_ce 9.1080e-4 against 9.1015e-4, the oracle 1.7e-12 away); trained values 86 ulp (one ray, 8.0e-8 on
1.06e-2).  Cause: a cross-entropy entry was (A_p + b_lp) / N, A_p the float32 chunk sums of -log(1-P) over ALL rays and b_lp
taking the label's own rays back out -- on a converged channel the two cancel.  The entry is now [other labels' rays] + [own rays],
each a sum of like-sized terms, combined in float64.  Two converged cases (129_63_V63, 129_65_V65) failed on the gradient instead:
whole matched columns 16.5 ulp off where the oracle is 0.6 ulp off; cause: the per-channel sum of P over a chunk added 0.001s onto
a partial sum near 1 in float32, in ray order; it is accumulated in float64 now.  Everything else -- assignments at C, V > 64, ties,
ragged chunks, label ins_num, bad labels, the work buffer, the two-level entry -- passed unchanged.
"""

import numpy as np
import pytest
import torch

import _criterion_restate as CR
import _gpu
from _gpu import cpu
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

STATS = {}


@pytest.fixture(scope="module")
def A():
    yield _gpu.namespace()
    for fam, st in STATS.items():
        print(f"\n[criterion edges] {fam}: largest error {st.get('ulps', 0.0):.2f} ulp of the scale, needs {st.get('ratio', 0.0):.2f} x the oracle's error + 8 ulp")


def stats(family, what):
    return STATS.setdefault(f"{family}, {what}", {})


def _run(A, c, check=None):
    """The four outputs and d(w . outputs) / d pred for every weight vector of CR.WEIGHTS, through autograd."""
    outs, grads = [], []
    lab = c.labels.cuda()
    for w in CR.WEIGHTS:
        pred = c.pred.cuda().requires_grad_(True)
        out = torch.stack(A.E.ins_criterion(pred, lab, c.C, check=check))
        g, = torch.autograd.grad((out * torch.tensor(w, dtype=torch.float32, device="cuda")).sum(), pred)
        outs.append(cpu(out))
        grads.append(cpu(g))
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), (c.name, "the outputs changed from one call to the next")
    return outs[0], grads


def _check_case(A, c):
    ref = CR.reference(c.name)
    out, grads = _run(A, c)
    labels = c.labels.numpy()
    # the assignment
    cols = CR.decode_assignment(grads[0], labels)
    if not c.tied:
        assert np.array_equal(cols, ref.cols), (c.name, "assignment differs from scipy's on the float64 cost", cols.tolist(), ref.cols.tolist())
    else:
        assert len(set(cols.tolist())) == ref.V == len(cols), (c.name, cols.tolist())
        total = float(ref.cost[np.arange(ref.V), cols].sum())
        print(f"{c.name}: total {total:.9e}, optimum {ref.total:.9e}, bound {ref.bound:.2e}")
        assert total - ref.total <= ref.bound, (c.name, total, ref.total, ref.bound)
        if c.identity:
            assert np.array_equal(cols, np.arange(ref.V)) and np.array_equal(cols, ref.cols), (c.name, cols.tolist())
    # values and gradients at the kernel's own assignment
    want_out, want_grads, o_out, o_grads, which = CR.yardsticks(c.name, cols, O)
    CR.compare_values(out, want_out, o_out, f"{c.name} [{which}]", stats(c.family, "values"))
    if ref.U == 0:
        assert float(out[2]) == 0.0, (c.name, "invalid_ce with every channel matched", float(out[2]))
    un = sorted(set(range(c.C)) - set(cols.tolist()))
    for w, g, wg, og in zip(CR.WEIGHTS, grads, want_grads, o_grads):
        assert g.shape == (c.N, c.C)
        CR.compare_grad(g, wg, og, f"{c.name} w={w}", stats(c.family, "gradient"))
        if un:
            assert bool((g[:, un] == g[0, un[0]]).all()), (c.name, w, "unmatched columns are not one constant")
    st = stats(c.family, "gradient")
    print(f"{c.name}: gradient so far {st['ulps']:.2f} ulp, {st['ratio']:.2f} x the oracle's error + 8 ulp")


@pytest.mark.parametrize("name", CR.case_names())
def test_case_vs_float64(A, name):
    _check_case(A, CR.case(name))


def test_label_flags(A):
    """``check=True`` raises on the two conditions the reference raises on and on nothing else (values and gradients of the same
    cases without ``check``: test_case_vs_float64 under the stated semantics)."""
    for name in ("trained_65_13_V13hi", "trained_1025_128_V65", "tied_half_65_13_V13"):        # ins_num itself is a label: clean
        c = CR.case(name)
        out = A.E.ins_criterion(c.pred.cuda(), c.labels.cuda(), c.C, check=True)
        assert bool(torch.isfinite(out[0]))
    for name, match in (("bad_range", "outside"), ("bad_none", "outside"), ("bad_many", "distinct labels")):
        c = CR.case(name)
        with pytest.raises(ValueError, match=match):
            A.E.ins_criterion(c.pred.cuda(), c.labels.cuda(), c.C, check=True)


def _raw(A, cs, fill, gouts):
    """The C entry points on one or two predictions (the *2 entries for two) with work buffers pre-filled with ``fill``."""
    L = A.L
    lib = L.load()
    N, C = cs[0].N, cs[0].C
    nbytes = lib.dmnerf_ins_criterion_work_bytes(N, C)
    assert nbytes > 0
    lab = cs[0].labels.to(torch.int32).cuda()
    pred = [c.pred.cuda() for c in cs]
    work = [torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda") for _ in cs]
    out = [torch.full((4,), float("nan"), device="cuda") for _ in cs]
    grad = [torch.full_like(p, float("nan")) for p in pred]
    g = [torch.tensor(w, dtype=torch.float32, device="cuda") for w in gouts]
    if len(cs) == 1:
        L.check(lib.dmnerf_ins_criterion_fwd(L.ptr(pred[0]), L.ptr(lab), N, C, L.ptr(work[0]), nbytes, L.ptr(out[0]), L.stream()), "dmnerf_ins_criterion_fwd")
        L.check(lib.dmnerf_ins_criterion_bwd(L.ptr(pred[0]), L.ptr(lab), N, C, L.ptr(work[0]), L.ptr(g[0]), L.ptr(grad[0]), L.stream()), "dmnerf_ins_criterion_bwd")
    else:
        L.check(lib.dmnerf_ins_criterion_fwd2(L.ptr(pred[0]), L.ptr(pred[1]), L.ptr(lab), N, C, L.ptr(work[0]), L.ptr(work[1]), nbytes,
                                              L.ptr(out[0]), L.ptr(out[1]), L.stream()), "dmnerf_ins_criterion_fwd2")
        L.check(lib.dmnerf_ins_criterion_bwd2(L.ptr(pred[0]), L.ptr(pred[1]), L.ptr(lab), N, C, L.ptr(work[0]), L.ptr(work[1]), L.ptr(g[0]), L.ptr(g[1]),
                                              L.ptr(grad[0]), L.ptr(grad[1]), L.stream()), "dmnerf_ins_criterion_bwd2")
    return [cpu(o) for o in out], [cpu(x) for x in grad]


@pytest.mark.parametrize("name", ["saturated_65_13_V13lo", "trained_65_13_V13hi", "trained_1025_128_V65", "bad_range"])
def test_work_buffer_is_written_before_it_is_read(A, name):
    """The kernels clear nothing and claim to write everything they read: a work buffer of 0xFF bytes (NaNs, -1) and one of zeros
    give the same bits."""
    c = CR.case(name)
    w = CR.WEIGHTS[4]
    out_f, grad_f = _raw(A, [c], 0xFF, [w])
    out_z, grad_z = _raw(A, [c], 0, [w])
    assert bool(torch.isfinite(out_f[0]).all()) and bool(torch.isfinite(grad_f[0]).all()), name
    assert torch.equal(out_f[0], out_z[0]) and torch.equal(grad_f[0], grad_z[0]), name
    # and they are the floats autograd returns
    pred = c.pred.cuda().requires_grad_(True)
    out = torch.stack(A.E.ins_criterion(pred, c.labels.cuda(), c.C))
    g, = torch.autograd.grad((out * torch.tensor(w, dtype=torch.float32, device="cuda")).sum(), pred)
    assert torch.equal(cpu(out), out_f[0]) and torch.equal(cpu(g), grad_f[0]), name


def test_two_levels_per_launch_equal_two_calls(A):
    """dmnerf_ins_criterion_fwd2 / _bwd2 at (65, 128) on two predictions whose assignments differ, with different upstream
    weights: bit for bit the two single-level calls."""
    a, b = CR.two_level_case()
    wa, wb = CR.WEIGHTS[4], CR.WEIGHTS[0]
    out2, grad2 = _raw(A, [a, b], 0xFF, [wa, wb])
    for c, w, o, g in ((a, wa, out2[0], grad2[0]), (b, wb, out2[1], grad2[1])):
        o1, g1 = _raw(A, [c], 0xFF, [w])
        assert torch.equal(o, o1[0]) and torch.equal(g, g1[0]), c.name
    _, ga = _raw(A, [a], 0, [CR.WEIGHTS[0]])
    cols_a, cols_b = CR.decode_assignment(ga[0], a.labels.numpy()), CR.decode_assignment(grad2[1], b.labels.numpy())
    assert not np.array_equal(cols_a, cols_b), "the two levels were meant to be assigned differently"
    for c, cols in ((a, cols_a), (b, cols_b)):
        ce, siou, _ = CR.cost_matrices64(c.pred, c.labels.numpy(), c.C)
        from scipy.optimize import linear_sum_assignment
        assert np.array_equal(cols, linear_sum_assignment(ce + siou)[1]), c.name
