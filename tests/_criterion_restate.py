"""float64 restatement of the object-code loss ``ins_criterion`` (networks/evaluator.py:19-74; plain numpy / torch / scipy on the
CPU, no import from the package), the edge-case generator shared by tests/test_criterion_restate.py (CPU) and
tests/test_gpu_criterion_edges.py (GPU), and the tolerance rule of both.

WHAT IS FLOAT32 AND WHAT IS NOT.  The two logarithm arguments ``P + 1e-8`` and ``(1 - P) + 1e-8`` are formed in float32, as the
reference and the kernels both form them (at P = 1 - 2^-24 or P = 2^-30 the rounding of that sum IS the value); everything after
them is float64.  Rows of the cost matrices are the labels that occur, ascending.

STATED SEMANTICS WHERE THE REFERENCE RAISES (restated here, not read out of the kernels):
  * a ray whose label lies outside [0, C] joins no row; it still counts in N, in the per-channel sums and in ``invalid_ce``;
  * if all C + 1 labels occur the first C are kept, and the rays of label C then behave like out-of-range rays;
  * with no row at all (V = 0) ``valid_ce`` and ``valid_siou`` are 0 and every channel is unmatched.

THE ASSIGNMENT is held fixed when values and gradients are evaluated (``evaluate64``): the kernel's own assignment is decoded from
the gradient it returns (``decode_assignment``) and compared with scipy's on the float64 cost separately.  That comparison is
meaningful because every untied case keeps an assignment margin (``assignment_margin``: the cheapest total that avoids one chosen
pair, minus the optimum) of at least ``margin_bound`` = 8 V 2^-23 max|cost| -- two assignments of V entries at 4 float32 ulp each.

TOLERANCE.  Values: per output, 4 x the float32 oracle's own error on that case and output + 8 float32 ulp of
max(|want|, 1e-3 |want loss|).  Gradient: per element, 4 x the oracle's error on that element + 8 ulp of max(|want_e|, 1e-3 x the
median |want| of the column); an element that is exactly 0 in float64 must be exactly 0.  Where the oracle cannot run (labels it
raises on) or ran at another assignment (a tie it broke differently), the same formulas evaluated in float32 torch take its place
(``evaluate32``; tests/test_criterion_restate.py holds it to the oracle where both run)."""
import functools
import types

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from _ins_eval_restate import assignment_margin
from _ray_restate import ulp32

F32, F64 = torch.float32, torch.float64
OUT = ("loss", "valid_ce", "invalid_ce", "valid_siou")
WEIGHTS = ((1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.7, 1.3, -0.4, 2.0))
CHUNK = 64                                                  # rays per partial-sum workgroup of csrc/criterion.hip


# ------------------------------------------------------------------------------------------
# restatement
# ------------------------------------------------------------------------------------------
def rows_of(labels, C):
    """The labels that form the rows: those in [0, C] that occur, ascending, the first C of them."""
    lab = np.asarray(labels).reshape(-1)
    present = np.unique(lab[(lab >= 0) & (lab <= C)])
    return present[:C].astype(np.int64)


def _logs(pred, dtype):
    """(P as a leaf of ``dtype``, log(P + 1e-8), log(1 - P + 1e-8)); in float64 the two arguments are the float32 sums exactly."""
    P32 = pred.detach().to(F32)
    P = P32.to(dtype).requires_grad_(True)
    if dtype == F64:
        a32, b32 = P32 + 1e-8, (1 - P32) + 1e-8
        a = P + (a32.double() - P32.double())                # value: a32 exactly; derivative 1
        b = (1 - P) + (b32.double() - (1 - P32.double()))
    else:
        a, b = P + 1e-8, 1 - P + 1e-8
    return P, torch.log(a), torch.log(b)


def _membership(labels, rows, dtype):
    lab = torch.as_tensor(np.asarray(labels).reshape(-1)).long()
    return (lab[None, :] == torch.as_tensor(rows).long()[:, None]).to(dtype)          # [V, N]


def _costs(P, la, lb, G):
    """cost_ce, cost_siou [V, C] (evaluator.py:60-67).  float64: two matrix products; float32: the reference's broadcast."""
    N = P.shape[0]
    if P.dtype == F64:
        ce = (G @ (-la) + (1 - G) @ (-lb)) / N
        TP = G @ P
        S, cnt = P.sum(0)[None, :], G.sum(1)[:, None]
    else:
        Pm, Gm = P.permute(1, 0)[None, :, :], G[:, None, :]
        ce = torch.mean(-Gm * la.permute(1, 0)[None] - (1 - Gm) * lb.permute(1, 0)[None], dim=-1)
        TP = torch.sum(Pm * Gm, dim=-1)
        S, cnt = torch.sum(Pm, dim=-1), torch.sum(Gm, dim=-1)
    FP = S - TP
    FN = cnt - TP
    return ce, 1.0 - TP / (TP + FP + FN + 1e-6)


def cost_matrices64(pred, labels, C):
    """``(cost_ce, cost_siou, rows)``: float64 numpy ``[V, C]`` matrices and the label of each row."""
    rows = rows_of(labels, C)
    with torch.no_grad():
        P, la, lb = _logs(pred, F64)
        ce, siou = _costs(P, la, lb, _membership(labels, rows, F64))
    return ce.numpy(), siou.numpy(), rows


def _evaluate(pred, labels, C, cols, gouts, dtype):
    rows = rows_of(labels, C)
    V = len(rows)
    cols = np.asarray(cols, dtype=np.int64).reshape(-1)
    assert len(cols) == V and len(set(cols.tolist())) == V and (V == 0 or (0 <= cols.min() and cols.max() < C)), (cols, V, C)
    P, la, lb = _logs(pred, dtype)
    zero = P.sum() * 0
    if V:
        ce, siou = _costs(P, la, lb, _membership(labels, rows, dtype))
        idx = torch.arange(V)
        valid_ce, valid_siou = ce[idx, torch.from_numpy(cols)].mean(), siou[idx, torch.from_numpy(cols)].mean()
    else:
        valid_ce = valid_siou = zero
    un = sorted(set(range(C)) - set(cols.tolist()))
    invalid_ce = P[:, un].mean() if un else zero
    out = torch.stack([valid_ce + invalid_ce + valid_siou, valid_ce, invalid_ce, valid_siou])
    grads = [torch.autograd.grad((out * torch.tensor(w, dtype=dtype)).sum(), P, retain_graph=True)[0].double() for w in gouts]
    return out.detach().double(), grads


def evaluate64(pred, labels, C, cols, gouts=WEIGHTS):
    """The four outputs (float64 ``[4]``) with row g assigned to channel ``cols[g]``, and for every upstream weight vector of
    ``gouts`` d(gout4 . outputs) / d pred with that assignment held fixed (float64 autograd)."""
    return _evaluate(pred, labels, C, cols, gouts, F64)


def evaluate32(pred, labels, C, cols, gouts=WEIGHTS):
    """The float32 yardstick: the reference's formulas in float32 torch under the stated semantics, returned as float64."""
    return _evaluate(pred, labels, C, cols, gouts, F32)


def oracle_runs(case):
    """Where ``oracle.ref_cpu.ins_criterion`` computes what is stated above: no label outside [0, C], at most C distinct ones."""
    return not case.bad


def oracle32(pred, labels, C, oracle, gouts=WEIGHTS):
    """``oracle.ins_criterion`` in float32: (outputs [4], gradients per weight vector, its assignment), all float64 / int64.
    With every channel matched its ``invalid_ce`` is the integer ``tensor([0])``: value 0, no gradient."""
    p = pred.detach().to(F32).clone().requires_grad_(True)
    outs = [o.reshape(-1)[0] for o in oracle.ins_criterion(p, torch.as_tensor(np.asarray(labels)).long(), C)]
    grads = []
    for w in gouts:
        tot = sum(float(wk) * o for wk, o in zip(w, outs) if wk != 0 and o.requires_grad)
        grads.append(torch.autograd.grad(tot, p, retain_graph=True)[0].double() if torch.is_tensor(tot) else torch.zeros_like(p).double())
    cols = decode_assignment(grads[0], labels)
    return torch.tensor([float(o.detach()) for o in outs], dtype=F64), grads, cols


def decode_assignment(grad, labels):
    """The assignment behind ``grad`` = d out[0] / d pred ``[N, C]``: the channel of every row, rows in ``rows_of`` order.
    An unmatched channel is one constant positive value over all rays; a matched channel is negative on exactly the rays of one
    label and positive elsewhere; anything else fails."""
    g = grad.detach().cpu().numpy() if torch.is_tensor(grad) else np.asarray(grad)
    lab = np.asarray(labels).reshape(-1)
    N, C = g.shape
    assert lab.shape[0] == N
    rows = rows_of(lab, C)
    col_of = {}
    for p in range(C):
        col = g[:, p]
        neg = col < 0
        if not neg.any():
            assert bool((col > 0).all()) and bool((col == col[0]).all()), (p, "an unmatched channel is one constant positive value", col[:8])
            continue
        l = int(lab[neg][0])
        assert l in rows and np.array_equal(neg, lab == l), (p, l, "negative on other rays than those of one label")
        assert bool((col[~neg] > 0).all()), (p, l, "a matched channel is positive off its label's rays")
        assert l not in col_of, (p, l, "two channels matched to one label")
        col_of[l] = p
    assert sorted(col_of) == rows.tolist(), ("rows without a channel", sorted(set(rows.tolist()) - set(col_of)))
    return np.array([col_of[int(l)] for l in rows], dtype=np.int64)


def margin_bound(cost):
    """8 V 2^-23 max|cost|: two assignments of V entries, each entry 4 float32 ulp off."""
    c = np.asarray(cost, dtype=np.float64)
    return 8.0 * c.shape[0] * 2.0 ** -23 * float(np.abs(c).max()) if c.size else 0.0


# ------------------------------------------------------------------------------------------
# the tolerance rule
# ------------------------------------------------------------------------------------------
def _note(stats, err, scale, err_o):
    if stats is None:
        return
    u = ulp32(scale)
    ulps = float(torch.where(u > 0, err / u.clamp(min=1e-300), torch.zeros_like(err)).max())
    over = (err - 8 * u).clamp(min=0)
    ratio = float(torch.where(over > 0, over / err_o.clamp(min=1e-300), over).max())
    stats["ulps"] = max(stats.get("ulps", 0.0), ulps)
    stats["ratio"] = max(stats.get("ratio", 0.0), ratio)
    return ulps, ratio


def compare_values(got, want, o32, what, stats=None):
    """The four outputs: |got - want| <= 4 |o32 - want| + 8 ulp of max(|want|, 1e-3 |want loss|), per output."""
    got, want, o32 = (torch.as_tensor(t).detach().cpu().double().reshape(4) for t in (got, want, o32))
    assert bool(torch.isfinite(got).all()), (what, got.tolist())
    err, err_o = (got - want).abs(), (o32 - want).abs()
    scale = torch.maximum(want.abs(), 1e-3 * want[0].abs())
    allowed = 4 * err_o + 8 * ulp32(scale)
    fig = _note(stats, err, scale, err_o)
    print(f"{what}: " + ", ".join(f"{n} {float(w):.6e} err {float(e):.2e} (oracle {float(o):.2e})" for n, w, e, o in zip(OUT, want, err, err_o))
          + (f"; {fig[0]:.2f} ulp, needs {fig[1]:.2f} x the oracle's error + 8 ulp" if fig else ""))
    bad = err > allowed
    assert not bool(bad.any()), (what, [(OUT[k], float(got[k]), float(want[k]), float(err[k]), float(allowed[k]), float(err_o[k])) for k in bad.nonzero().flatten().tolist()])
    assert bool((got[want == 0] == 0).all()), (what, "nonzero where the float64 value is exactly 0", got.tolist(), want.tolist())


def compare_grad(got, want, o32, what, stats=None):
    """Every element: |got - want| <= 4 |o32 - want| + 8 ulp of max(|want_e|, 1e-3 median |want| of the column); zeros kept."""
    got, want, o32 = (torch.as_tensor(t).detach().cpu().double() for t in (got, want, o32))
    assert got.shape == want.shape == o32.shape, (what, got.shape, want.shape, o32.shape)
    assert bool(torch.isfinite(got).all()), (what, "not finite")
    err, err_o = (got - want).abs(), (o32 - want).abs()
    scale = torch.maximum(want.abs(), 1e-3 * want.abs().median(0).values[None, :])
    allowed = 4 * err_o + 8 * ulp32(scale)
    _note(stats, err, scale, err_o)
    bad = err > allowed
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError((what, int(bad.sum()), "elements out of", bad.numel(),
                              [(n, p, float(got[n, p]), float(want[n, p]), float(err[n, p]), float(allowed[n, p]), float(err_o[n, p])) for n, p in idx]))
    z = want == 0
    assert bool((got[z] == 0).all()), (what, "nonzero where the float64 gradient is exactly 0", int((got[z] != 0).sum()))


# ------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------
def _gen(*key):
    """A generator per key tuple: positional mixing, so that distinct (group, index, seed) tuples give distinct streams."""
    h = 0
    for k in key:
        h = (h * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def _pick(C, V, g):
    """V of the values 0..C, ascending, ins_num = C (LDS row L - 1 of the partial sums) among them."""
    return sorted(torch.randperm(C, generator=g)[:V - 1].tolist() + [C])


# (N, C, tag, label set): the smallest shapes at which a path changes -- one ray; a ragged only chunk; one full chunk; a ragged
# second chunk; C on both sides of the second column per lane (64 | 65) and V of the second row per lane; 17 chunks (one more
# than the 16 lanes per entry of the chunk sum) at C = 127 | 128
SHAPES = (
    (1, 1, "l0", lambda g: [0]),
    (1, 5, "l5", lambda g: [5]),
    (63, 2, "l02", lambda g: [0, 2]),
    (64, 13, "V9", lambda g: _pick(13, 9, g)),
    (65, 13, "V13lo", lambda g: list(range(13))),
    (65, 13, "V13hi", lambda g: list(range(1, 14))),
    (129, 63, "V63", lambda g: list(range(1, 64))),
    (129, 63, "V62", lambda g: _pick(63, 62, g)),
    (129, 64, "V64", lambda g: list(range(64))),
    (129, 64, "V63", lambda g: _pick(64, 63, g)),
    (129, 65, "V65", lambda g: list(range(1, 66))),
    (129, 65, "V64", lambda g: _pick(65, 64, g)),
    (1025, 127, "V100", lambda g: _pick(127, 100, g)),
    (1025, 128, "V128", lambda g: list(range(1, 129))),
    (1025, 128, "V65", lambda g: _pick(128, 65, g)),
)
SATURATED = ("63_2_l02", "65_13_V13lo", "129_64_V63", "129_65_V65", "1025_127_V100", "1025_128_V65")
# seeds: 0 unless the case then misses the margin condition or (saturated) planting moved the assignment off a planted spot
# (tests/test_criterion_restate.py::test_margin_condition, ::test_planted_values_are_where_the_case_says)
SEEDS = {"trained_63_2_l02": 1, "trained_1025_127_V100": 7, "saturated_1025_127_V100": 1, "trained_1025_128_V65": 1,
         "saturated_1025_128_V65": 1}
PLANTED = (0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -30)


def _labels(N, label_set, g):
    s = torch.tensor(label_set, dtype=torch.int64)
    lab = torch.cat([s, s[torch.randint(0, len(s), (N - len(s),), generator=g)]])
    return lab[torch.randperm(N, generator=g)]


def _channels(labels, C, g):
    """A random channel for every row, so that the assignment is not the identity: {label: channel}."""
    rows = rows_of(labels.numpy(), C)
    return dict(zip(rows.tolist(), torch.randperm(C, generator=g)[:len(rows)].tolist()))


def _hot(labels, chan, C):
    h = torch.zeros(labels.shape[0], C)
    for n, l in enumerate(labels.tolist()):
        if l in chan:
            h[n, chan[l]] = 1.0
    return h


def _trained(labels, chan, C, g):
    return torch.sigmoid(torch.randn(labels.shape[0], C, generator=g) + 3.0 * _hot(labels, chan, C))


def _converged(labels, chan, C, g):
    return torch.sigmoid(14.0 * _hot(labels, chan, C) - 7.0 + 0.1 * torch.randn(labels.shape[0], C, generator=g))


def _plant(pred, labels, chan, C, k):
    """0, 1, 1 - 2^-24 and 2^-30 on a matched channel's own rays, on its other rays and on an unmatched channel, in the first
    chunk, the last full chunk and the ragged chunk (those that exist).  ``k`` rotates which value meets which ray."""
    N = pred.shape[0]
    full, rag = N // CHUNK, N % CHUNK
    chunks = [(0, min(N, CHUNK))]
    if full > 1:
        chunks.append(((full - 1) * CHUNK, CHUNK))
    if full >= 1 and rag:
        chunks.append((full * CHUNK, rag))
    matched = sorted(set(chan.values()))
    unmatched = sorted(set(range(C)) - set(matched))
    done = set()
    for ci, (start, length) in enumerate(chunks):
        for i, v in enumerate(PLANTED):
            n = start + (11 * i + 5 * ci + 3) % length
            own = chan[int(labels[n])]
            vi = PLANTED[(i + k + ci) % 4] if length == 1 else v        # a one-ray chunk has one own entry: rotate it per case
            spots = [(n, own, vi)]
            other = [p for p in matched if p != own]
            if other:
                spots.append((n, other[(i + ci + k) % len(other)], v))
            if unmatched:
                spots.append((n, unmatched[(i + ci + k) % len(unmatched)], v))
            for nn, p, val in spots:
                if (nn, p) not in done:
                    done.add((nn, p))
                    pred[nn, p] = val
    return pred


def _case(name, family, labels, pred, C, tied=False, bad=False, identity=False, chan=None):
    return types.SimpleNamespace(name=name, chan=chan, family=family, N=int(pred.shape[0]), C=int(C), labels=labels.contiguous(), pred=pred.to(F32).contiguous(),
                                 tied=tied, bad=bad, identity=identity)


@functools.lru_cache(maxsize=None)
def _all_cases():
    cases = []
    for si, (N, C, tag, label_set) in enumerate(SHAPES):
        shape = f"{N}_{C}_{tag}"
        for fi, family in enumerate(("trained", "converged", "saturated")):
            if family == "saturated" and shape not in SATURATED:
                continue
            name = f"{family}_{shape}"
            g = _gen(si, fi, SEEDS.get(name, 0))
            labels = _labels(N, label_set(g), g)
            chan = _channels(labels, C, g)
            pred = (_converged if family == "converged" else _trained)(labels, chan, C, g)
            if family == "saturated":                         # planted by the assignment the planted predictions have (few rays per
                base, chan = pred, None                       # label: not `chan`, and planting moves it: a few rounds to a fixed point)
                for _ in range(8):
                    ce, siou, rows = cost_matrices64(pred, labels.numpy(), C)
                    now = dict(zip(rows.tolist(), linear_sum_assignment(ce + siou)[1].tolist()))
                    if now == chan:
                        break
                    chan = now
                    pred = _plant(base.clone(), labels, chan, C, si)
            cases.append(_case(name, family, labels, pred, C, chan=chan))
    # labels the reference raises on: N = 65 (a one-ray ragged chunk), C = 5
    N, C = 65, 5
    for bi, kind in enumerate(("range", "many", "none")):
        name = f"bad_{kind}"
        g = _gen(100, bi, SEEDS.get(name, 0))
        if kind == "range":                                   # one negative label, one just above C in the ragged chunk
            labels = _labels(N, [0, 1, 3, 5], g)
            labels[17], labels[64] = -1, C + 1
        elif kind == "many":                                  # all six labels: 0..4 form the rows, the rays of 5 join none
            labels = _labels(N, list(range(C + 1)), g)
        else:                                                 # no row at all
            labels = torch.tensor([-1, -7, C + 1, C + 4], dtype=torch.int64)[torch.randint(0, 4, (N,), generator=g)]
        chan = _channels(labels, C, g)
        cases.append(_case(name, "bad labels", labels, _trained(labels, chan, C, g), C, bad=True))
    # ties
    ti = 0
    for C, N in ((13, 65), (70, 129)):
        for V in (C - 3, C):
            for kind in ("half", "dup"):
                name = f"tied_{kind}_{N}_{C}_V{V}"
                g = _gen(200, ti, SEEDS.get(name, 0))
                ti += 1
                labels = _labels(N, list(range(1, V + 1)) if V == C else _pick(C, V, g), g)
                if kind == "half":                            # every row of the cost is one constant
                    pred = torch.full((N, C), 0.5)
                else:                                         # one matched channel copied bit for bit into another
                    chan = _channels(labels, C, g)
                    pred = _trained(labels, chan, C, g)
                    rows = sorted(chan)
                    src = chan[rows[len(rows) // 2]]
                    free = sorted(set(range(C)) - set(chan.values()))
                    dst = free[len(free) // 2] if free else chan[rows[0]]
                    pred[:, dst] = pred[:, src]
                cases.append(_case(name, "tied", labels, pred, C, tied=True, identity=(kind == "half")))
    return tuple(cases)


def case_names(pred=lambda c: True):
    return [c.name for c in _all_cases() if pred(c)]


def case(name):
    return {c.name: c for c in _all_cases()}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 cost matrices of a case, scipy's assignment on their sum, its total and the margin-condition bound."""
    c = case(name)
    ce, siou, rows = cost_matrices64(c.pred, c.labels.numpy(), c.C)
    cost = ce + siou
    cols = linear_sum_assignment(cost)[1].astype(np.int64) if len(rows) else np.zeros(0, dtype=np.int64)
    return types.SimpleNamespace(ce=ce, siou=siou, rows=rows, cost=cost, cols=cols, V=len(rows), U=c.C - len(rows),
                                 total=float(cost[np.arange(len(rows)), cols].sum()), bound=margin_bound(cost))


def margin(name):
    r = reference(name)
    return assignment_margin(r.cost, r.cols) if r.V else np.inf


@functools.lru_cache(maxsize=None)
def _oracle_of(name, oracle):
    c = case(name)
    return oracle32(c.pred, c.labels.numpy(), c.C, oracle)


def yardsticks(name, cols, oracle):
    """``(want_out, want_grads, o32_out, o32_grads, which)`` at the assignment ``cols``: float64, and the float32 oracle's (or,
    where it cannot run or ran at another assignment, the float32 yardstick's); ``which`` names the float32 side."""
    c = case(name)
    want_out, want_grads = evaluate64(c.pred, c.labels.numpy(), c.C, cols)
    if oracle_runs(c):
        o_out, o_grads, o_cols = _oracle_of(name, oracle)
        if np.array_equal(o_cols, np.asarray(cols)):
            return want_out, want_grads, o_out, o_grads, "oracle"
    o_out, o_grads = evaluate32(c.pred, c.labels.numpy(), c.C, cols)
    return want_out, want_grads, o_out, o_grads, "float32 yardstick"


def two_level_case():
    """(65, 128): one label vector, two predictions trained towards different channel permutations (the two levels of a step)."""
    N, C = 65, 128
    g = _gen(300, 0)
    labels = _labels(N, _pick(C, 40, g), g)
    a = _trained(labels, _channels(labels, C, g), C, g)
    b = _trained(labels, _channels(labels, C, g), C, g)
    return _case("two_level_a", "two level", labels, a, C), _case("two_level_b", "two level", labels, b, C)


def planted_census(name):
    """Where the planted values of a saturated case sit under the case's own (scipy, float64) assignment:
    {chunk kind: {(place, value)}} with place in own | other | unmatched."""
    c, ref = case(name), reference(name)
    lab = c.labels.numpy()
    col_of = dict(zip(ref.rows.tolist(), ref.cols.tolist()))
    matched = set(ref.cols.tolist())
    full, rag = c.N // CHUNK, c.N % CHUNK
    chunks = {"first": (0, min(c.N, CHUNK))}
    if full > 1:
        chunks["last full"] = ((full - 1) * CHUNK, full * CHUNK)
    if full >= 1 and rag:
        chunks["ragged"] = (full * CHUNK, c.N)
    census = {}
    for where, (n0, n1) in chunks.items():
        census[where] = set()
        for v in PLANTED:
            for n, p in (c.pred[n0:n1] == np.float32(v)).nonzero().tolist():
                place = "own" if col_of[int(lab[n + n0])] == p else ("other" if p in matched else "unmatched")
                census[where].add((place, v))
    return census
