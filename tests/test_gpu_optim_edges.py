"""GPU tests (-m gpu) of the two kernels of csrc/optim.hip at their edges, through the C entries ``dmnerf_adam_step`` and
``dmnerf_repack_train`` directly (tests/test_gpu_optim.py drives them through ``FlatAdam`` at one shape): vector lengths around the
quad, the block and the grid-stride trip; 4-byte-aligned vectors (the scalar path); zero, denormal, overflowing and non-finite
gradients; the device step counter across launches of different grids and from a loaded count; ``d_lr``; the re-pack with 1, 3 and
4 models of different widths, with and without ``d_f_pos`` and ``d_flat_copy``; ``FlatAdam`` with 1, 3 and 4 models.

Yardsticks.  Bits, non-finite placement and the overflow edge: ``torch.optim.Adam(foreach=True)`` on the device over one flat
parameter -- the twin csrc/optim.hip documents (``g * g`` first: a gradient beyond ~1.8e19 makes v = inf and freezes its element;
single-tensor Adam would not).  Its bounds are those of test_gpu_optim.py.  Away from that edge the float64 restatement
tests/_optim_restate.py::adam_f64 referees too, within 4 x the f32 class below.

The f32 class.  How close an f32 Adam can be to float64 is measured, not guessed: torch's CPU float32 Adam (single-tensor form) is
run on every case of ``_optim_restate.gpu_adam_cases()`` -- the very (sequence, length) pairs compared with float64 here -- and per
quantity the worst deviation from ``adam_f64`` is taken, overflow elements excluded.  The constants are those CPU measurements
(x86-64, torch 2.10, rounded up to three digits; tests/test_optim_restate.py re-measures them); none comes from the kernels.  The
device must be within 4 x: a differently contracted f32 chain of the same length is the same class of arithmetic, not the same
rounding.  Likewise the head product: a CPU float32 matmul of the two named tensors against float64, worst over the four widths."""
import functools
import types

import numpy as np
import pytest
import torch

import _gpu
import _optim_restate as RS
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

# torch CPU float32 Adam vs adam_f64, worst over _optim_restate.gpu_adam_cases() (measured on the CPU):
F32_P = 3.82e-7                        # |dp| / (|p| + 1e-3)
F32_M = 1.47e-8                        # |dm| / max |g| the vector saw
F32_V = 5.08e-7                        # |dv| / v, over v above the smallest normal float
# CPU float32 matmul A . W_rf vs float64, worst over _optim_restate.REPACK_INS: max |error| / max |F|
F32_HEAD = 6.99e-7
FACTOR = 4.0

LR, BETAS, EPS = RS.LR, RS.BETAS, RS.EPS
N = RS.N_EDGE
GUARD = 64                             # floats of NaN before and after every vector (256 B: the vector itself stays 16-byte aligned)
NAN_BITS = 0x7FC00000                  # what torch.full(nan) writes


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from dm_nerf_amd import _lib
    _lib.load()
    return _lib


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Vec:
    """``n`` floats inside a NaN-filled allocation with GUARD floats before and behind; ``offset`` floats past 16-byte alignment."""

    def __init__(self, n, data=None, offset=0):
        self.n, self.lo = n, GUARD + offset
        self.buf = torch.full((self.lo + n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.v = self.buf[self.lo:self.lo + n]
        if data is None:
            self.v.zero_()
        else:
            self.v.copy_(data)
        assert self.buf.data_ptr() % 16 == 0 and self.v.data_ptr() % 16 == 4 * offset

    def guards_intact(self):
        b = bits(self.buf)
        return bool((b[:self.lo] == NAN_BITS).all()) and bool((b[self.lo + self.n:] == NAN_BITS).all())


def run_own(L, p0, grads, offsets=(0, 0, 0, 0), lr=LR, d_lr=None, betas=BETAS, eps=EPS, t0=0, m0=None, v0=None, history=False):
    """``len(grads)`` calls of dmnerf_adam_step on guarded vectors; ``lr``: one number or one per step.  Returns p, m, v (clones),
    the state2 tensor and, with ``history``, (p, m, v) after every step.  The guards are checked here."""
    lib = L.load()
    n = p0.numel()
    p, g, m, v = Vec(n, p0, offsets[0]), Vec(n, None, offsets[1]), Vec(n, m0, offsets[2]), Vec(n, v0, offsets[3])
    state2 = torch.tensor([t0, 0], dtype=torch.int64, device="cuda")
    lrs = [float(lr)] * len(grads) if np.ndim(lr) == 0 else [float(x) for x in lr]
    hist = []
    for k, gr in enumerate(grads):
        g.v.copy_(gr)
        L.check(lib.dmnerf_adam_step(L.ptr(p.v), L.ptr(g.v), L.ptr(m.v), L.ptr(v.v), n, lrs[k], L.ptr(d_lr), betas[0], betas[1], eps,
                                     L.ptr(state2), L.stream()), "dmnerf_adam_step")
        if history:
            hist.append((p.v.clone(), m.v.clone(), v.v.clone()))
    torch.cuda.synchronize()
    assert all(x.guards_intact() for x in (p, g, m, v)), "a guard element around p / g / m / v was written"
    assert same_bits(g.v, grads[-1].cuda()), "the gradient vector was written"
    assert state2.tolist() == [t0 + len(grads), 0]
    return types.SimpleNamespace(p=p.v.clone(), m=m.v.clone(), v=v.v.clone(), state2=state2, hist=hist)


def run_twin(p0, grads, lr=LR, betas=BETAS, eps=EPS, state=None, history=False):
    """The device twin: one flat f32 parameter under torch.optim.Adam(foreach=True), the same gradients.  ``state``: a
    torch.optim.Adam state_dict to load first."""
    p = torch.nn.Parameter(p0.cuda().clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=True)
    if state is not None:
        opt.load_state_dict(state)
    hist = []
    for gr in grads:
        p.grad = gr.cuda().clone()
        opt.step()
        if history:
            hist.append((p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()))
    torch.cuda.synchronize()
    st = opt.state[p]
    return types.SimpleNamespace(p=p.detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(), hist=hist, opt=opt)


def follows_twin(own, twin, grads):
    """Non-finite values sit where the twin's sit (same kind, same sign); every finite element within test_gpu_optim.py's bounds:
    p 2.4e-7 |p| + 2e-8, m 2.4e-7 |m| + 2.4e-7 max|g|, v 1e-6 v + 1e-37.  max|g| is taken over the elements that never saw an
    overflowing gradient (an element's error depends on its own gradients only; 1e20 there would make the bound of all the others
    vacuous); the overflow elements themselves get the vector's full max|g|.  Returns which of p / m / v came out bit-equal."""
    keep = ~RS.overflow_mask(grads)
    gm = torch.full_like(twin.p, RS.gmax(grads, keep) if keep.any() else 0.0)
    gm[torch.from_numpy(~keep).cuda()] = RS.gmax(grads)
    for a, b in ((own.p, twin.p), (own.m, twin.m), (own.v, twin.v)):
        assert torch.equal(torch.isnan(a), torch.isnan(b)), "NaN placement differs from the twin's"
        assert torch.equal(torch.isinf(a), torch.isinf(b)) and torch.equal(a[torch.isinf(b)], b[torch.isinf(b)]), "inf placement differs"
    fin = torch.isfinite(twin.p)
    dp = (own.p - twin.p).abs()[fin]
    assert bool((dp <= 2.4e-7 * twin.p.abs()[fin] + 2e-8).all()), float(dp.max())
    fin = torch.isfinite(twin.m)
    dm = (own.m - twin.m).abs()[fin]
    assert bool((dm <= 2.4e-7 * twin.m.abs()[fin] + 2.4e-7 * gm[fin]).all()), float(dm.max())
    fin = torch.isfinite(twin.v)
    dv = (own.v - twin.v).abs()[fin]
    assert bool((dv <= 1e-6 * twin.v[fin] + 1e-37).all()), float(dv.max())
    return {"p": same_bits(own.p, twin.p), "m": same_bits(own.m, twin.m), "v": same_bits(own.v, twin.v)}


@functools.lru_cache(maxsize=None)
def ref64(name, n):
    """adam_f64 over the whole case: computed once, shared, never modified."""
    p0, grads = RS.case(name, n)
    return RS.adam_f64(p0, grads)


def within_f32_class(own, name, n):
    """Within 4 x the measured f32 class of the float64 restatement (overflow elements excluded)."""
    _, grads = RS.case(name, n)
    dev = RS.deviation((own.p.cpu().numpy(), own.m.cpu().numpy(), own.v.cpu().numpy()), ref64(name, n), grads)
    assert dev["p"] <= FACTOR * F32_P and dev["m"] <= FACTOR * F32_M and dev["v"] <= FACTOR * F32_V, dev
    return dev


def report(capsys, what, exact, dev=None):
    with capsys.disabled():
        tail = "" if dev is None else (f"; vs float64: |dp| / (|p| + 1e-3) {dev['p']:.2e}, |dm| / max|g| {dev['m']:.2e}, |dv| / v {dev['v']:.2e} "
                                       f"(bounds {FACTOR * F32_P:.2e}, {FACTOR * F32_M:.2e}, {FACTOR * F32_V:.2e})")
        print(f"\n[adam_step {what}] bit-equal to the device twin: {exact}{tail}")


# ------------------------------------------------------------------------------------------ Adam against the device twin
@pytest.mark.parametrize("n", RS.LENGTHS)
def test_adam_lengths_follow_the_twin_and_float64(L, capsys, n):
    """Below a quad, a quad, quad + tail, one block exactly, a second block of one element, a ragged tail, three grid-stride
    trips (2^21 + 4099: 1024 blocks, a ragged third trip, a three-element tail); all four vectors 16-byte aligned."""
    p0, grads = RS.case("spread", n)
    assert len(grads) == (3 if n == RS.BIG else 12)
    own, twin = run_own(L, p0, grads), run_twin(p0, grads)
    exact = follows_twin(own, twin, grads)
    dev = within_f32_class(own, "spread", n)
    assert float((own.p.cpu() - p0).abs().max()) > 1e-4                   # it moved
    report(capsys, f"spread n={n}", exact, dev)


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
def test_adam_with_one_vector_four_byte_aligned(L, capsys, which):
    """One of the four vectors starts one float into a 16-byte-aligned allocation: legal, and the kernel must take its scalar
    path for ALL elements (a float4 access there would be misaligned).  Same results, guards untouched."""
    offsets = tuple(int(w == which) for w in "pgmv")
    p0, grads = RS.case("spread", N)
    own, twin = run_own(L, p0, grads, offsets=offsets), run_twin(p0, grads)
    exact = follows_twin(own, twin, grads)
    dev = within_f32_class(own, "spread", N)
    aligned = run_own(L, p0, grads)
    assert same_bits(own.p, aligned.p) and same_bits(own.m, aligned.m) and same_bits(own.v, aligned.v)      # scalar path == quad path
    report(capsys, f"spread n={N}, {which} offset by one float", exact, dev)


# ------------------------------------------------------------------------------------------ value edges
OVER = (2, 3, N - 6, N - 5)            # where "edges" carries +-1e20


@pytest.mark.parametrize("p_offset", [0, 1])
def test_adam_value_edges_denormal_overflow_signed_zero(L, capsys, p_offset):
    """Step 3 carries 1e-40, -1e-40, 1e20, -1e20, 0.0, -0.0, 3e-23, 1e-30 at 0..7 and in the last eight elements.  Non-finite
    placement as the twin's; the overflow elements get v = +inf and stop moving from step 3 on (m stays finite) in BOTH; the
    denormal / zero elements follow the twin within the bounds and float64 within the f32 class."""
    p0, grads = RS.case("edges", N)
    own = run_own(L, p0, grads, offsets=(p_offset, 0, 0, 0), history=True)
    twin = run_twin(p0, grads, history=True)
    exact = follows_twin(own, twin, grads)
    dev = within_f32_class(own, "edges", N)
    idx = torch.tensor(OVER, device="cuda")
    for run in (own, twin):
        assert bool((run.v[idx] == float("inf")).all()) and bool(torch.isfinite(run.m[idx]).all()) and bool(torch.isfinite(run.p[idx]).all())
        assert not same_bits(run.hist[1][0][idx], p0.cuda()[idx])                          # moved in steps 1 and 2
        for k in range(RS.EDGE_STEP - 1, len(grads)):
            assert same_bits(run.hist[k][0][idx], run.hist[RS.EDGE_STEP - 2][0][idx]), k    # frozen from step 3 on
            assert bool((run.hist[k][2][idx] == float("inf")).all())
    for x in (own.p, own.m, own.v):
        rest = torch.ones(N, dtype=torch.bool, device="cuda")
        rest[idx] = False
        assert bool(torch.isfinite(x[rest]).all())
    assert not same_bits(own.hist[-1][0][:2], own.hist[RS.EDGE_STEP - 2][0][:2])            # the denormal elements keep moving
    report(capsys, f"edges n={N}, p offset {p_offset}", exact, dev)


@pytest.mark.parametrize("p_offset", [0, 1])
def test_adam_all_zero_gradients_on_zero_moments_leave_p_bit_equal(L, capsys, p_offset):
    p0, grads = RS.case("all_zero_first", N)
    own = run_own(L, p0, grads, offsets=(p_offset, 0, 0, 0), history=True)
    twin = run_twin(p0, grads)
    p2, m2, v2 = own.hist[1]
    assert same_bits(p2, p0.cuda()), "p moved on a zero gradient with zero moments"
    assert same_bits(m2, torch.zeros(N, device="cuda")) and same_bits(v2, torch.zeros(N, device="cuda"))
    exact = follows_twin(own, twin, grads)
    dev = within_f32_class(own, "all_zero_first", N)
    report(capsys, f"all_zero_first n={N}, p offset {p_offset}", exact, dev)


@pytest.mark.parametrize("p_offset", [0, 1])
def test_adam_eps_zero_and_zero_gradient_on_zero_moments_is_nan_as_in_the_twin(L, capsys, p_offset):
    """0 / (sqrt(0) / c + 0) = NaN exactly where the gradient is zero, finite elsewhere; m = v = 0 there."""
    p0, grads = RS.case("spread", N)
    grads = grads[:1]
    zero = (grads[0] == 0).cuda()
    assert 20 < int(zero.sum()) < N // 4
    own = run_own(L, p0, grads, offsets=(p_offset, 0, 0, 0), eps=0.0)
    twin = run_twin(p0, grads, eps=0.0)
    exact = follows_twin(own, twin, grads)
    for run in (own, twin):
        assert torch.equal(torch.isnan(run.p), zero)
        assert not bool(run.m[zero].any()) and not bool(run.v[zero].any())
    report(capsys, f"eps = 0, n={N}, p offset {p_offset}", exact)


# ------------------------------------------------------------------------------------------ poison stays in its element
POISON_AT = (0, 3, 4, 2047, 2048, 2050)           # the first quad's ends, the next quad, the last quad's end, the tail's first and last


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_adam_poisoned_gradient_entry_stays_in_its_element(L, poison):
    p0, grads = RS.case("spread", N)
    grads = grads[:3]
    clean = run_own(L, p0, grads)
    for at in POISON_AT:
        bad = [g.clone() for g in grads]
        bad[1][at] = poison
        got = run_own(L, p0, bad)
        rest = torch.ones(N, dtype=torch.bool, device="cuda")
        rest[at] = False
        for a, b in ((got.p, clean.p), (got.m, clean.m), (got.v, clean.v)):
            assert same_bits(a[rest], b[rest]), at
        assert bool(torch.isnan(got.p[at])) and not bool(torch.isfinite(got.m[at])) and not bool(torch.isfinite(got.v[at])), at


# ------------------------------------------------------------------------------------------ step counter and ticket
def test_step_counter_and_ticket_across_launches_of_different_grids(L):
    """One state2 tensor, one stream, five launches on their own vectors: 1, 2, 147, 1024 and 1 workgroups.  The last workgroup to
    finish stores the count and resets the ticket, whatever the grid of the launch before was."""
    lib = L.load()
    state2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(21)
    keep = []
    for k, n in enumerate((5, 2049, 300000, RS.BIG, 5), start=1):
        assert min((n + 2047) // 2048, 1024) == (1, 2, 147, 1024, 1)[k - 1]
        p = torch.randn(n, device="cuda", generator=g)
        gr = torch.randn(n, device="cuda", generator=g)
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        keep.append((p, gr, m, v))
        p_before = p.clone()
        L.check(lib.dmnerf_adam_step(L.ptr(p), L.ptr(gr), L.ptr(m), L.ptr(v), n, LR, None, BETAS[0], BETAS[1], EPS, L.ptr(state2), L.stream()),
                "dmnerf_adam_step")
        torch.cuda.synchronize()
        assert state2.tolist() == [k, 0], (k, n, state2.tolist())
        # the t this launch used, read off the update: on fresh moments m = (1 - b1) g and v = (1 - b2) g^2, so every element moves
        # by lr (1 - b1) / (1 - b1^t) . sqrt((1 - b2^t) / (1 - b2)) whatever g is -- t = k here, the count the other vectors left
        want = LR * (1 - BETAS[0]) / (1 - BETAS[0] ** k) / (((1 - BETAS[1]) / (1 - BETAS[1] ** k)) ** 0.5)
        moved = (p - p_before).abs()
        big = gr.abs() > 1e-3                                               # (eps = 1e-8 is negligible against |g| there)
        assert bool(((moved[big] - want).abs() <= 1e-3 * want + 6e-8 * (p_before.abs()[big] + want)).all()), (k, n)     # (eps; half an ulp of p)
    del keep


def _loaded_state(n, step):
    """A torch.optim.Adam state_dict with realistic moments (three steps of ``spread``) whose step count reads ``step``."""
    p0, grads = RS.spread(n, 8, 77)
    warm = run_twin(p0, grads[:3])
    sd = warm.opt.state_dict()
    st = sd["state"][0]
    assert float(st["step"]) == 3.0
    sd["state"] = {0: {"step": torch.tensor(float(step)), "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone()}}
    assert float(sd["state"][0]["step"]) == step
    return warm.p.cpu(), grads[3:], sd, st["exp_avg"].clone(), st["exp_avg_sq"].clone()      # (own copies: a twin may adopt sd's tensors)


@pytest.mark.parametrize("step", [999, 10 ** 6])
def test_adam_from_a_preloaded_step_count_follows_the_twin(L, capsys, step):
    """The checkpoint path: state2[0] preloaded, moments from a torch optimizer's state_dict at that step; five steps on n = 2049
    (two workgroups).  At 10^6 both b^t underflow to 0 in double: the bias corrections are exactly 1."""
    n = 2049
    p0, grads, sd, m0, v0 = _loaded_state(n, step)
    twin = run_twin(p0, grads, state=sd)
    assert float(twin.opt.state_dict()["state"][0]["step"]) == step + 5
    own = run_own(L, p0, grads, t0=step, m0=m0, v0=v0)
    assert own.state2.tolist() == [step + 5, 0]
    exact = follows_twin(own, twin, grads)
    fresh = run_own(L, p0, grads, m0=m0, v0=v0)
    assert not same_bits(fresh.p, own.p)                                   # the preloaded count is what the kernel used
    report(capsys, f"from step {step}, n={n}", exact)


def test_adam_with_no_elements_leaves_the_state_alone(L):
    lib = L.load()
    state2 = torch.tensor([7, 0], dtype=torch.int64, device="cuda")
    x = [torch.full((4,), float("nan"), device="cuda") for _ in range(4)]
    assert lib.dmnerf_adam_step(L.ptr(x[0]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(x[3]), 0, LR, None, BETAS[0], BETAS[1], EPS, L.ptr(state2), L.stream()) == 0
    torch.cuda.synchronize()
    assert state2.tolist() == [7, 0] and all(bool((bits(t) == NAN_BITS).all()) for t in x)


def test_refused_calls_leave_the_buffers_untouched(L):
    """The refusals of tests/test_optim_restate.py on real buffers: nothing is launched, nothing is written."""
    lib = L.load()
    state2 = torch.tensor([7, 0], dtype=torch.int64, device="cuda")
    x = [torch.full((8,), float("nan"), device="cuda") for _ in range(4)]
    for kw in (dict(n=-1), dict(b1=1.0), dict(b2=1.0), dict(eps=-1.0), dict(b1=0.5)):
        a = dict(dict(n=8, b1=0.9, b2=0.999, eps=1e-8), **kw)
        assert lib.dmnerf_adam_step(L.ptr(x[0]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(x[3]), a["n"], LR, None, a["b1"], a["b2"], a["eps"],
                                    L.ptr(state2), L.stream()) == -1, kw
    torch.cuda.synchronize()
    assert state2.tolist() == [7, 0] and all(bool((bits(t) == NAN_BITS).all()) for t in x)


# ------------------------------------------------------------------------------------------ d_lr
def test_device_learning_rate_overrides_the_host_one(L):
    p0, grads = RS.case("spread", N)
    lr32 = float(np.float32(3e-4))
    d_lr = torch.tensor(3e-4, dtype=torch.float32, device="cuda")
    dev = run_own(L, p0, grads[:1], lr=7.0, d_lr=d_lr)
    host = run_own(L, p0, grads[:1], lr=lr32)
    wrong = run_own(L, p0, grads[:1], lr=7.0)
    assert same_bits(dev.p, host.p) and same_bits(dev.m, host.m) and same_bits(dev.v, host.v)
    assert not same_bits(dev.p, wrong.p)
    assert float((wrong.p - dev.p).abs().max()) > 1.0                       # lr = 7 is not a subtle difference
    assert float(d_lr) == lr32                                              # the kernel only reads it


def test_device_learning_rate_written_between_launches_changes_the_next_step_only(L):
    lib = L.load()
    p0, grads = RS.case("spread", N)
    lr_a, lr_b = float(np.float32(3e-4)), float(np.float32(1e-5))
    d_lr = torch.tensor(lr_a, dtype=torch.float32, device="cuda")
    p, m, v = p0.cuda().clone(), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    state2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = [grads[0].cuda(), grads[1].cuda()]
    after = []
    for k in range(2):
        L.check(lib.dmnerf_adam_step(L.ptr(p), L.ptr(g[k]), L.ptr(m), L.ptr(v), N, 7.0, L.ptr(d_lr), BETAS[0], BETAS[1], EPS, L.ptr(state2),
                                     L.stream()), "dmnerf_adam_step")
        after.append(p.clone())
        d_lr.fill_(lr_b)                                                    # (same stream: ordered behind the launch that read lr_a)
    torch.cuda.synchronize()
    same = run_own(L, p0, grads[:2], lr=lr_a, history=True)
    changed = run_own(L, p0, grads[:2], lr=(lr_a, lr_b))
    assert same_bits(after[0], same.hist[0][0])                             # the first step saw lr_a
    assert same_bits(after[1], changed.p) and not same_bits(after[1], same.p)
    assert same_bits(m, changed.m) and same_bits(v, changed.v) and state2.tolist() == [2, 0]


# ------------------------------------------------------------------------------------------ re-pack
SHAPES = {"one": (13,), "three": (13, 127, 1), "four": (59, 13, 127, 1)}
PAD = 64                                # floats of NaN behind every output


@pytest.fixture(scope="module")
def packs(L):
    """Per width: the flat parameters on the device, the pack indices, d_f_pos, and the reference -- what a model packs for itself
    (weights.pack_blob: dmnerf_head_product + dmnerf_pack_weights) -- computed once, never modified."""
    from dm_nerf_amd import optim, weights
    lib = L.load()
    out = {}
    for ins in RS.REPACK_INS:
        state = {k: t.cuda() for k, t in O.make_weights(RS.REPACK_SEED[ins], ins, gain=1.7, sigma_bias=0.3).items()}
        flat = weights.flat_params(state)
        assert torch.equal(flat.cpu(), RS.repack_flat(ins))
        n = int(lib.dmnerf_param_count(ins))
        assert flat.numel() == n
        f_pos = optim._head_positions(ins, n, flat.device)
        assert f_pos is not None and f_pos.numel() == weights.HEAD_F_FLOATS and f_pos.dtype == torch.int32
        out[ins] = types.SimpleNamespace(
            ins=ins, n=n, flat=flat, idx=weights.pack_index(ins, flat.device, False), idx_t=weights.pack_index(ins, flat.device, True), f_pos=f_pos,
            n_blob=int(lib.dmnerf_blob_floats(ins)), n_blob_t=int(lib.dmnerf_blob_t_floats(ins)),
            blob=weights.pack_blob(state, ins, flat=flat), blob_t=weights.pack_blob(state, ins, transposed=True, flat=flat))
        assert out[ins].blob.numel() == out[ins].n_blob and out[ins].blob_t.numel() == out[ins].n_blob_t
    torch.cuda.synchronize()
    return out


def nan_filled(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def is_nan_fill(t):
    return bool((bits(t) == NAN_BITS).all())


def run_repack(L, packs, widths, gather, copy=True, src_offset=0):
    """One dmnerf_repack_train launch over ``widths``; outputs PAD floats longer than required, pre-filled with NaN."""
    arr = (L.RepackModel * len(widths))()
    outs = []
    for i, ins in enumerate(widths):
        P = packs[ins]
        src_buf = torch.empty(P.n + src_offset, dtype=torch.float32, device="cuda")
        src = src_buf[src_offset:]
        src.copy_(P.flat)
        assert src.data_ptr() % 16 == 4 * src_offset
        o = types.SimpleNamespace(P=P, src_buf=src_buf, src=src, copy=nan_filled(P.n + PAD), blob=nan_filled(P.n_blob + PAD), blob_t=nan_filled(P.n_blob_t + PAD))
        arr[i] = L.RepackModel(src.data_ptr(), ins, o.copy.data_ptr() if copy else None, P.idx.data_ptr(), o.blob.data_ptr(), P.idx_t.data_ptr(),
                               o.blob_t.data_ptr(), None if gather else P.f_pos.data_ptr())
        outs.append(o)
    L.check(L.load().dmnerf_repack_train(arr, len(widths), L.stream()), "dmnerf_repack_train")
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("variant", ["plain", "no_flat_copy", "source_offset_by_one_float"])
@pytest.mark.parametrize("gather", [False, True], ids=["f_pos", "gather"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_repack_models_of_different_widths_in_one_launch(L, packs, shape, gather, variant):
    """1, 3 and 4 models per launch (blockIdx.y picks the model, the grid is sized by the largest), d_f_pos given or NULL (every F
    slot of the W^T blob computes its element itself), with and without d_flat_copy, the source 16- or 4-byte aligned: flat copy,
    forward blob and W^T blob bit-equal to what each model packs for itself; NaN guards behind every output untouched."""
    outs = run_repack(L, packs, SHAPES[shape], gather, copy=variant != "no_flat_copy", src_offset=int(variant == "source_offset_by_one_float"))
    for o in outs:
        P = o.P
        assert same_bits(o.src, P.flat), P.ins                                            # the source is only read
        assert same_bits(o.blob[:P.n_blob], P.blob), P.ins
        assert same_bits(o.blob_t[:P.n_blob_t], P.blob_t), P.ins
        if variant == "no_flat_copy":
            assert is_nan_fill(o.copy), P.ins                                             # where the copy would go: still NaN
        else:
            assert same_bits(o.copy[:P.n], P.flat), P.ins
        assert is_nan_fill(o.copy[P.n:]) and is_nan_fill(o.blob[P.n_blob:]) and is_nan_fill(o.blob_t[P.n_blob_t:]), P.ins


@pytest.mark.parametrize("gather", [False, True], ids=["f_pos", "gather"])
def test_repack_head_product_against_float64(L, packs, capsys, gather):
    """The F block read back out of the W^T blob through d_f_pos = A . W_rf in float64, within 4 x the f32 class of that product
    (a transposed or shifted F is an O(1) error)."""
    outs = run_repack(L, packs, SHAPES["four"], gather)
    for o in outs:
        P = o.P
        got = o.blob_t[P.f_pos.long()].reshape(128, 256).cpu().double().numpy()
        want = RS.head_product_f64(RS.repack_flat(P.ins), P.ins)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        with capsys.disabled():
            print(f"\n[repack head product, ins_num {P.ins}, {'gather' if gather else 'f_pos'}] max |error| / max |F| {err:.2e} (bound {FACTOR * F32_HEAD:.2e})")
        assert err <= FACTOR * F32_HEAD, (P.ins, err)


# ------------------------------------------------------------------------------------------ FlatAdam with other model counts
def make_models(specs):
    return [_gpu.model_from(O.make_weights(seed, ins, gain=1.7, sigma_bias=0.3), ins, train=True) for seed, ins in specs]


COUNTS = {"one": ((61, 13),), "three": ((61, 13), (62, 59), (63, 13)), "four": ((61, 13), (62, 59), (63, 13), (64, 13))}


@pytest.mark.parametrize("count", list(COUNTS))
def test_flat_adam_with_one_three_and_four_models(L, capsys, count):
    """test_gpu_optim.py::test_flat_adam_follows_torch_adam_on_identical_gradients with 1, 3 (two widths) and 4 models (a flat
    vector beyond 2^21: a third grid-stride trip), 5 steps: its bounds, its identity and data_ptr assertions; the re-packed
    caches equal what the models pack for themselves."""
    from dm_nerf_amd import weights
    from dm_nerf_amd.optim import FlatAdam
    ref_models, own_models = make_models(COUNTS[count]), make_models(COUNTS[count])
    ref_params = [p for m in ref_models for p in m.parameters()]
    before = [p.detach().clone() for m in own_models for p in m.parameters()]
    ids = [id(p) for m in own_models for p in m.parameters()]
    ref = torch.optim.Adam(ref_params, lr=5e-4, betas=(0.9, 0.999))
    own = FlatAdam(own_models, lr=5e-4, betas=(0.9, 0.999))
    assert [id(p) for m in own_models for p in m.parameters()] == ids
    assert all(torch.equal(a, p) for a, p in zip(before, [p for m in own_models for p in m.parameters()]))
    assert all(p.data_ptr() == own.flat.data_ptr() + 4 * o for p, o in zip(own.params, np.cumsum([0] + [p.numel() for p in own.params[:-1]])))
    assert (own.flat.numel() > 2 ** 21) == (count == "four")
    g = torch.Generator(device="cuda").manual_seed(3)
    gmax = [0.0] * len(own.params)
    for it in range(1, 6):
        ref.zero_grad(); own.zero_grad()
        for k, (pr, po) in enumerate(zip(ref_params, own.params)):
            gr = torch.randn(pr.shape, device="cuda", generator=g) * 10.0 ** torch.randint(-6, 1, (1,), device="cuda", generator=g).float()
            gr[torch.rand(pr.shape, device="cuda", generator=g) < 0.05] = 0.0
            gmax[k] = max(gmax[k], float(gr.abs().max()))
            pr.grad, po.grad = gr, gr.clone()
        ref.step(); own.step()
    torch.cuda.synchronize()
    exact = {"p": True, "m": True, "v": True}
    o = 0
    for pr, po, gm in zip(ref_params, own.params, gmax):
        n = pr.numel()
        st = ref.state[pr]
        dp = (pr.detach() - po.detach()).abs()
        assert bool((dp <= 2.4e-7 * pr.detach().abs() + 2e-8).all()), float(dp.max())
        dm = (st["exp_avg"].reshape(-1) - own.exp_avg[o:o + n]).abs()
        assert bool((dm <= 2.4e-7 * st["exp_avg"].reshape(-1).abs() + 2.4e-7 * gm).all()), (float(dm.max()), gm)
        dv = (st["exp_avg_sq"].reshape(-1) - own.exp_avg_sq[o:o + n]).abs()
        assert bool((dv <= 1e-6 * st["exp_avg_sq"].reshape(-1).abs() + 1e-37).all()), float(dv.max())
        exact = {"p": exact["p"] and float(dp.max()) == 0.0, "m": exact["m"] and float(dm.max()) == 0.0, "v": exact["v"] and float(dv.max()) == 0.0}
        o += n
    assert o == own.flat.numel()
    moved = max(float((a - p.detach()).abs().max()) for a, p in zip(before, own.params))
    assert own.state2.tolist() == [5, 0] and moved > 1e-3
    for m in own_models:
        state = dict(m.named_parameters())
        flat = weights.flat_params(state)
        assert torch.equal(m.flat(), flat) and m.flat().data_ptr() != flat.data_ptr()
        assert torch.equal(m.blob(), weights.pack_blob(state, m.ins_num, flat=flat))
        assert torch.equal(m.blob_t(), weights.pack_blob(state, m.ins_num, transposed=True, flat=flat))
    with capsys.disabled():
        print(f"\n[FlatAdam, {count} model(s), {own.flat.numel()} parameters, 5 steps] bit-equal to torch.optim.Adam: {exact}; moved by up to {moved:.2e}")


def test_flat_adam_refuses_five_models(L):
    from dm_nerf_amd.optim import FlatAdam
    ms = make_models(((61, 13),))
    with pytest.raises(ValueError, match="1..4 models"):
        FlatAdam(ms * 5)
    with pytest.raises(ValueError, match="1..4 models"):
        FlatAdam([])


def test_flat_adam_state_dict_before_any_step_and_mismatched_step_counts(L):
    """``state_dict()`` before any step has an empty ``state`` (as torch.optim.Adam's) and loads into torch.optim.Adam; a state
    whose parameters carry different step counts is refused (one counter serves all), and a correct load afterwards leaves the
    optimizer usable: its next step follows torch.optim.Adam from the same state."""
    from dm_nerf_amd.optim import FlatAdam
    own_models, ref_models = make_models(((61, 13),)), make_models(((61, 13),))
    ref_params = [p for m in ref_models for p in m.parameters()]
    own = FlatAdam(own_models, lr=5e-4)
    sd0 = own.state_dict()
    assert sd0["state"] == {} and sd0["param_groups"][0]["params"] == list(range(len(own.params)))
    ref = torch.optim.Adam(ref_params, lr=1e-3)
    ref.load_state_dict(sd0)
    assert ref.param_groups[0]["lr"] == 5e-4 and len(ref.state) == 0
    g = torch.Generator(device="cuda").manual_seed(9)
    grads = [[torch.randn(p.shape, device="cuda", generator=g) * 1e-2 for p in ref_params] for _ in range(3)]

    def step(opt, params, gset):
        opt.zero_grad()
        for p, gr in zip(params, gset):
            p.grad = gr.clone()
        opt.step()
    step(ref, ref_params, grads[0]); step(ref, ref_params, grads[1])
    good = ref.state_dict()
    bad = ref.state_dict()
    bad["state"] = {k: dict(v) for k, v in bad["state"].items()}
    bad["state"][3]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="different step counts"):
        own.load_state_dict(bad)
    own.load_state_dict(good)
    assert own.state2.tolist() == [2, 0]
    with torch.no_grad():
        for po, pr in zip(own.params, ref_params):
            po.copy_(pr)
    step(ref, ref_params, grads[2]); step(own, own.params, grads[2])
    torch.cuda.synchronize()
    assert own.state2.tolist() == [3, 0]
    assert all(bool(((pr.detach() - po.detach()).abs() <= 2.4e-7 * pr.detach().abs() + 2e-8).all()) for pr, po in zip(ref_params, own.params))
    assert all(float(s["step"]) == 3.0 for s in own.state_dict()["state"].values())
