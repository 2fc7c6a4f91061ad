"""GPU tests of the skip grid built from rendered views: ``dmnerf_skip_grid_mark`` / ``dmnerf_skip_grid_dilate`` (csrc/skip.hip),
``field.SkipGrid.mark`` / ``.dilated`` / ``|`` / ``.from_views``, ``render.dm_nerf_fine_mark`` and the ``mark=`` route of the frame
drivers.  The kernels are compared with the numpy restatement (tests/_mark_restate.py, checked on the CPU by
tests/test_mark_restate.py), the renders with the existing dense and skipping product calls.  Bits and rendered values are compared
exactly: there is no tolerance anywhere.  ``frame_rays``, ``random_grid`` and ``words_of`` are the shared ones of tests/_gpu.py."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _gpu
import _mark_restate as RM
from _gpu import A, frame_rays, random_grid, words_of  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

POISON = 0x40000000
# The density head's bias of the models below.  sigma is about 60 everywhere, so a ray is opaque after a short stretch and every
# sample behind it has weight EXACTLY 0 (the transmittance product rounds to 0 in f32): measured on the CPU with the oracle on the
# n = 130 case, 84 % (coarse) and 83 % (fine) of the samples without jitter, 84 % and 60 % with it; the grid marked from them flags
# 22 % / 23 % of the samples (23 % / 45 % with jitter).  (sigma_bias 0.3 of test_gpu_skip.py: 0 % / 3 % exact zeros, nothing to skip.)
SIGMA_BIAS = 60.0
SCENE = ((-12.0, -12.0, -12.0), (12.0, 12.0, 12.0), (32, 32, 32))         # holds every sample of the rays below
KEYS = ("rgb_fine", "ins_fine", "depth_fine", "z_vals_fine", "raw_fine")


_cache = {}


def models(ins_num=13):
    return _gpu.models(ins_num, sigma_bias=SIGMA_BIAS, cache=_cache)


def restate_mark(grid, words, ro, rd, z, w, thr):
    return RM.mark(words, ro.cpu().numpy(), rd.cpu().numpy(), z.cpu().numpy(), w.cpu().numpy(), grid.lo, grid.hi, grid.dims, thr)


def select_flags(A, grid, ro, rd, z):
    """``dmnerf_skip_select`` (pinned against its restatement by test_gpu_skip.py) -> flag [N,S] bool."""
    N, S = z.shape
    L, lib = A.L, A.lib
    flag = torch.full((N, S), 77, dtype=torch.uint8, device="cuda")
    sel = torch.empty(N * S, dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(N * S)), dtype=torch.int32, device="cuda")
    g = grid.c_struct()
    L.check(lib.dmnerf_skip_select(ctypes.byref(g), L.ptr(ro), L.ptr(rd), L.ptr(z.contiguous()), N, S, L.ptr(flag), L.ptr(sel), L.ptr(count),
                                   L.ptr(work), L.stream()), "dmnerf_skip_select")
    return flag != 0


# ---- 1. the mark kernel against the restatement
def mark_inputs(n, s, lo, hi, tau, seed):
    """Rays and weights in which every branch occurs: a point exactly on ``lo`` (inside), one exactly on ``hi`` (outside), a NaN
    point, rays that cross, start in and miss the box, and the weights 0, -0.0, tau, nextafter(tau), NaN and 1."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    size = hi - lo
    o = (lo + (rng.rand(n, 3).astype(np.float32) * 1.4 - 0.2) * size).astype(np.float32)        # some start outside
    d = ((rng.rand(n, 3).astype(np.float32) - 0.4) * size).astype(np.float32)
    z = np.sort(rng.rand(n, s).astype(np.float32) * 1.5, axis=-1)
    special = np.array([0.0, -0.0, tau, np.nextafter(np.float32(tau), np.float32(1)), np.nan, 1.0], np.float32)
    w = np.where(rng.rand(n, s) < 0.5, special[rng.randint(0, 6, size=(n, s))], rng.rand(n, s).astype(np.float32) * np.float32(4 * tau + 1e-3))
    w = w.astype(np.float32)
    o[0], d[0], z[0, 0], w[0, 0] = lo, size, 0.0, 1.0                # exactly on lo: cell (0, 0, 0)
    if s > 1:
        z[0, -1], w[0, -1] = 1.0, 1.0                                # exactly on hi: outside
    if n > 2:
        o[1, 1], w[1] = np.nan, 1.0                                  # NaN points with marking weights: outside
        z[2, s // 2] = np.nan
        w[2, s // 2] = 1.0
    return o, d, z, w


@pytest.mark.parametrize("dims", [(5, 7, 9), (32, 32, 32)])
@pytest.mark.parametrize("n,s", [(1, 1), (3, 5), (7, 64), (130, 192)])
def test_mark_equals_the_restatement(A, n, s, dims):
    lo, hi = (-1.0, -2.0, 0.0), (1.0, 2.0, 3.0)
    cells = dims[0] * dims[1] * dims[2]
    for tau in (0.0, 1e-3):
        pre = random_grid(dims, lo, hi, 0.1, seed=n + s)
        before = words_of(pre).copy()
        o, d, z, w = mark_inputs(n, s, lo, hi, tau, seed=n * s + dims[0])
        want = RM.mark(before, o, d, z, w, lo, hi, dims, tau)
        t = [torch.from_numpy(x).cuda() for x in (o, d, z, w)]
        again = pre.copy()
        assert pre.mark(*t, threshold=tau) is pre
        got = words_of(pre)
        assert np.array_equal(got, want), (tau, np.flatnonzero(got != want)[:8])
        assert np.array_equal(got & before, before)                  # the pre-set bits survive
        assert np.array_equal(words_of(again.mark(*t, threshold=tau)), got)                         # the same words every run
        assert np.array_equal(words_of(pre.mark(*t, threshold=tau)), got)                           # idempotent
        if cells & 31:
            assert int(got[-1]) >> (cells & 31) == 0                 # the unused bits of the last word
        assert got[0] & 1                                            # the point exactly on lo
        if n * s >= 448:
            assert not np.array_equal(got, before) and not np.array_equal(got, words_of(A.F.SkipGrid.full(lo, hi, dims)))
    if (n, s) == (1, 1):
        only = A.F.SkipGrid.empty(lo, hi, dims).mark(*t, threshold=0.0)
        assert words_of(only).tolist()[0] == 1 and not words_of(only)[1:].any()


def test_mark_argument_checks(A):
    L, lib = A.L, A.lib
    grid = random_grid((5, 7, 9), (0, 0, 0), (1, 1, 1), 0.1, seed=1)
    before = grid.bits.clone()
    ro, rd = torch.zeros(4, 3, device="cuda") + 0.5, torch.zeros(4, 3, device="cuda")
    z, w = torch.zeros(4, 8, device="cuda"), torch.ones(4, 8, device="cuda")
    g = grid.c_struct()

    def call(grid_p=ctypes.byref(g), bits=grid.bits, o=ro, zz=z, ww=w, N=4, S=8, thr=0.0):
        return lib.dmnerf_skip_grid_mark(grid_p, L.ptr(bits), L.ptr(o), L.ptr(rd), L.ptr(zz), L.ptr(ww), N, S, thr, L.stream())

    for kw, text in ((dict(grid_p=None), "null grid"), (dict(bits=None), "null pointer"), (dict(o=None), "null pointer"),
                     (dict(zz=None), "null pointer"), (dict(ww=None), "null pointer"), (dict(thr=float("nan")), "threshold"),
                     (dict(thr=-1e-6), "threshold"), (dict(S=0), "S=0"), (dict(N=1 << 20, S=1 << 11), "do not fit")):
        assert call(**kw) == -1 and text in L.last_error(), (kw, L.last_error())
    assert call(N=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(grid.bits, before)                            # nothing was launched
    with pytest.raises(ValueError):
        grid.mark(ro, rd, z, w[:, :7].contiguous())
    with pytest.raises(ValueError):
        grid.mark(ro, rd, z, w, threshold=-1.0)
    with pytest.raises(ValueError):
        grid.mark(ro, rd, z.double(), w)
    with pytest.raises(RuntimeError):
        grid.mark(ro.cpu(), rd, z, w)
    assert call() == 0                                               # the good call marks cell (2, 3, 4) = the point (0.5, 0.5, 0.5)
    cell = (2 * 7 + 3) * 9 + 4
    want = words_of(A.F.SkipGrid.from_bits(before, grid.lo, grid.hi, grid.dims)).copy()
    want[cell >> 5] |= np.uint32(1 << (cell & 31))
    assert np.array_equal(words_of(grid), want)


# ---- 2. dilation of bits, and the algebra of grids
@pytest.mark.parametrize("dims", [(5, 7, 9), (33, 8, 40)])
def test_dilated_equals_the_build_with_that_dilation(A, dims):
    rng = np.random.RandomState(dims[1])
    sig = rng.randn(*dims).astype(np.float32) - np.float32(2.05)             # about 2 % above the threshold 0
    sig.reshape(-1)[rng.choice(sig.size, 2, replace=False)] = np.nan
    sig[0, 0, 0] = sig[-1, -1, -1] = 1.0                                    # two corners
    s = torch.from_numpy(sig).cuda()
    lo, hi = (-1.0, -2.0, 0.0), (1.0, 2.0, 3.0)
    base = A.F.SkipGrid.from_sigma(s, lo, hi, dilate=0, outside="empty")
    keep = base.bits.clone()
    for r in (0, 1, 4):
        got = base.dilated(r)
        want = A.F.SkipGrid.from_sigma(s, lo, hi, dilate=r)
        assert torch.equal(got.bits, want.bits), r
        assert np.array_equal(words_of(got), RM.dilate(words_of(base), dims, r)), r
        assert got.outside == "empty" and got.dims == base.dims and got.bits.data_ptr() != base.bits.data_ptr()
    assert torch.equal(base.bits, keep)
    assert 0 < float(base.occupancy()) < 0.1 < float(base.dilated(1).occupancy()) < 1.0
    L, lib = A.L, A.lib
    out = torch.zeros_like(base.bits)
    assert lib.dmnerf_skip_grid_dilate(L.ptr(base.bits), *dims, 1, L.ptr(base.bits), L.stream()) == -1 and "different buffers" in L.last_error()
    assert lib.dmnerf_skip_grid_dilate(L.ptr(base.bits), *dims, 5, L.ptr(out), L.stream()) == -1 and "0..4" in L.last_error()
    with pytest.raises(RuntimeError):
        base.dilated(5)
    torch.cuda.synchronize()
    assert not bool(out.any()) and torch.equal(base.bits, keep)


def test_or_copy_and_their_refusals(A):
    lo, hi, dims = (0, 0, 0), (1, 1, 1), (5, 7, 9)
    a, b = random_grid(dims, lo, hi, 0.2, seed=3), random_grid(dims, lo, hi, 0.2, seed=4)
    wa, wb = words_of(a).copy(), words_of(b).copy()
    assert np.array_equal(words_of(a | b), wa | wb) and np.array_equal(words_of(a), wa)
    assert np.array_equal(words_of(a | A.F.SkipGrid.empty(lo, hi, dims)), wa)                     # empty is neutral
    c = a.copy()
    assert c.bits.data_ptr() != a.bits.data_ptr() and np.array_equal(words_of(c), wa)
    ptr = c.bits.data_ptr()
    c |= b
    assert c.bits.data_ptr() == ptr and np.array_equal(words_of(c), wa | wb) and np.array_equal(words_of(a), wa)
    for other in (random_grid((5, 7, 8), lo, hi, 0.2, seed=5), random_grid(dims, lo, (1, 1, 2), 0.2, seed=5),
                  random_grid(dims, lo, hi, 0.2, seed=5, outside="empty")):
        with pytest.raises(ValueError):
            a | other
        with pytest.raises(ValueError):
            a.__ior__(other)


# ---- 3. the marking render
def render_case(A, perturb=False, n=130, split=None):
    ro, rd = frame_rays(n, start=90000)
    z = A.H.z_val_sample(n, 4.0, 15.0, 64, device="cuda")
    args = types.SimpleNamespace(perturb=1.0 if perturb else False, N_importance=128, is_train=False, N_ins=None)
    if split:
        args.mfma_split = split
    g = torch.Generator().manual_seed(5)
    draws = dict(t_rand=torch.rand(n, 64, generator=g).cuda(), u=torch.rand(n, 128, generator=g).cuda()) if perturb else {}
    return ro, rd, z, args, draws


def dense_weights(A, mc, ro, rd, z, out, t_rand=None):
    """The two (depths, weights) pairs of a dense render from the existing product calls: the fine one from ``render_train`` of the
    returned ``raw_fine``, the coarse one as ``restate_render`` of test_gpu_skip.py recomputes it (density, ``dmnerf_weights_from_sigma``)."""
    L, lib = A.L, A.lib
    n, s = z.shape
    w_f = A.R.render_train(out["raw_fine"], out["z_vals_fine"], rd)[1]
    z_c = A.H.stratify(z, t_rand) if t_rand is not None else z
    sigma = torch.empty(n, s, device="cuda")
    L.check(lib.dmnerf_mlp_fwd_rays_density(L.ptr(mc.blob()), mc.ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z_c), n, s, L.ptr(sigma), L.stream()), "density")
    w_c = torch.empty(n, s, device="cuda")
    L.check(lib.dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z_c), L.ptr(rd), n, s, L.ptr(w_c), L.stream()), "weights")
    return (out["z_vals_fine"], w_f), (z_c, w_c)


_render_cache = {}


def marked_case(A, perturb, tau=0.0):
    """The n = 130 case rendered dense and by ``dm_nerf_fine_mark`` at both levels (computed once per (perturb, tau))."""
    key = (perturb, tau)
    if key not in _render_cache:
        mc, mf = models()
        ro, rd, z, args, draws = render_case(A, perturb)
        grid = A.F.SkipGrid.empty(*SCENE)
        with torch.no_grad():
            dense = A.R.dm_nerf_fine(torch.stack([ro, rd]), None, None, mc, mf, z, args, **draws)
            got = A.R.dm_nerf_fine_mark(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid, threshold=tau, **draws)
            pairs = dense_weights(A, mc, ro, rd, z, dense, draws.get("t_rand"))
        _render_cache[key] = types.SimpleNamespace(ro=ro, rd=rd, z=z, args=args, draws=draws, grid=grid, dense=dense, got=got, fine=pairs[0],
                                                   coarse=pairs[1])
    return _render_cache[key]


@pytest.mark.parametrize("perturb", [False, True])
def test_marking_render_leaves_the_render_alone_and_marks_what_it_used(A, perturb):
    mc, mf = models()
    c = marked_case(A, perturb)
    assert set(c.got) == set(KEYS)
    for k in KEYS:
        assert torch.equal(c.got[k], c.dense[k]), k
    empty = np.zeros(c.grid.n_words, np.uint32)
    want_f = restate_mark(c.grid, empty, c.ro, c.rd, *c.fine, 0.0)
    want = restate_mark(c.grid, want_f, c.ro, c.rd, *c.coarse, 0.0)
    assert np.array_equal(words_of(c.grid), want)
    assert want.any() and want_f.any()
    for levels, w in ((("fine",), want_f), (("coarse",), restate_mark(c.grid, empty, c.ro, c.rd, *c.coarse, 0.0))):
        g = A.F.SkipGrid.empty(*SCENE)
        with torch.no_grad():
            A.R.dm_nerf_fine_mark(torch.stack([c.ro, c.rd]), None, None, mc, mf, c.z, c.args, g, levels=levels, **c.draws)
        assert np.array_equal(words_of(g), w), levels
    if perturb:
        assert not torch.equal(c.coarse[0], c.z)                     # the coarse level was marked at the JITTERED depths
    with pytest.raises(ValueError):
        A.R.dm_nerf_fine_mark(torch.stack([c.ro, c.rd]), None, None, mc, mf, c.z, c.args, c.grid, levels=("medium",))
    with pytest.raises(TypeError):
        A.R.dm_nerf_fine_mark(torch.stack([c.ro, c.rd]), None, None, mc, mf, c.z, c.args, None)
    bad = types.SimpleNamespace(**{**vars(c.args), "mfma_split": "bf16x3"})
    with pytest.raises(ValueError):
        A.R.dm_nerf_fine_mark(torch.stack([c.ro, c.rd]), None, None, mc, mf, c.z, bad, c.grid)


# ---- 4. the guarantee: re-rendering the marked views through the grid at threshold 0 is the dense render, bit for bit
@pytest.mark.parametrize("case", ["both", "fine_only", "perturb", "f16x2"])
def test_skip_render_through_the_marked_grid_equals_the_dense_render(A, case):
    """With ``sigma_bias = 60`` the dense render alone leaves well over a quarter of the samples with weight exactly 0 (asserted
    below on the device's own weights; on the CPU with the oracle: 84 % coarse / 83 % fine, with jitter 84 % / 60 %), so the grid
    leaves samples out and the equality is not vacuous: ``0 < n_eval <= 0.75 N S`` at every level that is skipped."""
    mc, mf = models()
    perturb = case == "perturb"
    levels = ("fine",) if case == "fine_only" else ("coarse", "fine")
    if case == "f16x2":
        ro, rd, z, args, draws = render_case(A, split="f16x2")
        grid = A.F.SkipGrid.empty(*SCENE)
        with torch.no_grad():
            dense = A.R.dm_nerf_fine_f16(torch.stack([ro, rd]), None, None, mc, mf, z, args)
            marked = A.R.dm_nerf_fine_mark(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid)
        for k in KEYS:
            assert torch.equal(marked[k], dense[k]), k
        w_f = A.R.render_train(dense["raw_fine"], dense["z_vals_fine"], rd)[1]
    else:
        c = marked_case(A, perturb)
        ro, rd, z, args, draws, dense = c.ro, c.rd, c.z, c.args, c.draws, c.dense
        w_f = c.fine[1]
        assert float((c.coarse[1] == 0).float().mean()) >= 0.25
        if case == "fine_only":
            grid = A.F.SkipGrid.empty(*SCENE)
            with torch.no_grad():
                A.R.dm_nerf_fine_mark(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid, levels=levels)
        else:
            grid = c.grid
    assert float((w_f == 0).float().mean()) >= 0.25
    with torch.no_grad():
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid, levels=levels, **draws)
    for k in ("rgb_fine", "ins_fine", "depth_fine", "z_vals_fine"):
        assert torch.equal(got[k], dense[k]), k
    flag = select_flags(A, grid, ro, rd, dense["z_vals_fine"])
    assert torch.equal(got["raw_fine"], torch.where(flag[..., None], dense["raw_fine"], torch.zeros_like(dense["raw_fine"])))
    n_eval = got["n_eval"].tolist()
    n = z.shape[0]
    print(f"{case}: n_eval {n_eval} of {[n * 64, n * 192]}, dense weights exactly 0: fine {float((w_f == 0).float().mean()):.3f}")
    assert n_eval[1] == int(flag.sum()) and 0 < n_eval[1] <= 0.75 * n * 192
    if "coarse" in levels:
        assert 0 < n_eval[0] <= 0.75 * n * 64
    else:
        assert n_eval[0] == n * 64


# ---- 5. threshold > 0: what is left out had a dense weight <= threshold
def test_positive_threshold_leaves_out_only_weights_up_to_it(A):
    tau = 1e-3
    c0, c = marked_case(A, False), marked_case(A, False, tau)
    for k in KEYS:
        assert torch.equal(c.got[k], c.dense[k]), k
    w0, w = words_of(c0.grid), words_of(c.grid)
    assert np.array_equal(w & w0, w) and w.any() and not np.array_equal(w, w0)           # a strict subset of the threshold-0 grid
    for z_l, w_l in (c.fine, c.coarse):
        flag = select_flags(A, c.grid, c.ro, c.rd, z_l)
        left_out = w_l[~flag]
        assert left_out.numel() and bool((left_out <= tau).all())
        assert bool((w_l[flag] > tau).any())
    flag = select_flags(A, c.grid, c.ro, c.rd, c.fine[0])
    assert bool((c.fine[1][~flag] > 0).any())                        # (it does leave out samples the threshold-0 grid keeps)


# ---- 6. the frame drivers
def frame_setup(A, chunk):
    mc, mf = models()
    K = O.dmsr_intrinsics(480, 640)
    c2w = O.pose_spherical(30.0, -65.0, 7.0).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, N_test=chunk, N_samples=64, near=4.0, far=15.0)
    return mc, mf, K, c2w, args


N_FRAME = 192            # rays of the restricted frame: chunk 96 = two whole chunks, chunk 100 leaves a ragged chunk of 92


def few_rows(A):
    """``raygen=`` that restricts the 480 x 640 pose to the first ``N_FRAME`` pixels of image row 240."""
    def raygen(H, W, K, c2w, row0, nrows):
        ro, rd = A.H.get_rays_k(H, W, K, c2w, row0=240, nrows=1)
        return ro.reshape(-1, 3)[:N_FRAME].contiguous(), rd.reshape(-1, 3)[:N_FRAME].contiguous()
    return raygen


@pytest.mark.parametrize("chunk", [96, 100])
def test_frame_with_mark_is_the_dense_frame_and_marks_every_chunk(A, chunk):
    mc, mf, K, c2w, args = frame_setup(A, chunk)
    raygen = few_rows(A)
    g = A.F.SkipGrid.empty(*SCENE)
    with torch.no_grad():
        dense = A.D.render_frame(480, 640, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64, raygen=raygen)
        dense = [t.reshape(480 * 640, -1)[:N_FRAME].clone() for t in dense]
        got = A.D.render_frame(480, 640, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64, raygen=raygen, mark=g)
        got = [t.reshape(480 * 640, -1)[:N_FRAME].clone() for t in got]
        for a, b in zip(got, dense):
            assert torch.equal(a, b)
        ro, rd = raygen(480, 640, K, c2w, 0, 480)
        want = np.zeros(g.n_words, np.uint32)
        for s0 in range(0, N_FRAME, chunk):
            e = min(s0 + chunk, N_FRAME)
            o, d = ro[s0:e].contiguous(), rd[s0:e].contiguous()
            z = A.H.z_val_sample(e - s0, 4.0, 15.0, 64, device="cuda")
            out = A.R.dm_nerf_fine(torch.stack([o, d]), None, None, mc, mf, z, args)
            for z_l, w_l in dense_weights(A, mc, o, d, z, out):
                want = restate_mark(g, want, o, d, z_l, w_l, 0.0)
    assert np.array_equal(words_of(g), want) and want.any()
    if chunk == 96:
        with pytest.raises(ValueError, match="skip="):
            A.D.render_frame(480, 640, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, raygen=raygen, mark=g, skip=A.F.SkipGrid.full(*SCENE))
        with pytest.raises(ValueError, match="render_chunk="):
            A.D.render_frame(480, 640, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, raygen=raygen, mark=g,
                             render_chunk=lambda *a, **k: None)


def test_from_views_is_the_or_of_the_single_pose_grids(A):
    H, W = 20, 24
    mc, mf = models()
    K = np.array([[30.0, 0, W / 2], [0, -30.0, H / 2], [0, 0, -1]])
    poses = [O.pose_spherical(30.0, -65.0, 7.0).cuda(), O.pose_spherical(75.0, -40.0, 7.0).cuda()]
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, N_test=100, N_samples=64, near=4.0, far=15.0)
    lo, hi, dims = SCENE
    with torch.no_grad():
        one = [A.F.SkipGrid.from_views([p], (H, W, K), (mc, mf), args, lo, hi, dims=dims, chunk=100) for p in poses]
        both = A.F.SkipGrid.from_views(poses, (H, W, K), (mc, mf), args, lo, hi, dims=dims, chunk=100)
        dil = A.F.SkipGrid.from_views(poses, (H, W, K), (mc, mf), args, lo, hi, dims=dims, chunk=100, dilate=1, outside="empty")
        tau = A.F.SkipGrid.from_views(poses, (H, W, K), (mc, mf), args, lo, hi, dims=dims, chunk=100, threshold=1e-3, levels=("fine",))
    assert torch.equal(both.bits, (one[0] | one[1]).bits)
    assert not torch.equal(one[0].bits, one[1].bits) and bool(one[0].bits.any()) and bool(one[1].bits.any())
    assert torch.equal(dil.bits, both.dilated(1).bits) and dil.outside == "empty" and both.outside == "evaluate"
    assert torch.equal(tau.bits & both.bits, tau.bits) and not torch.equal(tau.bits, both.bits) and bool(tau.bits.any())


# ---- 7. capture
def test_captured_marking_render_gives_the_eager_words(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A, n=96)
    rays = torch.stack([ro, rd])
    eager_grid, grid = A.F.SkipGrid.empty(*SCENE), A.F.SkipGrid.empty(*SCENE)
    with torch.no_grad():
        eager = A.R.dm_nerf_fine_mark(rays, None, None, mc, mf, z, args, eager_grid)            # (also the warm-up of every kernel)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = A.R.dm_nerf_fine_mark(rays, None, None, mc, mf, z, args, grid)
        for _ in range(2):
            grid.bits.zero_()                                        # cleared in place: the capture holds the pointer
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(grid.bits, eager_grid.bits)
            for k in KEYS:
                assert torch.equal(out[k], eager[k]), k
    assert bool(eager_grid.bits.any())
