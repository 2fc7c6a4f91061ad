"""GPU tests of the manipulation render that skips empty space: ``dmnerf_skip_select_fill`` (csrc/skip.hip), ``render.run_network_skip``,
``manipulator(..., skip=grid)`` and the ``skip=`` route of ``ManipulationFrameRenderer`` / ``manipulate_frame`` / the path drivers.

A skipped sample's row is the EMPTY ROW E = (0, 0, 0, 0 | 0, .., 0, 1) and an evaluated row is the dense call's bit for bit, so the
result is by definition the dense chain with those rows replaced: every comparison is ``torch.equal`` against the restatement of
tests/_manip_skip_restate.py (dense public pieces + ``fill_rows`` with the numpy select's flags).  There is no tolerance anywhere."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

import _gpu
import _manip_skip_restate as MR
import _skip_restate as RS
from _gpu import A  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

POISON = 0x40000000
N, NS, NI = 130, 8, 8                   # rays (no multiple of a wave or of a 32-sample tile), coarse samples, importance samples
DIMS = (9, 11, 10)                      # 990 cells: 30 full words and 30 bits of the last one


_models = {}


def models(ins_num=13, power=False):
    key = (ins_num, power)
    if key not in _models:
        _models[key] = _gpu.models(ins_num, state_dicts=MR.power_weights(O) if power else None)
    return _models[key]


def product_grid(A, spec):
    return A.F.SkipGrid.from_bits(spec.words, spec.lo, spec.hi, spec.dims, outside=spec.outside)


def make_args(labels, split=None, chunk=4096):
    a = types.SimpleNamespace(N_samples=NS, N_importance=NI, near=MR.NEAR, far=MR.FAR, N_test=chunk, target_labels=list(labels))
    if split:
        a.mfma_split = split
    return a


# the five configurations of tests 2 and 3: (name, T_r target ray sets, target_labels, kinds, keep_labels)
def configs(A):
    MA = A.MA
    return {"ref_T1": (1, [2], None, None), "ref_T2": (2, [2, 4], None, None),
            "move_copy": (2, [2, 4], [MA.MOVE, MA.COPY], None), "remove": (0, [3], [MA.REMOVE], None),
            "keep_only": (0, [], None, [1, 2, 5])}


CONFIGS = ("ref_T1", "ref_T2", "move_copy", "remove", "keep_only")
_rays = {}


def rays_and_draws(T):
    if T not in _rays:
        ori, tars = MR.case_rays(O, N, T)
        _rays[T] = (ori.cuda(), [t.cuda() for t in tars], [u.cuda() for u in MR.case_draws(N, NI, 2 + T)])
    return _rays[T]


def run_product(A, mc, mf, name, args, **kw):
    T, labels, kinds, keep = configs(A)[name]
    ori, tars, us = rays_and_draws(T)
    a = copy.copy(args)
    a.target_labels = labels
    with torch.no_grad():
        return A.MA.manipulator(None, None, mc, mf, ori, tars, a, us=us, kinds=kinds, keep_labels=keep, **kw)


def run_restated(A, mc, mf, name, args, spec, levels, zero_rows=False, split=None):
    T, labels, kinds, keep = configs(A)[name]
    ori, tars, us = rays_and_draws(T)
    a = copy.copy(args)
    a.target_labels = labels
    net = MR.Net(A.MA, mc, mf, a, spec, levels, zero_rows=zero_rows, split=split)
    with torch.no_grad():
        out = MR.chain(A.MA, A.H, net, ori, tars, a, us, kinds=kinds, keep_labels=keep)
    return out, net


def assert_same(got, want, what=""):
    assert len(got) == len(want) == 4
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), (what, i)


# ---- 1. the select-and-fill kernel against the restatement
def select_fill(A, grid, ro, rd, z, width, rows=True, totals=None):
    n, s = z.shape
    L, lib = A.L, A.lib
    flag = torch.full((n, s), 77, dtype=torch.uint8, device="cuda")
    sel = torch.full((n * s,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(n * s)), dtype=torch.int32, device="cuda")
    buf = None
    if rows:
        # a NaN pattern that differs from float to float, with one guard row behind the buffer
        pat = (0x7FC00000 + torch.arange((n * s + 1) * width, dtype=torch.int64) % 0x10000).to(torch.int32)
        buf = pat.view(torch.float32).reshape(n * s + 1, width).cuda()
    fill = MR.empty_row(width - 4).cuda()
    g = grid.c_struct()
    L.check(lib.dmnerf_skip_select_fill(ctypes.byref(g), L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(flag), L.ptr(sel), L.ptr(count),
                                        L.ptr(work), L.ptr(buf), L.ptr(fill), width, L.ptr(totals), L.stream()), "dmnerf_skip_select_fill")
    assert int(count[1]) == POISON
    return flag, sel, count[:1], buf


def select_plain(A, grid, ro, rd, z):
    n, s = z.shape
    L, lib = A.L, A.lib
    flag = torch.full((n, s), 77, dtype=torch.uint8, device="cuda")
    sel = torch.full((n * s,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(n * s)), dtype=torch.int32, device="cuda")
    g = grid.c_struct()
    L.check(lib.dmnerf_skip_select(ctypes.byref(g), L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(flag), L.ptr(sel), L.ptr(count),
                                   L.ptr(work), L.stream()), "dmnerf_skip_select")
    return flag, sel, count[:1]


def kernel_rays(n, s, seed):
    """Rays of the shared case (crossing, entering and missing the box) with sorted random depths; one NaN depth."""
    ori, _ = MR.case_rays(O, n, 0, start=4000 + seed)
    g = torch.Generator().manual_seed(seed)
    z = (MR.NEAR + (MR.FAR - MR.NEAR) * torch.rand(n, s, generator=g)).sort(-1).values
    if n * s > 20:
        z[n // 2, s // 2] = float("nan")
    return ori[0].contiguous(), ori[1].contiguous(), z


@pytest.mark.parametrize("outside", ["evaluate", "empty"])
@pytest.mark.parametrize("n,s", [(1, 1), (130, 8), (33, 24), (7, 321)])
def test_select_fill_equals_the_restatement(A, n, s, outside):
    o, d, z = kernel_rays(n, s, seed=n + s)
    ro, rd, zz = o.cuda(), d.cuda(), z.cuda()
    specs = {"random": MR.random_spec(DIMS, 0.3, 11, outside), "empty": MR.GridSpec(np.zeros(DIMS, bool), MR.BOX_LO, MR.BOX_HI, outside),
             "full": MR.GridSpec(np.ones(DIMS, bool), MR.BOX_LO, MR.BOX_HI, outside)}
    for name, spec in specs.items():
        grid = product_grid(A, spec)
        want_flag, want_sel, want_count = RS.select(o.numpy(), d.numpy(), z.numpy(), spec.words, spec.lo, spec.hi, spec.dims, outside)
        keep = torch.from_numpy(want_flag.reshape(-1) != 0)
        for width in (6, 18, 98):
            totals = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
            flag, sel, count, buf = select_fill(A, grid, ro, rd, zz, width, totals=totals)
            assert torch.equal(flag.cpu(), torch.from_numpy(want_flag)), (name, width)
            assert int(count) == want_count and torch.equal(sel[:want_count].cpu(), torch.from_numpy(want_sel))
            assert bool((sel[want_count:] == POISON).all())
            assert totals.tolist() == [5 + want_count, 7 + n * s]
            pat = (0x7FC00000 + torch.arange((n * s + 1) * width, dtype=torch.int64) % 0x10000).to(torch.int32).reshape(n * s + 1, width)
            got = buf.cpu()
            bits = got.view(torch.int32)
            assert torch.equal(bits[:-1][keep], pat[:-1][keep]), (name, width)          # flagged rows keep the NaN pattern, bit for bit
            assert torch.equal(bits[-1], pat[-1])                                      # nothing behind the last row
            assert bool((got[:-1][~keep] == MR.empty_row(width - 4)).all()), (name, width)  # clear rows are E
        # d_rows = NULL is dmnerf_skip_select
        f0, s0, c0, _ = select_fill(A, grid, ro, rd, zz, 18, rows=False)
        f1, s1, c1 = select_plain(A, grid, ro, rd, zz)
        assert torch.equal(f0, f1) and torch.equal(s0, s1) and torch.equal(c0, c1)
        if name == "random" and n * s >= 700:
            assert 0 < want_count < n * s
        if name == "empty" and outside == "empty":
            assert want_count == 0
        if name == "full" and outside == "evaluate":
            assert want_count == n * s                                                 # (the NaN sample is outside: evaluated)


def test_select_fill_refuses_2_31_samples_without_a_launch(A):
    lib = A.lib
    g = A.F.SkipGrid.empty((0, 0, 0), (1, 1, 1), 2).c_struct()
    rc = lib.dmnerf_skip_select_fill(ctypes.byref(g), None, None, None, 1 << 20, 1 << 11, None, None, None, None, None, None, 18, None, None)
    assert rc == -1 and "int32" in A.L.last_error()
    rc = lib.dmnerf_skip_select_fill(ctypes.byref(g), None, None, None, 4, 0, None, None, None, None, None, None, 18, None, None)
    assert rc == -1
    rc = lib.dmnerf_skip_select_fill(ctypes.byref(g), None, None, None, 4, 4, None, None, None, None, None, None, 18, None, None)
    assert rc == -1 and "null" in A.L.last_error()
    with pytest.raises(ValueError, match="int32"):
        mc, _ = models()
        z = torch.zeros(1, 1, device="cuda").expand(1 << 20, 1 << 11)                  # (a view: no 8 GiB of depths)
        A.R.run_network_skip(mc, torch.zeros(1 << 20, 3, device="cuda"), torch.zeros(1 << 20, 3, device="cuda"), z,
                             A.F.SkipGrid.empty((0, 0, 0), (1, 1, 1), 2))


# ---- 2. a full grid is the dense call
@pytest.mark.parametrize("name", CONFIGS)
def test_full_grid_equals_the_dense_manipulator(A, name):
    mc, mf = models()
    a = make_args([])
    grid = A.F.SkipGrid.full(MR.BOX_LO, MR.BOX_HI, DIMS)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = run_product(A, mc, mf, name, a)
    got = run_product(A, mc, mf, name, a, skip=grid, skip_counts=counts)
    assert_same(got, want, name)
    assert counts[0].item() == counts[1].item() > 0
    assert float(want[0].abs().max()) > 0


# ---- 3. a random grid is the restated chain with E rows
@pytest.mark.parametrize("outside", ["evaluate", "empty"])
@pytest.mark.parametrize("levels", [("coarse", "fine"), ("fine",)])
@pytest.mark.parametrize("name", CONFIGS)
def test_random_grid_equals_the_restated_chain(A, name, levels, outside):
    mc, mf = models()
    a = make_args([])
    spec = MR.random_spec(DIMS, 0.3, 21, outside)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = run_product(A, mc, mf, name, a, skip=product_grid(A, spec), skip_levels=levels, skip_counts=counts)
    want, net = run_restated(A, mc, mf, name, a, spec, levels)
    assert_same(got, want, (name, levels, outside))
    assert counts.tolist() == net.counts and 0 < net.counts[0] < net.counts[1]
    dense = run_product(A, mc, mf, name, a)
    assert not torch.equal(dense[0], got[0])                                           # the grid really took samples away


# ---- 4. a skipped sample is never the moved object
def test_a_skipped_sample_is_never_the_moved_object(A):
    """Moving object 0 (``target_labels = [0]``, T = 1) through a ~30 % grid: the result is the restated chain with E rows, and NOT the
    restated chain with all-zero rows -- an all-zero target row has argmax 0, reads as the moved object and overwrites real rows of
    the original.  The case (tests/_manip_skip_restate.POWER: ``ins_linear.bias[0] += 0.2`` on the make_weights models, so that object
    0 wins the accumulated label on most rays while per-sample labels still vary) was chosen on the CPU with the oracle's
    ``manipulator``: there the two variants differ by more than 1e-3 on 96 of the 130 rays
    (tests/test_manip_skip_restate.py::test_the_power_case_tells_empty_rows_from_zero_rows_on_the_oracle)."""
    P = MR.POWER
    mc, mf = models(P["ins_num"], power=True)
    a = make_args([P["label"]])
    spec = MR.random_spec(P["dims"], P["frac"], P["grid_seed"], P["outside"])
    ori, tars, us = rays_and_draws(1)
    with torch.no_grad():
        got = A.MA.manipulator(None, None, mc, mf, ori, tars, a, us=us, skip=product_grid(A, spec))
        want = MR.chain(A.MA, A.H, MR.Net(A.MA, mc, mf, a, spec, ("coarse", "fine")), ori, tars, a, us)
        naive = MR.chain(A.MA, A.H, MR.Net(A.MA, mc, mf, a, spec, ("coarse", "fine"), zero_rows=True), ori, tars, a, us)
    differ = (want[0] != naive[0]).any(-1) | (want[1] != naive[1]).any(-1)
    print(f"power: {int(differ.sum())} of {N} rays differ between E rows and zero rows")
    assert int(differ.sum()) >= 1                                                      # the power condition: the case can tell them apart
    assert_same(got, want, "power")
    assert not (torch.equal(got[0], naive[0]) and torch.equal(got[1], naive[1]))


# ---- 5. an empty grid
@pytest.mark.parametrize("name", ["ref_T1", "ref_T2", "move_copy"])
def test_empty_grid_evaluates_nothing(A, name):
    mc, mf = models()
    a = make_args([])
    spec = MR.GridSpec(np.zeros(DIMS, bool), MR.BOX_LO, MR.BOX_HI, "empty")
    grid = product_grid(A, spec)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    got = run_product(A, mc, mf, name, a, skip=grid, skip_counts=counts)
    want, net = run_restated(A, mc, mf, name, a, spec, ("coarse", "fine"))
    assert_same(got, want, name)
    C = 14
    for raw in net.raws:
        assert bool((raw == MR.empty_row(C).cuda()).all())
    T = configs(A)[name][0]
    merged = NS + NI + NI * T
    if name.startswith("ref"):         # the reference form: 2 + 4 T launches (the original's merged rows once per object)
        samples = N * (NS + (NS + NI) + T * (NS + (NS + NI)) + 2 * T * merged)
    else:                              # the edit form: the original's merged rows once
        samples = N * (NS + (NS + NI) + T * (NS + (NS + NI)) + (1 + T) * merged)
    assert counts.tolist() == [0, samples] and net.counts == [0, samples]
    ori, _, _ = rays_and_draws(T)
    z = A.MA.manipulator_z(N, MR.NEAR, MR.FAR, NS, "cuda")
    with torch.no_grad():
        raw = A.R.run_network_skip(mf, ori[0], ori[1], z, grid)
    assert raw.shape == (N, NS, 4 + C) and bool((raw == MR.empty_row(C).cuda()).all())


# ---- 6. f16x2
def test_f16x2_full_and_random_grid(A):
    mc, mf = models()
    a = make_args([], split="f16x2")
    for name in ("ref_T1", "move_copy"):
        want = run_product(A, mc, mf, name, a)
        got = run_product(A, mc, mf, name, a, skip=A.F.SkipGrid.full(MR.BOX_LO, MR.BOX_HI, DIMS))
        assert_same(got, want, ("f16 full", name))
        spec = MR.random_spec(DIMS, 0.3, 23, "empty")
        got = run_product(A, mc, mf, name, a, skip=product_grid(A, spec))
        want_r, net = run_restated(A, mc, mf, name, a, spec, ("coarse", "fine"), split="f16x2")
        assert_same(got, want_r, ("f16 random", name))
        assert 0 < net.counts[0] < net.counts[1]
    f32 = run_product(A, mc, mf, "ref_T1", make_args([]))
    assert not torch.equal(f32[0], run_product(A, mc, mf, "ref_T1", a)[0])            # (the f16x2 kernels really ran)


# ---- 7. refusals
def test_refusals(A):
    mc, mf = models()
    grid = A.F.SkipGrid.full(MR.BOX_LO, MR.BOX_HI, DIMS)
    with pytest.raises(ValueError, match="bf16x3"):
        run_product(A, mc, mf, "ref_T1", make_args([], split="bf16x3"), skip=grid)
    narrow = A.M.DM_NeRF(4, 64, 63, 27, [2], 13).cuda().eval()
    assert not narrow._fused_ok()
    with pytest.raises(ValueError, match="8 x 256"):
        run_product(A, narrow, narrow, "ref_T1", make_args([]), skip=grid)
    ori, _, _ = rays_and_draws(1)
    z = A.MA.manipulator_z(N, MR.NEAR, MR.FAR, NS, "cuda")
    with pytest.raises(ValueError, match="8 x 256"):
        A.R.run_network_skip(narrow, ori[0], ori[1], z, grid)
    with pytest.raises(ValueError, match="bf16x3"):
        A.R.run_network_skip(mc, ori[0], ori[1], z, grid, split="bf16x3")
    on_cpu = copy.copy(grid)
    on_cpu.bits = grid.bits.cpu()
    with pytest.raises(RuntimeError):
        A.R.run_network_skip(mc, ori[0], ori[1], z, on_cpu)
    with pytest.raises(RuntimeError):
        run_product(A, mc, mf, "ref_T1", make_args([]), skip=on_cpu)
    for bad in ((), ("coarse", "medium"), "both"):
        with pytest.raises(ValueError, match="levels"):
            run_product(A, mc, mf, "ref_T1", make_args([]), skip=grid, skip_levels=bad)
    K, pose, trans = frame_scene()
    with pytest.raises(ValueError, match="manipulate_chunk"):
        A.D.ManipulationFrameRenderer(FH, FW, K, pose.cuda(), trans[:1], (mc, mf), make_args([2], chunk=50), skip=grid,
                                      manipulate_chunk=lambda *a_: None)
    with pytest.raises(ValueError, match="levels"):
        A.D.ManipulationFrameRenderer(FH, FW, K, pose.cuda(), trans[:1], (mc, mf), make_args([2], chunk=50), skip=grid, skip_levels=("x",))


# ---- 8. the frame
FH, FW, CHUNK = 10, 13, 50             # 130 rays: two whole chunks and a ragged one of 30


def frame_scene():
    K = np.array([[15.0, 0, FW / 2], [0, -15.0, FH / 2], [0, 0, -1]])
    pose = O.pose_spherical(30.0, -65.0, 7.0)
    ang = 0.2
    trans = [torch.tensor([[np.cos(ang), -np.sin(ang), 0., 0.3], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]],
                          dtype=torch.float32)]
    return K, pose, trans


def test_frame_with_skip_equals_the_per_chunk_restatement(A):
    mc, mf = models()
    K, pose, trans = frame_scene()
    a = make_args([2], chunk=CHUNK)
    spec = MR.random_spec(DIMS, 0.3, 25, "evaluate")
    grid = product_grid(A, spec)
    n_chunks = -(-FH * FW // CHUNK)
    gen = torch.Generator().manual_seed(9)
    us = [[torch.rand(min(CHUNK, FH * FW - c * CHUNK), NI, generator=gen).cuda() for _ in range(3)] for c in range(n_chunks)]

    def draws_from(calls):
        def draws(n, n_imp, count, dev):
            calls.append(n)
            return us[len(calls) - 1]
        return draws
    with torch.no_grad():
        fr = A.D.ManipulationFrameRenderer(FH, FW, K, pose.cuda(), trans, (mc, mf), a, draws=draws_from([]), skip=grid)
        for c in range(fr.n_chunks):
            fr.step(c)
        frame = fr.gather()
        ro, rd = A.H.get_rays_k(FH, FW, K, pose.cuda())
        to, td = A.H.get_rays_k(FH, FW, K, A.D._matmul4_f32(trans[0], pose).cuda())
        ro, rd, to, td = [t.reshape(-1, 3) for t in (ro, rd, to, td)]
        cols, total = [[], [], [], []], [0, 0]
        for c, s in enumerate(range(0, FH * FW, CHUNK)):
            e = min(s + CHUNK, FH * FW)
            net = MR.Net(A.MA, mc, mf, a, spec, ("coarse", "fine"))
            out = MR.chain(A.MA, A.H, net, torch.stack([ro[s:e], rd[s:e]]).contiguous(), [torch.stack([to[s:e], td[s:e]]).contiguous()], a, us[c])
            for col, t in zip(cols, out):
                col.append(t)
            total = [total[0] + net.counts[0], total[1] + net.counts[1]]
        for got, col in zip(frame, cols):
            want = torch.cat(col, 0).reshape(FH, FW, -1)
            assert got.shape == want.shape and torch.equal(got, want)
        # the counts: 2 + 4 T launches of 8, 16, 8, 16, 24, 24 samples per ray
        assert fr.n_eval.dtype == torch.int64 and fr.n_eval.tolist() == total
        assert total[1] == FH * FW * (NS + 2 * (NS + NI) + NS + 2 * (NS + 2 * NI)) and 0 < total[0] <= total[1]
        # bands of a world of 1 and of 3, rendered by one process: the concatenation is the frame, bit for bit
        for world in (1, 3):
            bands = [A.D.manipulate_frame(FH, FW, K, pose.cuda(), trans, (mc, mf), a, draws=draws_from([]), skip=grid, rank=r, world=world)
                     for r in range(world)]
            for i in range(4):
                assert torch.equal(torch.cat([b[i] for b in bands], 0), frame[i]), (world, i)
        # a deformation and a removal go through with the grid; the full grid gives the dense frame
        edits = [A.Ed.Deform("ex", 0), A.Ed.Remove()]
        a2 = make_args([2, 4], chunk=CHUNK)
        us2 = [[torch.rand(min(CHUNK, FH * FW - c * CHUNK), NI, generator=gen).cuda() for _ in range(3)] for c in range(n_chunks)]

        def draws2(calls):
            def draws(n, n_imp, count, dev):
                calls.append(n)
                return us2[len(calls) - 1]
            return draws
        dense = A.D.manipulate_frame(FH, FW, K, pose.cuda(), edits, (mc, mf), a2, draws=draws2([]))
        full = A.D.manipulate_frame(FH, FW, K, pose.cuda(), edits, (mc, mf), a2, draws=draws2([]),
                                    skip=A.F.SkipGrid.full(MR.BOX_LO, MR.BOX_HI, DIMS))
        some = A.D.manipulate_frame(FH, FW, K, pose.cuda(), edits, (mc, mf), a2, draws=draws2([]), skip=grid)
        for i in range(4):
            assert torch.equal(dense[i], full[i]), i
        assert bool(torch.isfinite(torch.cat([t.reshape(-1) for t in some])).all()) and not torch.equal(some[0], dense[0])
        # ... and under the partial grid it is the restated edit chain, chunk by chunk.  The deformed object's target rays are the
        # original pose's with the origin's x shifted by the row's offset, summed in f64 and rounded once
        off = torch.from_numpy(A.Ed.deform_offsets(FH, "ex", 0)).cuda().repeat_interleave(FW)
        to = ro.clone()
        to[:, 0] = (ro[:, 0].double() + off).float()
        cols = [[], [], [], []]
        for c, s in enumerate(range(0, FH * FW, CHUNK)):
            e = min(s + CHUNK, FH * FW)
            net = MR.Net(A.MA, mc, mf, a2, spec, ("coarse", "fine"))
            out = MR.chain(A.MA, A.H, net, torch.stack([ro[s:e], rd[s:e]]).contiguous(), [torch.stack([to[s:e], rd[s:e]]).contiguous()], a2,
                           us2[c], kinds=[A.MA.MOVE, A.MA.REMOVE])
            for col, t in zip(cols, out):
                col.append(t)
        for i, col in enumerate(cols):
            assert torch.equal(some[i], torch.cat(col, 0).reshape(FH, FW, -1)), i


def test_path_drivers_hand_the_grid_on(A):
    """``manipulate_eval_path`` / ``manipulate_demo_path`` with ``skip=``: the frames are ``manipulate_frame(skip=)``'s."""
    mc, mf = models()
    K, pose, trans = frame_scene()
    a = make_args([2], chunk=CHUNK)
    a.target_label = 2
    grid = product_grid(A, MR.random_spec(DIMS, 0.3, 25, "evaluate"))
    n_chunks = -(-FH * FW // CHUNK)
    gen = torch.Generator().manual_seed(10)
    us = [[torch.rand(min(CHUNK, FH * FW - c * CHUNK), NI, generator=gen).cuda() for _ in range(3)] for c in range(n_chunks)]

    def fresh():
        calls = []

        def draws(n, n_imp, count, dev):
            calls.append(n)
            return us[len(calls) - 1][:count]
        return draws
    with torch.no_grad():
        want = A.D.manipulate_frame(FH, FW, K, pose.cuda(), trans, (mc, mf), a, draws=fresh(), skip=grid, skip_levels=("fine",))
        out = A.Ed.manipulate_eval_path([pose.cuda()], (FH, FW, K), (mc, mf), a, trans[0], keep_maps=True, draws=fresh(), skip=grid,
                                        skip_levels=("fine",))
        for name, t in zip(A.Ed.MAP_NAMES, want):
            assert torch.equal(out[name][0], t), name
        objs = [{"obj_name": "chair", "tar_id": 2, "mani_mode": "rigid"}, {"obj_name": "lamp", "tar_id": 4, "mani_mode": "rigid"}]
        objs_trans = {"chair": [{"transformation": A.Ed.Copy(trans[0])}], "lamp": [{"transformation": A.Ed.Remove()}]}
        a2 = make_args([], chunk=CHUNK)
        want = A.D.manipulate_frame(FH, FW, K, pose.cuda(), [A.Ed.Copy(trans[0]), A.Ed.Remove()], (mc, mf), make_args([2, 4], chunk=CHUNK),
                                    draws=fresh(), skip=grid, keep_labels=[1, 2, 4])
        rgbs = np.random.RandomState(0).randint(0, 255, (20, 3)).astype(np.uint8)
        out = A.Ed.manipulate_demo_path([pose.cuda()], (FH, FW, K), (mc, mf), a2, objs, objs_trans, rgbs, {str(i): i for i in range(14)},
                                        {str(i): i for i in range(14)}, keep_maps=True, keep_labels=[1, 2, 4], draws=fresh(), skip=grid)
        for name, t in zip(A.Ed.MAP_NAMES, want):
            assert torch.equal(out[name][0], t), name
