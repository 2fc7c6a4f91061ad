"""GPU tests of the render that skips empty space: the occupancy bit grid (csrc/skip.hip, ``field.SkipGrid``), the mark + compact
pass, the networks over a selection (csrc/mlp_fwd_sparse.hip), ``render.dm_nerf_fine_skip`` and the ``skip=`` route of the frame
drivers.  The grid and the select are compared with the numpy restatement (tests/_skip_restate.py, checked on the CPU by
tests/test_skip_restate.py); the networks and the render with the existing dense product calls.  A selected row is the dense row
bit for bit and a masked row is exactly zero, so every comparison is ``torch.equal``: there is no tolerance anywhere."""
import types

import numpy as np
import pytest
import torch

import _gpu
import _skip_restate as RS
from _gpu import A, frame_rays, random_grid, words_of  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

POISON = 0x40000000                    # an int32 far beyond every sample index used here

_cache = {}


def models(ins_num=13):
    return _gpu.models(ins_num, cache=_cache)


def select(A, grid, ro, rd, z):
    """``dmnerf_skip_select`` -> (flag [N,S] uint8, sel int32 [N*S] (valid below count), count int32 [1])."""
    N, S = z.shape
    L, lib = A.L, A.lib
    flag = torch.full((N, S), 77, dtype=torch.uint8, device="cuda")
    sel = torch.full((N * S,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(N * S)), dtype=torch.int32, device="cuda")
    g = grid.c_struct()
    import ctypes
    L.check(lib.dmnerf_skip_select(ctypes.byref(g), L.ptr(ro), L.ptr(rd), L.ptr(z), N, S, L.ptr(flag), L.ptr(sel), L.ptr(count),
                                   L.ptr(work), L.stream()), "dmnerf_skip_select")
    assert int(count[1]) == POISON                                   # one int32 is written, no more
    return flag, sel, count[:1]


# ---- 1. the grid build against the restatement
@pytest.mark.parametrize("dims", [(5, 7, 9), (32, 32, 32), (33, 8, 40)])
def test_grid_build_equals_the_restatement(A, dims):
    rng = np.random.RandomState(dims[0])
    sig = rng.randn(*dims).astype(np.float32) + np.float32(0.5 - 1.2816)       # about 10 % above the threshold 0.5
    sig.reshape(-1)[rng.choice(sig.size, 3, replace=False)] = np.nan
    cases = {"random": sig, "below": np.full(dims, 0.5, np.float32), "above": np.full(dims, 0.75, np.float32)}
    lo, hi = (-1.0, -2.0, 0.0), (1.0, 2.0, 3.0)
    for name, s in cases.items():
        for dilate in (0, 1, 2):
            g = A.F.SkipGrid.from_sigma(torch.from_numpy(s).cuda(), lo, hi, threshold=0.5, dilate=dilate)
            want = RS.build(s, 0.5, dilate, fast=True)
            assert g.bits.dtype == torch.int32 and g.bits.shape == (want.size,)
            assert np.array_equal(words_of(g), want), (name, dilate)
    assert 0.05 < np.mean(RS.occupied(sig, 0.5)) < 0.2
    assert not words_of(A.F.SkipGrid.from_sigma(torch.from_numpy(cases["below"]).cuda(), lo, hi, 0.5, 2)).any()
    full = A.F.SkipGrid.full(lo, hi, dims)
    assert np.array_equal(words_of(A.F.SkipGrid.from_sigma(torch.from_numpy(cases["above"]).cuda(), lo, hi, 0.5, 0)), words_of(full))
    assert np.array_equal(words_of(full), RS.pack_bits(np.ones(dims, bool)))
    assert not words_of(A.F.SkipGrid.empty(lo, hi, dims)).any()


# ---- 2. mark + compact against the restatement
def select_rays(n, s, seed):
    """Rays against the box [0, 2)^3 with 0.25 cells: crossing it, starting inside it, missing it, lying in a cell face, one NaN."""
    rng = np.random.RandomState(seed)
    kinds = [((-1.0, 0.9, 1.1), (1.0, 0.05, -0.02)),      # crosses the box
             ((1.0, 1.0, 1.0), (0.3, -0.2, 0.25)),         # starts inside
             ((-1.0, 5.0, 5.0), (1.0, 0.0, 0.1)),          # misses
             ((-0.5, 0.5, 0.3), (1.0, 0.0, 0.0)),          # along the cell face y = 0.5
             ((0.1, 0.1, 0.1), (0.5, 0.5, 0.5))]           # the diagonal: through cell corners
    o = np.zeros((n, 3), np.float32)
    d = np.zeros((n, 3), np.float32)
    for i in range(n):
        oo, dd = kinds[i % len(kinds)]
        jit = (rng.rand(3) * 0.2).astype(np.float32) if i >= len(kinds) else np.zeros(3, np.float32)
        o[i], d[i] = np.asarray(oo, np.float32) + jit, dd
    z = np.sort((rng.rand(n, s) * 4.0).astype(np.float32), axis=-1)
    z[0, 0] = 0.0
    if n * s > 20:
        z[n // 2, s // 2] = np.nan
    return o, d, z


@pytest.mark.parametrize("outside", ["evaluate", "empty"])
@pytest.mark.parametrize("n,s", [(1, 1), (3, 5), (7, 64), (130, 192)])
def test_select_equals_the_restatement(A, n, s, outside):
    dims, lo, hi = (8, 8, 8), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)
    grid = random_grid(dims, lo, hi, 0.4, seed=11, outside=outside)
    o, d, z = select_rays(n, s, seed=n + s)
    want_flag, want_sel, want_count = RS.select(o, d, z, words_of(grid), lo, hi, dims, outside)
    ro, rd, zz = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(z).cuda()
    flag, sel, count = select(A, grid, ro, rd, zz)
    flag2, sel2, count2 = select(A, grid, ro, rd, zz)
    assert torch.equal(flag.cpu(), torch.from_numpy(want_flag))
    assert int(count) == want_count
    assert torch.equal(sel[:want_count].cpu(), torch.from_numpy(want_sel))
    assert bool((sel[want_count:] == POISON).all())                  # nothing is written beyond count
    assert torch.equal(flag2, flag) and torch.equal(sel2, sel) and torch.equal(count2, count)      # the same bits every run
    if n * s >= 448:
        assert 0 < want_count < n * s


def test_select_refuses_2_31_samples(A):
    import ctypes
    grid = A.F.SkipGrid.empty((0, 0, 0), (1, 1, 1), 2)
    g = grid.c_struct()
    rc = A.lib.dmnerf_skip_select(ctypes.byref(g), None, None, None, 1 << 20, 1 << 11, None, None, None, None, None)
    assert rc == -1 and "int32" in A.L.last_error()
    assert A.lib.dmnerf_skip_select_work_ints(1 << 31) == -1


# ---- 3. the networks over a selection against their dense twins
SENTINEL = 777.0


def sel_cases(M, seed):
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    return [(c, perm[:c]) for c in (0, 1, 31, 32, 33, 127, 128, 129, M) if c <= M]


def check_sparse(A, run_sel, dense, M):
    """``run_sel(sel, count, out)`` writes rows ``sel[:count]`` of ``out`` (pre-filled with the sentinel); they must equal ``dense``'s,
    the rest must still hold the sentinel.  ``sel`` beyond count is out of range and count is followed by a poison word."""
    flat = dense.reshape(M, -1)
    for c, idx in sel_cases(M, seed=M):
        sel = torch.full((M,), POISON, dtype=torch.int32, device="cuda")
        sel[:c] = idx.cuda()
        count = torch.tensor([c, POISON], dtype=torch.int32, device="cuda")
        out = torch.full_like(flat, SENTINEL)
        run_sel(sel, count, out)
        keep = torch.zeros(M, dtype=torch.bool, device="cuda")
        keep[idx.long().cuda()] = True
        assert torch.equal(out[keep], flat[keep]), c
        assert bool((out[~keep] == SENTINEL).all()), c
    assert float(flat.abs().max()) > 0 and not bool((flat == SENTINEL).any())


@pytest.mark.parametrize("n,s", [(7, 64), (5, 5)])
@pytest.mark.parametrize("variant", ["full14", "full60", "fused14", "density"])
def test_sparse_networks_equal_the_dense_rows(A, variant, n, s):
    ins_num = 59 if variant == "full60" else 13
    mc, mf = models(ins_num)
    ro, rd = frame_rays(n, start=4000)
    z = (4.0 + 11.0 * torch.rand(n, s, generator=torch.Generator().manual_seed(n * s))).sort(-1).values.cuda()
    L, lib = A.L, A.lib
    M = n * s
    with torch.no_grad():
        if variant == "density":
            dense = torch.empty(n, s, device="cuda")
            L.check(lib.dmnerf_mlp_fwd_rays_density(L.ptr(mc.blob()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(dense), L.stream()), "density")
            for blob in (mc.blob(), mc.blob_fused()):
                check_sparse(A, lambda sel, count, out: L.check(lib.dmnerf_mlp_fwd_rays_density_sel(
                    L.ptr(blob), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(sel), L.ptr(count), L.ptr(out), L.stream()), "density_sel"), dense, M)
        else:
            fused = variant == "fused14"
            blob = mf.blob_fused() if fused else mf.blob()
            dense = torch.empty(n, s, 4 + ins_num + 1, device="cuda")
            fn = lib.dmnerf_mlp_fwd_rays_fused if fused else lib.dmnerf_mlp_fwd_rays
            L.check(fn(L.ptr(blob), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(dense), L.stream()), "dense")
            check_sparse(A, lambda sel, count, out: L.check(lib.dmnerf_mlp_fwd_rays_sel(
                L.ptr(blob), ins_num, 1 if fused else 0, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(sel), L.ptr(count), L.ptr(out), L.stream()),
                "rays_sel"), dense, M)


# ---- 4. the whole render
KEYS = ("rgb_fine", "ins_fine", "depth_fine", "z_vals_fine", "raw_fine")
BOX = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0), (16, 16, 16))


def render_case(A, perturb=False, n=130):
    ro, rd = frame_rays(n, start=90000)
    z = A.H.z_val_sample(n, 4.0, 15.0, 64, device="cuda")
    args = types.SimpleNamespace(perturb=1.0 if perturb else False, N_importance=128, is_train=False, N_ins=None)
    g = torch.Generator().manual_seed(5)
    draws = dict(t_rand=torch.rand(n, 64, generator=g).cuda(), u=torch.rand(n, 128, generator=g).cuda()) if perturb else {}
    return ro, rd, z, args, draws


def restate_render(A, mc, mf, ro, rd, z, args, grid, levels, t_rand=None, u=None):
    """The masked render from the existing dense product calls: dense density, flags applied in torch, weights, resampling, the dense
    full network, rows masked to zero, compositing."""
    L, lib = A.L, A.lib
    n, s = z.shape
    n_imp = args.N_importance
    z_c = A.H.stratify(z, t_rand) if t_rand is not None else z
    sigma = torch.empty(n, s, device="cuda")
    L.check(lib.dmnerf_mlp_fwd_rays_density(L.ptr(mc.blob()), mc.ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z_c), n, s, L.ptr(sigma), L.stream()), "density")
    n_eval = [n * s, n * (s + n_imp)]
    if "coarse" in levels:
        flag, _, count = select(A, grid, ro, rd, z_c)
        sigma = torch.where(flag != 0, sigma, torch.zeros_like(sigma))
        n_eval[0] = int(count)
    w = torch.empty(n, s, device="cuda")
    L.check(lib.dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z_c), L.ptr(rd), n, s, L.ptr(w), L.stream()), "weights")
    z_f = A.H.importance_resample(z_c, w, n_imp, u=u)
    raw = A.R.run_network(mf, ro, rd, z_f)
    if "fine" in levels:
        flag, _, count = select(A, grid, ro, rd, z_f)
        raw = torch.where((flag != 0)[..., None], raw, torch.zeros_like(raw))
        n_eval[1] = int(count)
    rgb, _, depth, ins = A.R.render_train(raw, z_f, rd)
    return {"rgb_fine": rgb, "ins_fine": ins, "depth_fine": depth, "z_vals_fine": z_f, "raw_fine": raw}, n_eval


def test_render_with_a_full_grid_equals_dm_nerf_fine(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    grid = A.F.SkipGrid.full(*BOX)
    with torch.no_grad():
        want = A.R.dm_nerf_fine(torch.stack([ro, rd]), None, None, mc, mf, z, args)
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid)
    assert set(got) == set(KEYS) | {"n_eval"}
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got["n_eval"].dtype == torch.int32 and got["n_eval"].tolist() == [130 * 64, 130 * 192]


def test_render_with_an_empty_grid_is_zero(A):
    """Nothing is evaluated: rgb, depth and raw_fine are exactly zero and the pre-sigmoid object sum is exactly zero, so ``ins_fine``
    is exactly sigmoid(0) = 0.5 (the reference applies the sigmoid AFTER the weighted sum, render.py:21-23; an all-zero ``ins_fine``
    cannot come out of the existing compositing)."""
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    grid = A.F.SkipGrid.empty(*BOX, outside="empty")
    with torch.no_grad():
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid)
    for k in ("rgb_fine", "depth_fine", "raw_fine"):
        assert not bool(got[k].any()), k
    # the object map is sigmoid(sum of weight * logit) (networks/render.py:21-23): the sum is exactly 0, so every entry is exactly
    # sigmoid(0) = 0.5 -- measured on the MI355X: ins_fine == 0.5 everywhere, not 0 -- which is what the existing compositing gives
    # for an all-zero raw, and what case (c)'s restatement gives for a ray without a marked sample
    assert bool((got["ins_fine"] == 0.5).all())
    want = A.R.render_train(torch.zeros_like(got["raw_fine"]), got["z_vals_fine"], rd)
    assert torch.equal(got["rgb_fine"], want[0]) and torch.equal(got["depth_fine"], want[2]) and torch.equal(got["ins_fine"], want[3])
    assert got["n_eval"].tolist() == [0, 0]


@pytest.mark.parametrize("case", ["both", "fine_only", "perturb"])
def test_render_with_a_random_grid_equals_the_masked_dense_render(A, case):
    mc, mf = models()
    ro, rd, z, args, draws = render_case(A, perturb=case == "perturb")
    levels = ("fine",) if case == "fine_only" else ("coarse", "fine")
    grid = random_grid(BOX[2], BOX[0], BOX[1], 0.3, seed=21)
    with torch.no_grad():
        want, n_eval = restate_render(A, mc, mf, ro, rd, z, args, grid, levels, **draws)
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid, levels=levels, **draws)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got["n_eval"].tolist() == n_eval
    assert 0 < n_eval[1] < 130 * 192 and float(want["rgb_fine"].abs().max()) > 0
    if case == "fine_only":
        assert n_eval[0] == 130 * 64


# ---- 5. the frame drivers
@pytest.mark.parametrize("chunk", [96, 100])
def test_frame_with_skip_equals_the_per_chunk_restatement(A, chunk):
    """24 x 20 = 480 rays: chunk 96 divides them into five whole chunks, chunk 100 leaves a ragged last chunk of 80."""
    H, W = 20, 24
    mc, mf = models()
    K = np.array([[30.0, 0, W / 2], [0, -30.0, H / 2], [0, 0, -1]])
    c2w = O.pose_spherical(30.0, -65.0, 7.0).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, N_test=chunk, N_samples=64, near=4.0, far=15.0)
    grid = random_grid(BOX[2], BOX[0], BOX[1], 0.3, seed=22)
    with torch.no_grad():
        rgb, ins, depth = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64, skip=grid)
        ro, rd = A.H.get_rays_k(H, W, K, c2w)
        ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
        parts = []
        for s0 in range(0, H * W, chunk):
            e = min(s0 + chunk, H * W)
            z = A.H.z_val_sample(e - s0, 4.0, 15.0, 64, device="cuda")
            parts.append(restate_render(A, mc, mf, ro[s0:e].contiguous(), rd[s0:e].contiguous(), z, args, grid, ("coarse", "fine"))[0])
    assert torch.equal(rgb.reshape(-1, 3), torch.cat([p["rgb_fine"] for p in parts]))
    assert torch.equal(ins.reshape(-1, 13), torch.cat([p["ins_fine"] for p in parts]))
    assert torch.equal(depth.reshape(-1), torch.cat([p["depth_fine"] for p in parts]))
    if chunk == 96:
        with torch.no_grad():
            dense = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64)
            full = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64, skip=A.F.SkipGrid.full(*BOX))
            gt = torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(4)).cuda()
            out = A.D.render_path(c2w[None], (H, W, K), (mc, mf), args, gt_imgs=gt, image_metrics=True, skip=grid)
        for a, b in zip(dense, full):
            assert torch.equal(a, b)
        assert torch.equal(out["rgb"][0], rgb)
        assert bool(torch.isfinite(out["ssim"]).all()) and bool(torch.isfinite(out["psnr_f64"]).all()) and bool(torch.isfinite(out["psnr"]).all())


# ---- 6. capture: no size ever passes through the host
def test_captured_render_follows_the_grid_overwritten_in_place(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A, n=96)
    rays = torch.stack([ro, rd])
    grid_a = random_grid(BOX[2], BOX[0], BOX[1], 0.3, seed=31)
    grid_b = random_grid(BOX[2], BOX[0], BOX[1], 0.7, seed=32)
    grid = A.F.SkipGrid.from_bits(grid_a.bits.clone(), BOX[0], BOX[1], BOX[2])
    with torch.no_grad():
        eager_a = A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, grid_a)          # (also the warm-up of every kernel)
        eager_b = A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, grid_b)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, grid)
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("n_eval",):
            assert torch.equal(out[k], eager_a[k]), k
        grid.bits.copy_(grid_b.bits)
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("n_eval",):
            assert torch.equal(out[k], eager_b[k]), k
    assert eager_a["n_eval"].tolist() != eager_b["n_eval"].tolist()


# ---- 7. the grid from the network
def test_from_model_equals_from_sigma_of_the_queried_centres(A):
    _, mf = models()
    lo, hi, dims = (-2.0, -1.0, 0.0), (1.0, 2.0, 1.5), (8, 8, 8)
    with torch.no_grad():
        ref = A.F.SkipGrid.empty(lo, hi, dims)
        centres = ref.cell_centres()
        assert torch.equal(centres.cpu(), torch.from_numpy(RS.cell_centres(lo, hi, dims)))
        sigma = A.F.query_density(mf, centres).reshape(dims)
        thr = float(sigma.median())                                  # (a threshold that splits the cells)
        for dilate in (0, 1):
            got = A.F.SkipGrid.from_model(mf, lo, hi, dims=dims, threshold=thr, dilate=dilate, slab=100)      # slabs of one plane
            want = A.F.SkipGrid.from_sigma(sigma, lo, hi, threshold=thr, dilate=dilate)
            assert torch.equal(got.bits, want.bits)
            assert np.array_equal(words_of(got), RS.build(sigma.cpu().numpy(), thr, dilate))
    occ0 = float(A.F.SkipGrid.from_sigma(sigma, lo, hi, threshold=thr, dilate=0).occupancy())
    assert 0.3 < occ0 < 0.7
