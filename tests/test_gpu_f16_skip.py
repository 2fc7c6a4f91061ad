"""GPU tests of the f16x2 (``args.mfma_split = "f16x2"``) density-only coarse pass and empty-space skipping: the density-only and
the selection kernels (csrc/mlp_f16_density.hip, csrc/mlp_f16_sparse.hip), ``render.dm_nerf_fine_f16``, ``render.dm_nerf_fine_skip``
with f16x2 args and the ``skip=`` route of the frame drivers.  A sample is one B-operand column of every MFMA, so its row cannot
depend on which other samples share the wave, and the kept passes are the dense kernel's: every comparison is ``torch.equal``."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _gpu
from _gpu import A, frame_rays, model_from, random_grid  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

POISON = 0x40000000                    # an int32 far beyond every sample index used here
SENTINEL = 777.0
SHAPES = [(1, 1), (3, 5), (7, 64), (130, 192)]

_cache = {}


def models(ins_num=13):
    return _gpu.models(ins_num, cache=_cache)


def select(A, grid, ro, rd, z):
    """``dmnerf_skip_select`` -> (flag [N,S] uint8, sel int32 [N*S] (poison beyond count), count int32 [1])."""
    N, S = z.shape
    L, lib = A.L, A.lib
    flag = torch.full((N, S), 77, dtype=torch.uint8, device="cuda")
    sel = torch.full((N * S,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(N * S)), dtype=torch.int32, device="cuda")
    g = grid.c_struct()
    L.check(lib.dmnerf_skip_select(ctypes.byref(g), L.ptr(ro), L.ptr(rd), L.ptr(z), N, S, L.ptr(flag), L.ptr(sel), L.ptr(count),
                                   L.ptr(work), L.stream()), "dmnerf_skip_select")
    return flag, sel, count[:1]


def depths(n, s):
    return (4.0 + 11.0 * torch.rand(n, s, generator=torch.Generator().manual_seed(n * s))).sort(-1).values.cuda()


_dense = {}


def dense_f16(A, ins_num, n, s):
    """(ro, rd, z, raw) of ``dmnerf_mlp_fwd_rays_f16`` with the fine model: computed once per shape, shared, never written again."""
    key = (ins_num, n, s)
    if key not in _dense:
        mf = models(ins_num)[1]
        ro, rd = frame_rays(n, start=4000)
        z = depths(n, s)
        L, lib = A.L, A.lib
        raw = torch.full((n, s, 4 + ins_num + 1), SENTINEL, device="cuda")
        L.check(lib.dmnerf_mlp_fwd_rays_f16(L.ptr(mf.blob_f16()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(raw), L.stream()), "f16")
        assert not bool((raw == SENTINEL).any()) and float(raw[..., 3].abs().max()) > 0
        _dense[key] = (ro, rd, z, raw)
    return _dense[key]


# ---- 1. density-only, dense
@pytest.mark.parametrize("n,s,ins_num", [(n, s, 13) for n, s in SHAPES] + [(3, 5, 93)])
def test_density_f16_equals_the_density_channel_of_the_full_kernel(A, n, s, ins_num):
    mf = models(ins_num)[1]
    ro, rd, z, raw = dense_f16(A, ins_num, n, s)
    L, lib = A.L, A.lib
    blob = mf.blob_f16_density()
    assert blob.numel() == lib.dmnerf_blob_f16_density_words(ins_num) and blob is mf.blob_f16_density()
    sigma = torch.full((n, s), SENTINEL, device="cuda")
    L.check(lib.dmnerf_mlp_fwd_rays_density_f16(L.ptr(blob), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(sigma), L.stream()), "density_f16")
    assert torch.equal(sigma, raw[..., 3])


def test_density_blob_refreshes_after_load_state_dict(A):
    ins_num, n, s = 13, 3, 5
    ro, rd, z, raw = dense_f16(A, ins_num, n, s)
    L, lib = A.L, A.lib
    m = model_from(O.make_weights(7, ins_num, gain=1.7, sigma_bias=0.3), ins_num)

    def sigma_of(model):
        out = torch.full((n, s), SENTINEL, device="cuda")
        L.check(lib.dmnerf_mlp_fwd_rays_density_f16(L.ptr(model.blob_f16_density()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(out),
                                                    L.stream()), "density_f16")
        return out
    before = sigma_of(m)
    assert not torch.equal(before, raw[..., 3])
    m.load_state_dict(O.make_weights(62, ins_num, gain=1.7, sigma_bias=0.3))       # the fine model's weights
    assert torch.equal(sigma_of(m), raw[..., 3])


# ---- 2. the selection kernels
def sel_lists(A, n, s, ro, rd, z):
    M = n * s
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M)).to(torch.int32)          # deliberately unsorted
    out = [(c, perm[:c].cuda()) for c in (0, 1, 31, 32, 33, 128, 129, M) if c <= M]
    grid = random_grid((8, 8, 8), (-4.0, -4.0, -4.0), (4.0, 4.0, 4.0), 0.4, seed=11)
    _, sel, count = select(A, grid, ro, rd, z)                       # ascending, from the product's own select
    out.append((int(count), sel[:int(count)].clone()))
    return out


def check_sel(A, run_sel, dense, n, s, lists):
    M = n * s
    flat = dense.reshape(M, -1)
    for c, idx in lists:
        sel = torch.full((M,), POISON, dtype=torch.int32, device="cuda")          # beyond count: never read
        sel[:c] = idx
        count = torch.tensor([c, POISON], dtype=torch.int32, device="cuda")
        out = torch.full_like(flat, SENTINEL)
        run_sel(sel, count, out)
        keep = torch.zeros(M, dtype=torch.bool, device="cuda")
        keep[idx.long()] = True
        assert torch.equal(out[keep], flat[keep]), c
        assert bool((out[~keep] == SENTINEL).all()), c


@pytest.mark.parametrize("n,s,ins_num", [(n, s, 13) for n, s in SHAPES] + [(3, 5, 59), (7, 64, 59), (3, 5, 93), (7, 64, 93)])
def test_f16_sel_writes_the_dense_rows_and_nothing_else(A, n, s, ins_num):
    mf = models(ins_num)[1]
    ro, rd, z, raw = dense_f16(A, ins_num, n, s)
    L, lib = A.L, A.lib
    lists = sel_lists(A, n, s, ro, rd, z)
    if n * s >= 448:
        assert 0 < lists[-1][0] < n * s
    check_sel(A, lambda sel, count, out: L.check(lib.dmnerf_mlp_fwd_rays_f16_sel(
        L.ptr(mf.blob_f16()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(sel), L.ptr(count), L.ptr(out), L.stream()), "f16_sel"),
        raw, n, s, lists)


@pytest.mark.parametrize("n,s", SHAPES)
def test_density_f16_sel_writes_the_dense_entries_and_nothing_else(A, n, s):
    ins_num = 13
    mf = models(ins_num)[1]
    ro, rd, z, raw = dense_f16(A, ins_num, n, s)
    L, lib = A.L, A.lib
    check_sel(A, lambda sel, count, out: L.check(lib.dmnerf_mlp_fwd_rays_density_f16_sel(
        L.ptr(mf.blob_f16_density()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), n, s, L.ptr(sel), L.ptr(count), L.ptr(out), L.stream()),
        "density_f16_sel"), raw[..., 3].contiguous(), n, s, sel_lists(A, n, s, ro, rd, z))


# ---- 3. dm_nerf_fine_f16
KEYS = ("rgb_fine", "ins_fine", "depth_fine", "z_vals_fine", "raw_fine")
BOX = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0), (16, 16, 16))


def f16_args(perturb=False, **kw):
    return types.SimpleNamespace(perturb=1.0 if perturb else False, N_importance=128, is_train=False, N_ins=None, mfma_split="f16x2", **kw)


def render_case(A, perturb=False, n=96):
    ro, rd = frame_rays(n, start=90000)
    z = A.H.z_val_sample(n, 4.0, 15.0, 64, device="cuda")
    g = torch.Generator().manual_seed(5)
    draws = dict(t_rand=torch.rand(n, 64, generator=g).cuda(), u=torch.rand(n, 128, generator=g).cuda()) if perturb else {}
    return ro, rd, z, f16_args(perturb), draws


@pytest.mark.parametrize("perturb", [False, True])
def test_dm_nerf_fine_f16_equals_dm_nerf(A, perturb):
    mc, mf = models()
    ro, rd, z, args, draws = render_case(A, perturb)
    rays = torch.stack([ro, rd])
    with torch.no_grad():
        assert A.R.fine_f16_eligible(mc, mf, args) and not A.R.fine_eligible(mc, mf, args)
        want = A.R.dm_nerf(rays, None, None, mc, mf, z, args, **draws)
        got = A.R.dm_nerf_fine_f16(rays, None, None, mc, mf, z, args, **draws)
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert float(got["rgb_fine"].std()) > 0


def test_fine_f16_eligibility_and_refusals(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    rays = torch.stack([ro, rd])
    f32 = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    bf16 = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, mfma_split="bf16x3")
    zero = f16_args()
    zero.N_importance = 0
    with torch.no_grad():
        assert A.R.fine_f16_eligible(mc, mf, args)
        for bad in (f32, bf16, zero):
            assert not A.R.fine_f16_eligible(mc, mf, bad)
            with pytest.raises(ValueError, match="dm_nerf_fine_f16"):
                A.R.dm_nerf_fine_f16(rays, None, None, mc, mf, z, bad)
        with pytest.raises(ValueError, match="dm_nerf_fine_skip"):
            A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, bf16, A.F.SkipGrid.full(*BOX))
    assert not A.R.fine_f16_eligible(mc, mf, args)                     # gradients enabled on trainable models: training


# ---- 4. dm_nerf_fine_skip with f16x2 args
def restate_render(A, mc, mf, ro, rd, z, args, grid, levels, t_rand=None, u=None):
    """The masked f16x2 render composed from product calls: dense f16 coarse -> raw[..., 3] * flag -> weights -> resampling -> dense
    f16 fine -> rows masked to zero -> compositing."""
    L, lib = A.L, A.lib
    n, s = z.shape
    n_imp = args.N_importance
    z_c = A.H.stratify(z, t_rand) if t_rand is not None else z
    sigma = A.R.run_network(mc, ro, rd, z_c, split="f16x2")[..., 3].contiguous()
    n_eval = [n * s, n * (s + n_imp)]
    if "coarse" in levels:
        flag, _, count = select(A, grid, ro, rd, z_c)
        sigma = torch.where(flag != 0, sigma, torch.zeros_like(sigma))
        n_eval[0] = int(count)
    w = torch.empty(n, s, device="cuda")
    L.check(lib.dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z_c), L.ptr(rd), n, s, L.ptr(w), L.stream()), "weights")
    z_f = A.H.importance_resample(z_c, w, n_imp, u=u)
    raw = A.R.run_network(mf, ro, rd, z_f, split="f16x2")
    if "fine" in levels:
        flag, _, count = select(A, grid, ro, rd, z_f)
        raw = torch.where((flag != 0)[..., None], raw, torch.zeros_like(raw))
        n_eval[1] = int(count)
    rgb, _, depth, ins = A.R.render_train(raw, z_f, rd)
    return {"rgb_fine": rgb, "ins_fine": ins, "depth_fine": depth, "z_vals_fine": z_f, "raw_fine": raw}, n_eval


def test_f16_skip_with_a_full_grid_equals_dm_nerf_fine_f16(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    rays = torch.stack([ro, rd])
    with torch.no_grad():
        want = A.R.dm_nerf_fine_f16(rays, None, None, mc, mf, z, args)
        got = A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, A.F.SkipGrid.full(*BOX))
    assert set(got) == set(KEYS) | {"n_eval"}
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got["n_eval"].tolist() == [96 * 64, 96 * 192]


def test_f16_skip_with_an_empty_grid_is_zero(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    with torch.no_grad():
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, A.F.SkipGrid.empty(*BOX, outside="empty"))
    for k in ("rgb_fine", "depth_fine", "raw_fine"):
        assert not bool(got[k].any()), k
    assert bool((got["ins_fine"] == 0.5).all())                      # sigmoid of an exactly zero weighted sum
    assert got["n_eval"].tolist() == [0, 0]


@pytest.mark.parametrize("case", ["both", "fine_only", "both_perturb", "fine_only_perturb"])
def test_f16_skip_with_a_random_grid_equals_the_masked_dense_render(A, case):
    mc, mf = models()
    ro, rd, z, args, draws = render_case(A, perturb=case.endswith("perturb"))
    levels = ("fine",) if case.startswith("fine_only") else ("coarse", "fine")
    grid = random_grid(BOX[2], BOX[0], BOX[1], 0.3, seed=21)
    with torch.no_grad():
        want, n_eval = restate_render(A, mc, mf, ro, rd, z, args, grid, levels, **draws)
        got = A.R.dm_nerf_fine_skip(torch.stack([ro, rd]), None, None, mc, mf, z, args, grid, levels=levels, **draws)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert got["n_eval"].tolist() == n_eval
    assert 0 < n_eval[1] < 96 * 192 and float(want["rgb_fine"].std()) > 0
    if "coarse" in levels:
        assert 0 < n_eval[0] < 96 * 64
    else:
        assert n_eval[0] == 96 * 64


# ---- 5. the frame drivers
@pytest.mark.parametrize("chunk", [96, 100])
def test_f16_frame_with_skip_equals_the_per_chunk_restatement(A, chunk):
    """24 x 20 = 480 rays: chunk 96 divides them into five whole chunks, chunk 100 leaves a ragged last chunk of 80."""
    H, W = 20, 24
    mc, mf = models()
    K = np.array([[30.0, 0, W / 2], [0, -30.0, H / 2], [0, 0, -1]])
    c2w = O.pose_spherical(30.0, -65.0, 7.0).cuda()
    args = f16_args(N_test=chunk, N_samples=64, near=4.0, far=15.0)
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
    assert float(rgb.std()) > 0
    if chunk == 96:                                                  # the dense f16x2 frame (density-only coarse pass) == the full grid == dm_nerf
        with torch.no_grad():
            dense = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64)
            full = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=chunk, n_samples=64, skip=A.F.SkipGrid.full(*BOX))
            z = A.H.z_val_sample(chunk, 4.0, 15.0, 64, device="cuda")
            first = A.R.dm_nerf(torch.stack([ro[:chunk].contiguous(), rd[:chunk].contiguous()]), None, None, mc, mf, z, args)
        for a, b in zip(dense, full):
            assert torch.equal(a, b)
        assert torch.equal(dense[0].reshape(-1, 3)[:chunk], first["rgb_fine"])


# ---- 6. capture
def test_f16_captured_render_follows_grid_and_rays_overwritten_in_place(A):
    mc, mf = models()
    ro, rd, z, args, _ = render_case(A)
    ro_b, rd_b = frame_rays(96, start=150000)
    grid_a = random_grid(BOX[2], BOX[0], BOX[1], 0.3, seed=31)
    grid_b = random_grid(BOX[2], BOX[0], BOX[1], 0.7, seed=32)
    grid = A.F.SkipGrid.from_bits(grid_a.bits.clone(), BOX[0], BOX[1], BOX[2])
    rays = torch.stack([ro, rd])
    with torch.no_grad():
        eager_a = A.R.dm_nerf_fine_skip(rays.clone(), None, None, mc, mf, z, args, grid_a)
        eager_b = A.R.dm_nerf_fine_skip(torch.stack([ro_b, rd_b]), None, None, mc, mf, z, args, grid_b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                                # warm-up on a side stream: every kernel loaded, every blob cached
            A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, grid)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = A.R.dm_nerf_fine_skip(rays, None, None, mc, mf, z, args, grid)
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("n_eval",):
            assert torch.equal(out[k], eager_a[k]), k
        grid.bits.copy_(grid_b.bits)
        rays[0].copy_(ro_b)
        rays[1].copy_(rd_b)
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS + ("n_eval",):
            assert torch.equal(out[k], eager_b[k]), k
    assert eager_a["n_eval"].tolist() != eager_b["n_eval"].tolist()
