"""GPU tests (-m gpu) of the training step that skips empty space: the three entries of csrc/train_skip.hip against torch indexing,
``autograd.run_network_train_skip`` against the dense training path (forward bit for bit on the flagged rows, exact zeros elsewhere)
and against the float64 referee of ``sum(raw * G * flag)`` (backward), the bucket edges and the split at MAX_TRAIN_SAMPLES,
``dm_nerf_train(..., skip=)`` / ``args.train_skip``, the refusals, ``field.TrainSkip`` and a short Adam run.

The scenes are tests/_train_skip_restate.py's: 37 rays, S = 5 (coarse) / 7 (fine), an 8^3 grid written by hand; the selection is
computed on the CPU from the restatement and its conditions (rays without a set cell, rays with every sample set, rays that leave or
miss the box, M' no multiple of 32, evaluated fraction in [0.2, 0.8]) are asserted there.  Gradient bound: the one
tests/test_gpu_train.py applies to the dense MLP backward (``tclose``, rel 2e-4 per tensor), here against float64."""
import copy
import types

import numpy as np
import pytest
import torch

import _train_skip_restate as T
from _gpu import A, model_from  # noqa: F401
from oracle import ref_cpu as O
from test_gpu_train import _loss_from, tclose

pytestmark = pytest.mark.gpu


def _grid(A, words, outside):
    return A.F.SkipGrid.from_bits(words, T.LO, T.HI, T.DIMS, outside=outside)


def _dev(s):
    return torch.from_numpy(s["o"]).cuda(), torch.from_numpy(s["d"]).cuda(), torch.from_numpy(s["z"]).cuda()


_cache = {}


def _case(ins_num, S, outside, seed):
    """Scene, weights, cotangent and the float64 referee of one (ins_num, S, outside): computed once, shared, never modified."""
    key = (ins_num, S, outside, seed)
    if key not in _cache:
        s = T.hand_scene(S, outside)
        sd = O.make_weights(seed, ins_num, gain=1.7)
        cot = torch.randn(T.N_RAYS, S, 4 + ins_num + 1, generator=torch.Generator().manual_seed(seed))
        raw64, want = T.masked_oracle_grads(sd, torch.from_numpy(s["o"]), torch.from_numpy(s["d"]), torch.from_numpy(s["z"]), cot, s["flag"])
        _cache[key] = (s, sd, cot, raw64, want)
    return _cache[key]


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [5, 18, 64])
@pytest.mark.parametrize("n_sel", [0, 1, 63, 64, 65, 300])
def test_kernels_alone(A, width, n_sel):
    lib, L = A.lib, A.L
    N, S = 67, 5                                                      # 335 dense rows: two blocks of 256
    g = torch.Generator().manual_seed(100 * width + n_sel)
    sel = torch.sort(torch.randperm(N * S, generator=g)[:n_sel])[0].to(torch.int32).cuda()
    idx = sel.long()
    n_pad = T.padded_length(n_sel, 64)
    o, d, z = torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda(), torch.rand(N, S, generator=g).cuda()
    nan = float("nan")
    oc, dc, zc = torch.full((n_pad, 3), nan).cuda(), torch.full((n_pad, 3), nan).cuda(), torch.full((n_pad,), nan).cuda()
    L.check(lib.dmnerf_skip_gather_samples(L.ptr(o), L.ptr(d), L.ptr(z), N, S, L.ptr(sel), n_sel, n_pad, L.ptr(oc), L.ptr(dc), L.ptr(zc),
                                           L.stream()), "gather_samples")
    if n_sel:
        full = torch.cat([idx, idx[-1:].expand(n_pad - n_sel)])       # the padding repeats row n_sel - 1
        assert torch.equal(oc, o[full // S]) and torch.equal(dc, d[full // S]) and torch.equal(zc, z.reshape(-1)[full])
        assert torch.equal(oc[n_sel:], oc[n_sel - 1:n_sel].expand(n_pad - n_sel, 3))
    else:
        assert n_pad == 0
    # scatter: compact rows -> dense rows; untouched rows keep the sentinel
    src = torch.randn(n_pad, width, generator=g).cuda()
    dst = torch.full((N * S, width), -7.5).cuda()
    L.check(lib.dmnerf_rows_scatter(L.ptr(src), n_pad, L.ptr(sel), n_sel, L.ptr(dst), N * S, width, L.stream()), "rows_scatter")
    want = torch.full((N * S, width), -7.5).cuda()
    want[idx] = src[:n_sel]
    assert torch.equal(dst, want)
    # gather: dense rows -> compact rows; padded rows exactly 0
    dense = torch.randn(N * S, width, generator=g).cuda()
    out = torch.full((n_pad, width), nan).cuda()
    L.check(lib.dmnerf_rows_gather(L.ptr(dense), N * S, L.ptr(sel), n_sel, L.ptr(out), n_pad, width, L.stream()), "rows_gather")
    assert torch.equal(out[:n_sel], dense[idx])
    assert out[n_sel:].numel() == (n_pad - n_sel) * width and bool((out[n_sel:] == 0).all())
    assert np.array_equal(out.cpu().numpy(), T.rows_gather(dense.cpu().numpy(), sel.cpu().numpy(), n_pad))


def test_entries_refuse_bad_arguments(A):
    lib, L = A.lib, A.L
    t = torch.zeros(64, 5).cuda()
    s = torch.zeros(64, dtype=torch.int32).cuda()
    assert lib.dmnerf_rows_scatter(L.ptr(t), 2, L.ptr(s), 3, L.ptr(t), 64, 5, L.stream()) == -1 and "padded" in L.last_error()
    assert lib.dmnerf_rows_gather(L.ptr(t), 64, L.ptr(s), -1, L.ptr(t), 64, 5, L.stream()) == -1
    assert lib.dmnerf_rows_gather(None, 64, L.ptr(s), 3, L.ptr(t), 64, 5, L.stream()) == -1 and "null" in L.last_error()
    assert lib.dmnerf_rows_scatter(L.ptr(t), 64, L.ptr(s), 3, L.ptr(t), 1 << 31, 5, L.stream()) == -1
    assert lib.dmnerf_rows_scatter(L.ptr(t), 64, L.ptr(s), 3, L.ptr(t), 64, 0, L.stream()) == -1
    assert lib.dmnerf_skip_gather_samples(L.ptr(t), L.ptr(t), L.ptr(t), 1 << 20, 1 << 12, L.ptr(s), 3, 64, L.ptr(t), L.ptr(t), L.ptr(t),
                                          L.stream()) == -1 and "int32" in L.last_error()
    assert lib.dmnerf_skip_gather_samples(L.ptr(t), L.ptr(t), L.ptr(t), 4, 5, L.ptr(s), 0, 64, L.ptr(t), L.ptr(t), L.ptr(t), L.stream()) == -1
    assert lib.dmnerf_skip_gather_samples(None, None, None, 4, 5, None, 0, 0, None, None, None, L.stream()) == 0      # a no-op


# ---- 2. forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, "f16x2"])
@pytest.mark.parametrize("ins_num,S,outside", [(13, 5, "empty"), (13, 5, "evaluate"), (13, 7, "empty"), (13, 7, "evaluate"), (59, 7, "empty")])
def test_forward_rows(A, split, ins_num, S, outside):
    s, sd, _, _, _ = _case(ins_num, S, outside, 7)
    m = model_from(sd, ins_num, train=True)
    o, d, z = _dev(s)
    flag = torch.from_numpy(s["flag"] != 0).cuda()
    dense = A.G.run_network_train(m, o, d, z, split=split).detach()
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    raw = A.G.run_network_train_skip(m, o, d, z, _grid(A, s["words"], outside), split=split, bucket=64, counts=counts)
    assert raw.requires_grad and raw.shape == dense.shape
    assert counts.tolist() == [s["count"], T.N_RAYS * S]
    assert torch.equal(raw.detach()[flag], dense[flag])              # flagged rows: the dense call's, bit for bit
    assert bool((raw.detach()[~flag] == 0).all())                     # every other row: exactly zero
    # the full grid: the dense tensor; the empty grid (outside = "empty"): all zeros, nothing evaluated
    full = A.F.SkipGrid.full(T.LO, T.HI, T.DIMS, outside="evaluate")
    assert torch.equal(A.G.run_network_train_skip(m, o, d, z, full, split=split, bucket=64).detach(), dense)
    counts.zero_()
    none = A.F.SkipGrid.empty(T.LO, T.HI, T.DIMS, outside="empty")
    zero = A.G.run_network_train_skip(m, o, d, z, none, split=split, bucket=64, counts=counts)
    assert counts.tolist() == [0, T.N_RAYS * S] and bool((zero == 0).all())


# ---- 3. backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_num,S,outside", [(13, 5, "empty"), (13, 7, "evaluate"), (59, 7, "empty")])
def test_backward_vs_float64_referee(A, ins_num, S, outside, capsys):
    s, sd, cot, raw64, want = _case(ins_num, S, outside, 7)
    o, d, z = _dev(s)
    flag = torch.from_numpy(s["flag"] != 0).cuda()
    G = cot.cuda()
    m = model_from(sd, ins_num, train=True)
    raw = A.G.run_network_train_skip(m, o, d, z, _grid(A, s["words"], outside), bucket=64)
    tclose(raw.detach()[flag], raw64[torch.from_numpy(s["flag"] != 0)], "raw (flagged rows)", rel=1e-5)
    (raw * G).sum().backward()                                        # unflagged rows are constants: G there reaches nothing
    worst = {}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        worst[k] = tclose(p.grad, want[k], f"grad {k} (skip, ins={ins_num}, S={S}, {outside})")
    # the sanity pair: the dense Function given G * flag meets the same bound
    md = model_from(sd, ins_num, train=True)
    (A.G.run_network_train(md, o, d, z) * (G * flag[..., None])).sum().backward()
    for k, p in md.named_parameters():
        tclose(p.grad, want[k], f"grad {k} (dense, masked cotangent)")
    with capsys.disabled():
        print(f"\n[train skip backward vs f64, ins {ins_num} S {S} {outside}] worst per-tensor max|diff| / max|want|: {max(worst.values()):.2e}")


def test_backward_with_the_empty_grid_gives_zero_gradients(A):
    s, sd, cot, _, _ = _case(13, 5, "empty", 7)
    o, d, z = _dev(s)
    m = model_from(sd, 13, train=True)
    raw = A.G.run_network_train_skip(m, o, d, z, A.F.SkipGrid.empty(T.LO, T.HI, T.DIMS, outside="empty"), bucket=64)
    assert raw.requires_grad                                          # documented: zeros, not None
    (raw * cot.cuda()).sum().backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k


# ---- 4. bucket edges and the split at MAX_TRAIN_SAMPLES --------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 65])
@pytest.mark.parametrize("max_samples", [None, 96])
def test_bucket_edges_and_split(A, K, max_samples, monkeypatch):
    s = T.exact_scene(K)
    assert T.padded_length(K, 64) == (64 if K == 64 else 128)
    if max_samples is not None:
        monkeypatch.setattr(A.G, "MAX_TRAIN_SAMPLES", max_samples)    # Mp = 128 then runs as two launches (96 + 32)
    sd = O.make_weights(9, 13, gain=1.7)
    cot = torch.randn(T.N_RAYS, 5, 18, generator=torch.Generator().manual_seed(9))
    _, want = T.masked_oracle_grads(sd, torch.from_numpy(s["o"]), torch.from_numpy(s["d"]), torch.from_numpy(s["z"]), cot, s["flag"])
    o, d, z = _dev(s)
    flag = torch.from_numpy(s["flag"] != 0).cuda()
    m = model_from(sd, 13, train=True)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    raw = A.G.run_network_train_skip(m, o, d, z, _grid(A, s["words"], "empty"), bucket=64, counts=counts)
    assert counts.tolist() == [K, T.N_RAYS * 5]
    monkeypatch.undo()
    dense = A.G.run_network_train(model_from(sd, 13, train=True), o, d, z).detach()
    assert torch.equal(raw.detach()[flag], dense[flag]) and bool((raw.detach()[~flag] == 0).all())
    (raw * cot.cuda()).sum().backward()
    for k, p in m.named_parameters():
        tclose(p.grad, want[k], f"grad {k} (K={K}, max_samples={max_samples})")


# ---- 5. dm_nerf_train(..., skip=) ------------------------------------------------------------------------------------------------
KEYS = ('rgb_fine', 'ins_fine', 'z_vals_fine', 'raw_fine', 'raw_coarse', 'rgb_coarse', 'ins_coarse', 'z_vals_coarse', 'depth_fine',
        'depth_coarse')


def _dm_nerf_setup(A, ins_num=13):
    s = T.hand_scene(5, "evaluate")
    sd_c, sd_f = O.make_weights(21, ins_num, gain=1.7, sigma_bias=0.3), O.make_weights(22, ins_num, gain=1.7, sigma_bias=0.3)
    o, d, z = _dev(s)
    g = torch.Generator().manual_seed(23)
    t_rand, u = torch.rand(T.N_RAYS, 5, generator=g).cuda(), torch.rand(T.N_RAYS, 2, generator=g).cuda()
    C = ins_num + 1
    cts = [c.cuda() for c in (torch.randn(T.N_RAYS, 3, generator=g), torch.randn(T.N_RAYS, 3, generator=g),
                              torch.randn(T.N_RAYS, ins_num, generator=g), torch.randn(T.N_RAYS, ins_num, generator=g),
                              0.01 * torch.randn(T.N_RAYS, 7, C, generator=g), 0.01 * torch.randn(T.N_RAYS, 5, C, generator=g))]
    args = types.SimpleNamespace(perturb=1.0, N_importance=2, is_train=True, N_ins=None, train_skip_bucket=64)
    return s, sd_c, sd_f, torch.stack([o, d]), z, t_rand, u, cts, args


@pytest.mark.parametrize("split", [None, "f16x2"])
def test_dm_nerf_train_through_the_grid(A, split):
    s, sd_c, sd_f, rays, z, t_rand, u, cts, args = _dm_nerf_setup(A)
    args.mfma_split = split or False
    mc, mf = model_from(sd_c, 13, train=True), model_from(sd_f, 13, train=True)
    dense = A.G.dm_nerf_train(rays, mc, mf, z, args, t_rand=t_rand, u=u)
    full = A.F.SkipGrid.full(T.LO, T.HI, T.DIMS, outside="evaluate")
    out = A.G.dm_nerf_train(rays, mc, mf, z, args, t_rand=t_rand, u=u, skip=full)
    assert sorted(out) == sorted(KEYS)
    for k in KEYS:
        assert torch.equal(out[k].detach(), dense[k].detach()), k
    # the hand-written grid at the fine level only: the coarse level and the fine depths are the dense ones
    for outside in ("evaluate", "empty"):
        grid = _grid(A, s["words"], outside)
        mc.zero_grad(); mf.zero_grad()
        out = A.G.dm_nerf_train(rays, mc, mf, z, args, t_rand=t_rand, u=u, skip=grid, skip_levels=("fine",))
        for k in ('raw_coarse', 'rgb_coarse', 'ins_coarse', 'z_vals_coarse', 'depth_coarse', 'z_vals_fine'):
            assert torch.equal(out[k].detach(), dense[k].detach()), k
        zf = out['z_vals_fine'].detach().cpu().numpy()
        flag, _, count = T.SR.select(s["o"], s["d"], zf, s["words"], T.LO, T.HI, T.DIMS, outside=outside)
        assert 0 < count < flag.size
        flag = torch.from_numpy(flag != 0).cuda()
        assert torch.equal(out['raw_fine'].detach()[flag], dense['raw_fine'].detach()[flag])
        assert bool((out['raw_fine'].detach()[~flag] == 0).all())
        _loss_from(out, cts).backward()
        for m in (mc, mf):
            for k, p in m.named_parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert any(float(p.grad.abs().max()) > 0 for p in mf.parameters())
        # the args route of networks.render.dm_nerf gives the same dict as the keyword route
        args2 = copy.copy(args)
        args2.train_skip, args2.train_skip_levels = grid, ("fine",)
        via = A.R.dm_nerf(rays, None, None, mc, mf, z, args2, t_rand=t_rand, u=u)
        for k in KEYS:
            assert torch.equal(via[k].detach(), out[k].detach()), k


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(A):
    s, sd_c, sd_f, rays, z, t_rand, u, cts, args = _dm_nerf_setup(A)
    mc, mf = model_from(sd_c, 13, train=True), model_from(sd_f, 13, train=True)
    grid = _grid(A, s["words"], "evaluate")
    o, d = rays[0], rays[1]
    with pytest.raises(ValueError, match="bf16x3"):
        A.G.run_network_train_skip(mc, o, d, z, grid, split="bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        A.G.dm_nerf_train(rays, mc, mf, z, types.SimpleNamespace(**vars(args), mfma_split="bf16x3"), t_rand=t_rand, u=u, skip=grid)
    with pytest.raises(ValueError, match="fuse_heads"):
        A.G.dm_nerf_train(rays, mc, mf, z, types.SimpleNamespace(**vars(args), fuse_heads=True), t_rand=t_rand, u=u, skip=grid)
    small = A.M.DM_NeRF(4, 128, 63, 27, [2], 13).cuda().train()
    with pytest.raises(ValueError, match="8 x 256"):
        A.G.run_network_train_skip(small, o, d, z, grid)
    on_cpu = copy.copy(grid)
    on_cpu.bits = grid.bits.cpu()
    with pytest.raises(RuntimeError, match="another device"):
        A.G.run_network_train_skip(mc, o, d, z, on_cpu)
    with pytest.raises(TypeError):
        A.G.run_network_train_skip(mc, o, d, z, s["words"])
    for bad in ((), ("medium",), "both"):
        with pytest.raises(ValueError, match="levels"):
            A.G.dm_nerf_train(rays, mc, mf, z, args, t_rand=t_rand, u=u, skip=grid, skip_levels=bad)
    gargs = copy.copy(args)
    gargs.train_skip = grid
    opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=torch.tensor(5e-4, device="cuda"), capturable=True)
    with pytest.raises(ValueError, match="train_skip"):
        A.graphed.GraphedTrainStep((mc, mf), opt, gargs, 13, rays, z, torch.rand(T.N_RAYS, 3).cuda(),
                                   torch.zeros(T.N_RAYS, dtype=torch.int64).cuda())


# ---- 7. TrainSkip ---------------------------------------------------------------------------------------------------------------
def test_train_skip_schedule(A):
    sd = O.make_weights(5, 13, gain=1.7)
    m = model_from(sd, 13, train=True)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    ts = A.F.TrainSkip(lo, hi, dims=16, every=3, warmup=2, threshold=0.0, dilate=1)
    full = A.F.SkipGrid.full(lo, hi, 16)
    ptr = ts.grid.bits.data_ptr()
    assert torch.equal(ts.grid.bits, full.bits)
    assert ts.step(m) is False and torch.equal(ts.grid.bits, full.bits)              # step 1: still the warm-up
    direct = A.F.SkipGrid.from_model(m, lo, hi, dims=16, threshold=0.0, dilate=0).dilated(1)
    assert ts.step(m) is True and torch.equal(ts.grid.bits, direct.bits)             # step 2 completes it: the first refresh
    assert int(direct.unpack().sum()) > 0
    with torch.no_grad():
        m.density_linear.bias.add_(-1e3)                                             # the field goes empty ...
    assert ts.step(m) is False and ts.step(m) is False
    assert torch.equal(ts.grid.bits, direct.bits)                                    # ... which the grid sees at its next refresh only
    assert ts.step(m) is True and ts.refreshes == 2
    assert torch.equal(ts.grid.bits, A.F.SkipGrid.from_model(m, lo, hi, dims=16, threshold=0.0, dilate=0).dilated(1).bits)
    assert int(ts.grid.unpack().sum()) == 0
    assert ts.grid.bits.data_ptr() == ptr


# ---- 8. a short run --------------------------------------------------------------------------------------------------------------
def test_short_run_with_a_full_grid_follows_the_dense_run(A):
    """20 Adam steps on the analytic scene at 256 rays: with a TrainSkip that is still in its warm-up (a full grid) the forward is
    the dense one bit for bit and only the order of the gradient sums differs (the compact batch is padded to the bucket), so the
    loss trajectory follows the dense run within test_adam_steps_follow_the_oracle_trajectory's rtol."""
    from dm_nerf_amd.networks import evaluator as E, penalizer as P
    from oracle import analytic_scene as S
    ins_num, H, W, views, batch, steps = 13, 30, 40, 4, 256, 20
    dev = torch.device("cuda:0")
    poses, ims, labs = S.make_views(H, W, list(np.linspace(0.0, 360.0, views, endpoint=False)), ins_num)
    K = S.dmsr_intrinsics(H, W)
    d_ims, d_labs = ims.to(dev), labs.to(dev)
    sd_c, sd_f = O.make_weights(51, ins_num, gain=1.7, sigma_bias=0.3), O.make_weights(52, ins_num, gain=1.7, sigma_bias=0.3)
    z = A.H.z_val_sample(batch, S.NEAR, S.FAR, 64, device=dev)

    def run(skip):
        mc, mf = model_from(sd_c, ins_num, train=True), model_from(sd_f, ins_num, train=True)
        opt = torch.optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
        args = types.SimpleNamespace(perturb=1.0, N_importance=128, is_train=True, N_ins=None, penalize=True, tolerance=0.05, deta_w=0.05,
                                     train_skip=skip)
        np.random.seed(0)
        torch.cuda.manual_seed(0)
        losses = []
        for _ in range(steps):
            v = np.random.choice(views)
            tc, ti, rays = A.H.get_select_full(d_ims[v], poses[v, :3, :4], K, d_labs[v], batch)
            out = A.R.dm_nerf(rays, None, None, mc, mf, z, args)
            loss = E.img2mse(out['rgb_fine'], tc) + E.img2mse(out['rgb_coarse'], tc) + E.ins_criterion(out['ins_fine'], ti, ins_num)[0] \
                + E.ins_criterion(out['ins_coarse'], ti, ins_num)[0] \
                + P.ins_penalizer(out['raw_fine'], out['z_vals_fine'], out['depth_fine'], rays[1], args).sum() \
                + P.ins_penalizer(out['raw_coarse'], out['z_vals_coarse'], out['depth_coarse'], rays[1], args).sum()
            opt.zero_grad(); loss.backward(); opt.step()
            if skip is not None:
                assert skip.step(mf) is False                         # the warm-up: the grid stays full
            losses.append(float(loss.detach()))
        return losses

    dense = run(None)
    ts = A.F.TrainSkip((-12.0,) * 3, (12.0,) * 3, dims=16, warmup=1000)
    got = run(ts)
    assert got[0] == dense[0]                                         # the first forward is bit-equal
    assert np.allclose(got, dense, rtol=2e-3), (got, dense)
    assert np.isfinite(got).all()
