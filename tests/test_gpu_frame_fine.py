"""GPU tests of the fine-only frame path: the density-only coarse pass (csrc/mlp_fwd_density.hip), the weights-from-sigma kernel
and ``dmnerf_render_rays_fwd_fine`` / ``render.dm_nerf_fine``, which ``FrameRenderer`` uses by default.  The claim is
bit-identity with the full path -- the trunk's MFMA sequence and the density dot product are the same instructions in the same
order -- so every comparison is ``torch.equal``; there is no tolerance to pick."""
import types

import numpy as np
import pytest
import torch

import _gpu
from _gpu import A, frame_rays  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

_model_cache = {}


def models(ins_num=13, D=8, W=256):
    return _gpu.models(ins_num, D, W, cache=_model_cache)


def jittered_z(n, s, seed):
    g = torch.Generator().manual_seed(seed)
    return (4.0 + 11.0 * torch.rand(n, s, generator=g)).sort(-1).values.cuda()


def density(A, blob, ins_num, ro, rd, z):
    sigma = torch.full(z.shape, float("nan"), dtype=torch.float32, device=z.device)
    L = A.L
    L.check(L.load().dmnerf_mlp_fwd_rays_density(L.ptr(blob), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), z.shape[0], z.shape[1],
                                                 L.ptr(sigma), L.stream()), "dmnerf_mlp_fwd_rays_density")
    return sigma


# ---- 1. the density entry against channel 3 of the full kernel
@pytest.mark.parametrize("ins_num", [13, 59, 93])
@pytest.mark.parametrize("n,s", [(8, 64), (3, 64), (7, 17), (1, 1), (300, 64)])
def test_density_entry_equals_the_full_kernels_sigma(A, ins_num, n, s):
    """N*S = 512 (a multiple of 128), 192 (of 32 but not 128: duplicate waves in the last workgroup), 119 and 1 (tail lanes),
    19200 (many workgroups); ins_num moves the table offsets of density_linear with the logit-block count."""
    mc, _ = models(ins_num)
    ro, rd = frame_rays(n, start=1000 * ins_num, stride=1)
    z = jittered_z(n, s, seed=n * 100 + s)
    with torch.no_grad():
        raw = A.R.run_network(mc, ro, rd, z)
        got = density(A, mc.blob(), ins_num, ro, rd, z)
        got_fused_blob = density(A, mc.blob_fused(), ins_num, ro, rd, z)
    assert torch.equal(got, raw[..., 3])
    assert torch.equal(got_fused_blob, got)                      # the trunk and the table entries used are the same in both blobs
    assert float(raw[..., 3].abs().max()) > 0


# ---- 2. weights from sigma against render_train
@pytest.mark.parametrize("s", [64, 192, 70, 3])
def test_weights_kernel_equals_render_trains_weights(A, s):
    n, C = 37, 14
    g = torch.Generator().manual_seed(s)
    raw = torch.randn(n, s, 4 + C, generator=g).cuda()
    raw[..., 3] = raw[..., 3] * 3.0                              # negative densities (relu), opaque and thin samples
    _, rd = frame_rays(n, start=5000, stride=1)
    z = jittered_z(n, s, seed=7 + s)
    sigma = raw[..., 3].contiguous()
    got = torch.full((n, s), float("nan"), dtype=torch.float32, device="cuda")
    L = A.L
    with torch.no_grad():
        _, want, _, _ = A.R.render_train(raw, z, rd)
        L.check(L.load().dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z), L.ptr(rd), n, s, L.ptr(got), L.stream()), "dmnerf_weights_from_sigma")
    assert torch.equal(got, want)
    assert float(want.sum()) > 0


# ---- 3. the fine entry against dm_nerf
FINE_KEYS = ("rgb_fine", "ins_fine", "depth_fine", "z_vals_fine", "raw_fine")


def bench_models(A):
    import bench_common as C
    if "bench" not in _model_cache:
        _model_cache["bench"] = C.build_models(torch.device("cuda"))
    return _model_cache["bench"]


@pytest.mark.parametrize("case", ["bench4096", "ragged17", "perturb", "perturb17", "fuse_heads", "ins59", "shared_u_row"])
def test_fine_entry_equals_dm_nerf(A, case):
    n = 17 if case in ("ragged17", "perturb17") else (4096 if case == "bench4096" else 256)
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    pe = ve = None
    if case == "bench4096":
        pe, ve, mc, mf = bench_models(A)
    else:
        mc, mf = models(59 if case == "ins59" else 13)
    ro, rd = frame_rays(n, start=640 * 200 + 100, stride=1)
    rays = torch.stack([ro, rd])
    z = A.H.z_val_sample(n, 4.0, 15.0, 64, device="cuda")
    kw = {}
    if case.startswith("perturb"):
        args.perturb = 1.0
        g = torch.Generator().manual_seed(5)
        kw = dict(t_rand=torch.rand(n, 64, generator=g).cuda(), u=torch.rand(n, 128, generator=g).cuda())
    if case == "fuse_heads":
        args.fuse_heads = True
    if case == "shared_u_row":
        kw = dict(u=torch.rand(128, generator=torch.Generator().manual_seed(9)).cuda())
    with torch.no_grad():
        want = A.R.dm_nerf(rays, pe, ve, mc, mf, z, args, **kw)
        got = A.R.dm_nerf_fine(rays, pe, ve, mc, mf, z, args, **kw)
    assert set(got) == set(FINE_KEYS)
    for k in FINE_KEYS:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (case, k)
    assert float(got["rgb_fine"].std()) > 0 and bool(torch.isfinite(got["raw_fine"]).all())


def test_fine_entry_draws_like_dm_nerf(A):
    """perturb > 0 without injected draws: t_rand [N,S] first, then u [N,n_imp], from the device generator -- the same stream
    state gives the same render."""
    mc, mf = models()
    ro, rd = frame_rays(64, start=90000, stride=1)
    rays = torch.stack([ro, rd])
    z = A.H.z_val_sample(64, 4.0, 15.0, 64, device="cuda")
    args = types.SimpleNamespace(perturb=1.0, N_importance=128, is_train=False, N_ins=None)
    with torch.no_grad():
        torch.manual_seed(123)
        want = A.R.dm_nerf(rays, None, None, mc, mf, z, args)
        torch.manual_seed(123)
        got = A.R.dm_nerf_fine(rays, None, None, mc, mf, z, args)
    for k in FINE_KEYS:
        assert torch.equal(got[k], want[k]), k


def test_fine_entry_refuses_what_it_cannot_serve(A):
    mc, mf = models()
    ro, rd = frame_rays(8, stride=1)
    z = A.H.z_val_sample(8, 4.0, 15.0, 64, device="cuda")
    for bad in (dict(mfma_split=True), dict(mfma_split="f16x2"), dict(N_importance=0)):
        args = types.SimpleNamespace(**{**dict(perturb=False, N_importance=128, is_train=False, N_ins=None), **bad})
        assert not A.R.fine_eligible(mc, mf, args)
        with torch.no_grad(), pytest.raises(ValueError, match="dm_nerf_fine"):
            A.R.dm_nerf_fine(torch.stack([ro, rd]), None, None, mc, mf, z, args)
    ok = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    assert any(p.requires_grad for p in mc.parameters())
    assert not A.R.fine_eligible(mc, mf, ok)                     # gradients wanted: the training path, both levels' heads feed the losses
    with torch.no_grad():
        assert A.R.fine_eligible(mc, mf, ok)


# ---- 4. the frame driver on the benchmark's configuration
def test_frame_renderer_step_on_the_bench_configuration(A):
    import bench_common as C
    pe, ve, mc, mf = bench_models(A)
    K = O.dmsr_intrinsics(C.H_IMG, C.W_IMG)
    c2w = O.pose_spherical(30.0, -65.0, 7.0).cuda()
    args = types.SimpleNamespace(perturb=False, N_importance=C.N_IMP, is_train=False, N_ins=None)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    with torch.no_grad():
        fr = A.D.FrameRenderer(C.H_IMG, C.W_IMG, K, c2w, (mc, mf), C.NEAR, C.FAR, args, chunk=C.N_RAYS, n_samples=C.S_COARSE)
        assert fr.n_chunks == 75
        i = 40
        rgb, ins, depth = fr.step(i, events=ev)
        torch.cuda.synchronize()
        s, e = i * C.N_RAYS, (i + 1) * C.N_RAYS
        want = A.R.dm_nerf(torch.stack([fr.rays_o[s:e], fr.rays_d[s:e]]), pe, ve, mc, mf, fr.z_full, args)
    assert torch.equal(rgb, want["rgb_fine"]) and torch.equal(ins, want["ins_fine"]) and torch.equal(depth, want["depth_fine"])
    band = fr.band[s:e]
    assert torch.equal(band[:, :3], want["rgb_fine"]) and torch.equal(band[:, 3:-1], want["ins_fine"]) and torch.equal(band[:, -1], want["depth_fine"])
    assert ev[0].elapsed_time(ev[1]) > 0                        # the pair brackets the fine MLP launch (bench.py: roofline.kernel_ms)


# ---- 5. what is not eligible goes the way it went
@pytest.mark.parametrize("case", ["mfma_split", "f16x2", "generic_6x128", "n_importance_0"])
def test_fallbacks_still_render_and_equal_dm_nerf(A, case):
    H, W = 9, 13
    mc, mf = models(13, 6, 128) if case == "generic_6x128" else models()
    args = types.SimpleNamespace(perturb=False, N_importance=0 if case == "n_importance_0" else 128, is_train=False, N_ins=None)
    if case == "mfma_split":
        args.mfma_split = True
    if case == "f16x2":
        args.mfma_split = "f16x2"
    assert not A.R.fine_eligible(mc, mf, args)
    K = np.array([[20.0, 0, W / 2], [0, -20.0, H / 2], [0, 0, -1]])
    c2w = O.pose_spherical(30.0, -65.0, 7.0).cuda()
    with torch.no_grad():
        rgb, ins, depth = A.D.render_frame(H, W, K, c2w, (mc, mf), 4.0, 15.0, args, chunk=50, n_samples=64)
        ro, rd = A.H.get_rays_k(H, W, K, c2w)
        z = A.H.z_val_sample(H * W, 4.0, 15.0, 64, device=ro.device)
        one = A.R.dm_nerf(torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)]), None, None, mc, mf, z, args)
    assert torch.equal(rgb.reshape(-1, 3), one["rgb_fine"])
    assert torch.equal(ins.reshape(-1, 13), one["ins_fine"])
    assert torch.equal(depth.reshape(-1), one["depth_fine"])
    assert float(rgb.std()) > 0


# ---- 6. no allocation, free or synchronisation inside the library
def test_fine_entry_is_graph_capturable(A):
    N = 256
    mc, mf = models()
    pick = lambda s: torch.stack(frame_rays(N, start=s, stride=1))
    z = A.H.z_val_sample(N, 4.0, 15.0, 64, device="cuda")
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    rays = pick(1000)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up on a side stream (weight blobs packed, workspaces sized)
            A.R.dm_nerf_fine(rays, None, None, mc, mf, z, args)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = A.R.dm_nerf_fine(rays, None, None, mc, mf, z, args)
        rays.copy_(pick(150000))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        want = A.R.dm_nerf_fine(pick(150000), None, None, mc, mf, z, args)
        full = A.R.dm_nerf(pick(150000), None, None, mc, mf, z, args)
    for k in FINE_KEYS:
        assert torch.equal(got[k], want[k]) and torch.equal(got[k], full[k]), k
    assert float(got["rgb_fine"].std()) > 0
