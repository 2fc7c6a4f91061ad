"""GPU tests of ``dm_nerf_amd.field``: the density of the field at free points and on the oriented grid of the reference's
``mesh_main`` (csrc/mlp_fwd_points.hip, ``dmnerf_mlp_fwd_points_density`` / ``dmnerf_occupancy_slab``), the occupancy activation,
the vertex labels and their colours.  What is claimed to be the same arithmetic is compared with ``torch.equal``; what is
compared with the reference (tests/golden/occupancy.npz) uses the project's MLP contract |d| <= 1e-5 (1 + |sigma|)."""
import os
import types

import numpy as np
import pytest
import torch

from _gpu import A, model_from  # noqa: F401
from dm_nerf_amd import field as F
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occupancy.npz")
EXP_ULP2 = 2.4e-7                        # the project's 2-ulp bound for a transcendental with a result in [0, 1]


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


_model_cache = {}


def model(A, ins_num, seed, D=8, W=256, **kw):
    key = (ins_num, seed, D, W, tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = model_from(O.make_weights(seed, ins_num, W=W, D=D, **kw), ins_num, D, W)
    return _model_cache[key]


def golden_model(A, G, ins_num):
    return model(A, ins_num, int(G[f"seed_{ins_num}"]), gain=float(G[f"gain_{ins_num}"]), sigma_bias=float(G[f"sigma_bias_{ins_num}"]))


def random_points(m, seed, radius=15.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(m, 3, generator=g) * 2 - 1) * radius).cuda()


def rays_density(A, blob, ins_num, ro, rd, z):
    sigma = torch.full(z.shape, float("nan"), dtype=torch.float32, device=z.device)
    L = A.L
    L.check(L.load().dmnerf_mlp_fwd_rays_density(L.ptr(blob), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z), z.shape[0], z.shape[1],
                                                 L.ptr(sigma), L.stream()), "dmnerf_mlp_fwd_rays_density")
    return sigma


# ---- 1. the same trunk as the rays' density kernel
@pytest.mark.parametrize("ins_num", [13, 93])
@pytest.mark.parametrize("m", [1, 31, 129, 1000])
def test_points_density_equals_the_rays_density_kernel(A, ins_num, m):
    """M = 1 and 31 (one ragged block), 129 (one workgroup and one sample), 1000 (eight workgroups, ragged tail).  The rays' kernel
    forms p + 0 * 0 = p exactly (S = 1).  Both blobs."""
    mdl = model(A, ins_num, 71, gain=1.7, sigma_bias=0.3)
    p = random_points(m, seed=m + ins_num)
    assert m < 31 or float(p.abs().max()) > 14.0
    zero_d, zero_z = torch.zeros_like(p), torch.zeros(m, 1, device="cuda")
    with torch.no_grad():
        want = rays_density(A, mdl.blob(), ins_num, p, zero_d, zero_z).reshape(-1)
        got = F.query_density(mdl, p)
        got_fused = F.query_density(mdl, p, fuse_heads=True)
    assert got.shape == (m,) and got.dtype == torch.float32
    assert torch.equal(got, want) and torch.equal(got_fused, want)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0


# ---- 2. the grid points
@pytest.mark.parametrize("dim", [5, 8])
def test_grid_points_equal_the_reference(A, G, dim):
    got = F.grid_points(G["occ_range"], G["extents"], G["transform"], dim)
    assert got.shape == (dim ** 3, 3) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(G[f"points_{dim}"]))


# ---- 3. the grid prologue against the points prologue
def test_grid_prologue_equals_points_prologue(A, G):
    """9^3 = 729 points: five workgroups and a tail; a slab of 200 cuts through workgroups and leaves a last slab of 129."""
    mdl = golden_model(A, G, 13)
    args = types.SimpleNamespace(near=float(G["near"]), far=float(G["far"]), N_importance=int(G["n_importance"]))
    voxel = float(G["voxel"])
    with torch.no_grad():
        a = F.occupancy_grid(mdl, G["transform"], args, extents=G["extents"], occ_range=G["occ_range"], grid_dim=9, slab=200)
        b = F.occupancy_grid(mdl, G["transform"], args, extents=G["extents"], occ_range=G["occ_range"], grid_dim=9, slab=729)
        pts = F.grid_points(G["occ_range"], G["extents"], G["transform"], 9)
        c = F.query_density(mdl, pts, voxel)
        explicit = F.occupancy_grid(mdl, G["transform"], args, extents=G["extents"], occ_range=G["occ_range"], grid_dim=9, slab=200, voxel=voxel)
    assert a.shape == (9, 9, 9) and a.dtype == torch.float32 and a.is_cuda
    assert torch.equal(a, b) and torch.equal(a.reshape(-1), c) and torch.equal(a, explicit)
    assert float(a.max()) > 0 and float(a.min()) == 0.0


# ---- 4. against the reference
@pytest.mark.parametrize("ins_num,dim", [(13, 5), (13, 8), (93, 5)])
def test_sigma_and_occupancy_against_the_reference(A, G, ins_num, dim):
    mdl = golden_model(A, G, ins_num)
    C = ins_num + 1
    want_s = torch.from_numpy(G[f"sigma_{C}_{dim}"]).double()
    want_o = torch.from_numpy(G[f"occ_{C}_{dim}"]).double()
    voxel = float(G["voxel"])
    args = types.SimpleNamespace(near=float(G["near"]), far=float(G["far"]), N_importance=int(G["n_importance"]))
    with torch.no_grad():
        sigma = F.query_density(mdl, torch.from_numpy(G[f"points_{dim}"]).cuda())
        occ = F.occupancy_grid(mdl, G["transform"], args, extents=G["extents"], occ_range=G["occ_range"], grid_dim=dim)
    err_s = (sigma.cpu().double() - want_s).abs()
    err_o = (occ.reshape(-1).cpu().double() - want_o).abs()
    print(f"ins_num {ins_num} dim {dim}: max sigma err / bound {float((err_s / (1e-5 * (1 + want_s.abs()))).max()):.3f}, "
          f"max occ err {float(err_o.max()):.3e}")
    assert bool((err_s <= 1e-5 * (1 + want_s.abs())).all())
    # |d occ / d sigma| <= voxel, plus the 2-ulp bound of the exponential
    assert bool((err_o <= voxel * 1e-5 * (1 + want_s.abs()) + EXP_ULP2).all())


# ---- 5. the activation alone
@pytest.mark.parametrize("voxel", [11.0 / 128, 3.0])
def test_occupancy_activation_against_float64(A, voxel):
    mdl = model(A, 13, 72, gain=1.7, sigma_bias=0.0)
    p = random_points(500, seed=5, radius=6.0)
    with torch.no_grad():
        sigma = F.query_density(mdl, p)
        occ = F.query_density(mdl, p, voxel)
    s64 = sigma.cpu().double()
    assert int((s64 < 0).sum()) > 20 and int((s64 > 0).sum()) > 20
    want = 1.0 - torch.exp(-s64.clamp(min=0) * float(np.float32(voxel)))
    err = (occ.cpu().double() - want).abs()
    print(f"voxel {voxel}: max |occ - f64| = {float(err.max()):.3e}")
    assert float(err.max()) <= EXP_ULP2
    assert bool((occ[sigma < 0] == 0).all())                       # exactly 0, not a rounding of it
    assert bool((occ >= 0).all()) and bool((occ < 1).all())


# ---- 6. vertex labels
def test_label_points_equals_argmax_of_dm_nerf(A):
    V, near = 100, 4.0
    rng = np.random.default_rng(6)
    normals = rng.standard_normal((V, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    vertices = (normals * rng.uniform(1.0, 2.5, size=(V, 1))).astype(np.float32)
    mc, mf = model(A, 13, 61, gain=1.7, sigma_bias=0.3), model(A, 13, 62, gain=1.7, sigma_bias=0.3)
    args = types.SimpleNamespace(perturb=False, N_importance=128, N_samples=64, N_test=64, near=near, far=15.0, is_train=False, N_ins=None)
    # the four reference lines (mesh_generator.py:106-113) in numpy f32
    rays_d = -torch.from_numpy(normals.copy())
    rays_d = rays_d[:, [0, 2, 1]]
    rays_d[:, 1] = rays_d[:, 1] * -1
    v = vertices.copy()[:, [0, 2, 1]]
    v[:, 1] = v[:, 1] * -1
    rays_o = torch.from_numpy(v) - rays_d * 0.03 * near
    assert rays_o.dtype == torch.float32
    with torch.no_grad():
        z = A.H.z_val_sample(V, 0.01, 15, 64, device="cuda")
        want = A.R.dm_nerf(torch.stack([rays_o, rays_d]).cuda(), None, None, mc, mf, z, args)["ins_fine"]
        label, conf = F.label_points(torch.from_numpy(vertices).cuda(), torch.from_numpy(normals).cuda(), (mc, mf), args)
    assert label.shape == (V,) and label.dtype == torch.int64 and conf.shape == (V,) and conf.dtype == torch.float32
    assert torch.equal(label, torch.argmax(want, dim=-1))
    assert torch.equal(conf, want.max(dim=-1).values)
    assert len(torch.unique(label)) > 1


# ---- 7. colours
def test_label_colors_equal_render_label2world(A):
    rng = np.random.default_rng(7)
    labels = torch.from_numpy(rng.integers(0, 13, size=300)).cuda()
    rgbs = rng.integers(0, 256, size=(20, 3))
    ins_map = {str(k): int(g) for k, g in zip((0, 1, 2, 3, 5, 6, 8, 9, 10, 12), rng.permutation(20))}     # 4, 7 and 11 are absent
    color_dict = {str(g): int(c) for g, c in zip(range(20), rng.permutation(20))}
    assert bool((labels == 7).any())
    # render_label2world (tools/visualizer.py:208-223), restated
    lab = labels.cpu().numpy()
    want = np.zeros((lab.shape[0], 3))
    for label in np.unique(lab):
        if str(int(label)) in ins_map:
            want[lab == label] = rgbs[color_dict[str(ins_map[str(int(label))])]]
    want = want.astype(np.uint8)
    got = F.label_colors(labels, rgbs, color_dict, ins_map)
    assert got.shape == (300, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want[lab == 7] == 0).all() and want.any()


# ---- 8. another network shape goes layer by layer
def test_query_density_on_a_generic_shape(A, monkeypatch):
    mdl = model(A, 13, 73, D=4, W=64, gain=1.7, sigma_bias=0.1)
    assert not mdl._fused_ok()
    monkeypatch.setattr(F, "GENERIC_SLAB", 50)                     # 130 points: three slabs, the last ragged
    p = random_points(130, seed=8, radius=6.0)
    pe, ve = A.M.get_embedder(10, 0)[0], A.M.get_embedder(4, 0)[0]
    voxel = 11.0 / 128
    with torch.no_grad():
        x = torch.cat([pe.embed(p), ve.embed(torch.zeros_like(p))], -1)
        own = mdl(x)[:, 3].cpu().double()
        got = F.query_density(mdl, p).cpu().double()
        occ = F.query_density(mdl, p, voxel).cpu().double()
    bound = 1e-5 * (1 + own.abs())
    assert got.shape == (130,) and bool(((got - own).abs() <= bound).all())
    assert bool(((occ - (1.0 - torch.exp(-own.clamp(min=0) * voxel))).abs() <= voxel * bound + EXP_ULP2).all())
    assert float(own.abs().max()) > 0


# ---- the entries validate before they launch; CPU tensors raise
def test_arguments_are_validated(A):
    mdl = model(A, 13, 71, gain=1.7, sigma_bias=0.3)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        F.query_density(mdl, torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        F.label_colors(torch.zeros(4, dtype=torch.int64), np.zeros((2, 3)), {}, {})
    with pytest.raises(ValueError):
        F.query_density(mdl, torch.zeros(4, 2, device="cuda"))
    with pytest.raises(ValueError):
        F.query_density(mdl, torch.zeros(4, 3, device="cuda"), voxel=-1.0)
    assert F.query_density(mdl, torch.zeros(0, 3, device="cuda")).shape == (0,)
    lib = A.lib
    import ctypes
    s, T = (ctypes.c_float * 3)(), (ctypes.c_float * 12)()
    assert lib.dmnerf_occupancy_slab(None, 13, None, 8, s, T, 500, 13, None, 0.1, None) == -1 and "leaves" in A.L.last_error()
    assert lib.dmnerf_occupancy_slab(None, 13, None, 2000, s, T, 0, 1, None, 0.1, None) == -1
    assert lib.dmnerf_occupancy_slab(None, 13, None, 8, s, T, 512, 0, None, 0.1, None) == 0      # an empty slab at the end
    assert lib.dmnerf_mlp_fwd_points_density(None, 13, None, 4, None, -1.0, None) == -1 and "null" in A.L.last_error()
