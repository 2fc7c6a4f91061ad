"""GPU tests of the surface functions of ``dm_nerf_amd.field`` (csrc/surface.hip): ``extract_surface``, ``vertex_normals``,
``surface_clusters``, ``clean_surface`` and ``mesh_scene``.  The kernels claim the arithmetic and the order of
tests/_surface_restate.py, so every array is compared with ``torch.equal``.  The count kernel's tile is 8 x 8 x 32 points;
``T`` below is its longest edge, and T + 1 = 33 = 4 * 8 + 1 and 2 T + 1 = 65 = 8 * 8 + 1 cross the tile boundaries of all three axes."""
import os
import types

import numpy as np
import pytest
import torch

import _gpu
import _surface_restate as S
from _gpu import A  # noqa: F401
from dm_nerf_amd import field as F
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = 32
FIXTURE_NAMES = ["9x9x9_s0", "9x9x9_s1", "9x9x9_s2", "17x17x17_s0", "17x17x17_s1", "17x17x17_s2", "33x33x33_s0", "33x33x33_s1",
                 "33x33x33_s2", "9x13x17_s0"]


@pytest.fixture(scope="module")
def G():
    with np.load(os.path.join(HERE, "golden", "surface.npz")) as z:
        return {k: z[k] for k in z.files}


def blobs(shape, centres, radii):
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    f = np.zeros(shape)
    for c, r in zip(centres, radii):
        f += np.exp(-((grid - np.asarray(c, dtype=np.float64)) ** 2).sum(-1) / (2.0 * r ** 2))
    return (1.0 - np.exp(-1.2 * f)).astype(np.float32)


_restated = {}


def restated(key, occ, min_triangles):
    """The restatement of one field, computed once and shared (read only)."""
    if key not in _restated:
        v, f = S.extract(occ, 0.45)
        n = S.vertex_normals(v, f)
        rep, size = S.clusters(f)
        _restated[key] = types.SimpleNamespace(v=v, f=f, n=n, rep=rep, size=size, clean=S.clean(v, n, f, min_triangles=min_triangles),
                                               single=S.clean(v, n, f, keep_single_cluster=True))
    return _restated[key]


def same(t, a):
    a = torch.from_numpy(np.ascontiguousarray(a))
    return t.dtype == a.dtype and t.shape == a.shape and torch.equal(t.cpu(), a)


def check_field(key, occ, min_triangles=8, expect_nonempty=True):
    want = restated(key, occ, min_triangles)
    dev = torch.from_numpy(occ).cuda()
    v, f = F.extract_surface(dev, 0.45)
    assert v.is_cuda and f.is_cuda
    print(f"{key}: V {want.v.shape[0]} F {want.f.shape[0]} clusters {len(set(want.rep.tolist()))} "
          f"kept F {want.clean[2].shape[0]} (min_triangles {min_triangles})")
    assert (want.f.shape[0] > 0) == expect_nonempty
    assert same(v, want.v) and same(f, want.f)
    n = F.vertex_normals(v, f, occ.shape)
    assert same(n, want.n)
    rep, size = F.surface_clusters(f)
    assert same(rep, want.rep) and same(size, want.size)
    for kw, ref in ((dict(min_triangles=min_triangles), want.clean), (dict(keep_single_cluster=True), want.single)):
        got = F.clean_surface(v, n, f, **kw)
        assert all(same(g, r) for g, r in zip(got, ref)), kw
    return want


# ---- 1. bit-equality with the restatement
@pytest.mark.parametrize("name", FIXTURE_NAMES)
def test_fixture_fields_equal_the_restatement(A, G, name):
    check_field(name, G[f"field_{name}"], min_triangles=200)


def random_field(shape, seed):
    return np.random.default_rng(seed).uniform(0.0, 0.9, size=shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 2, 7), (7, 2, 2), (5, 2 * T + 2, 3)])
def test_small_and_ragged_shapes(A, shape):
    """Uniform noise: about half of the grid edges cross, in every cell configuration the table has room for."""
    check_field(("noise", shape), random_field(shape, sum(shape)), min_triangles=4)


def test_one_cell_one_corner(A):
    occ = np.zeros((2, 2, 2), np.float32)
    occ[1, 1, 0] = 0.9
    want = check_field("corner", occ, min_triangles=1)
    assert want.f.shape == (1, 3) and want.v.shape == (3, 3)


def tile_field(n):
    """Blobs centred on the tile boundaries of every axis (multiples of 8 in i and j, of 32 in k), so that the surface runs through
    tile seams and the one-point halo, plus one that meets the far corner region."""
    c = [(8.0, 8.0, 32.0), (16.0, 7.5, 31.5), (n - 9.0, 16.0, 12.0), (7.5, n - 8.0, n - 1.0 - 32.0 + 0.5), (n - 4.0, n - 4.0, n - 4.0)]
    return blobs((n, n, n), c, [3.0, 2.5, 3.5, 3.0, 2.0])


def test_tile_and_halo_boundaries_T_plus_1(A):
    check_field("tile33", tile_field(T + 1), min_triangles=150)


def many_blobs_field():
    """65^3 = 2 T + 1 cubed, about 40 small blobs: thousands of cells with triangles, spread over hundreds of workgroups; a few sit on
    tile seams.  A wrong carry between blocks of the scan, or a wrong tile offset, moves every later vertex id."""
    rng = np.random.default_rng(65)
    centres = [tuple(rng.uniform(4.0, 60.0, size=3)) for _ in range(36)] + [(32.0, 32.0, 32.0), (8.0, 40.0, 32.0), (40.0, 8.0, 31.5), (56.0, 56.0, 32.5)]
    return blobs((65, 65, 65), centres, list(rng.uniform(1.3, 2.6, size=40)))


def test_scan_order_with_many_blobs_2T_plus_1(A):
    want = check_field("blobs65", many_blobs_field(), min_triangles=100)
    assert want.f.shape[0] > 4000 and len(set(want.rep.tolist())) >= 20
    kept = want.clean[2].shape[0]
    assert 0 < kept < want.f.shape[0]                                   # some clusters go, some stay


def test_surface_meets_all_six_borders(A):
    n = 12
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    r = np.sqrt(((grid - 5.5) ** 2).sum(-1))
    occ = np.clip(1.0 - r / 14.0, 0.0, 1.0).astype(np.float32)          # > 0.45 within 7.7 of the centre: face centres in, corners out
    assert occ[0, 5, 5] > 0.45 and occ[n - 1, 5, 5] > 0.45 and occ[5, 0, 5] > 0.45 and occ[5, 5, n - 1] > 0.45 and occ[0, 0, 0] < 0.45
    want = check_field("six", occ, min_triangles=10)
    for axis in range(3):
        assert (want.v[:, axis] == 0).any() and (want.v[:, axis] == n - 1).any()
    use = S.edge_use(want.f)
    assert any((b, a) not in use for (a, b) in use)                     # an open mesh


@pytest.mark.parametrize("value", [0.0, 1.0, float("nan")])
def test_empty_fields(A, value):
    v, f = F.extract_surface(torch.full((5, 9, 34), value, device="cuda"), 0.45)
    assert v.shape == (0, 3) and v.dtype == torch.float32 and f.shape == (0, 3) and f.dtype == torch.int32 and v.is_cuda
    n = F.vertex_normals(v, f, (5, 9, 34))
    cv, cn, cf, kept = F.clean_surface(v, n, f)
    assert n.shape == (0, 3) and cv.shape == (0, 3) and cf.shape == (0, 3) and kept.shape == (0,) and kept.dtype == torch.int64


def test_nan_is_outside(A):
    occ = random_field((6, 7, 8), 1)
    occ[2, 3, 4] = 0.9
    nan = occ.copy()
    nan[occ < 0.2] = np.nan                                              # outside either way
    nan[2, 3, 4] = 0.9
    a = F.extract_surface(torch.from_numpy(occ).cuda())
    b = F.extract_surface(torch.from_numpy(nan).cuda())
    assert torch.equal(a[1], b[1]) and a[0].shape == b[0].shape and a[1].shape[0] > 0


# ---- 2. row-major
def test_permuted_axes_give_the_same_vertex_set(A, G):
    occ = torch.from_numpy(G["field_9x13x17_s0"]).cuda()
    v, f = F.extract_surface(occ)
    perm = (2, 0, 1)
    vp, fp = F.extract_surface(occ.permute(*perm).contiguous())
    back = torch.empty_like(vp)
    for new_axis, old_axis in enumerate(perm):
        back[:, old_axis] = vp[:, new_axis]
    def rows(t):
        return sorted(map(tuple, t.cpu().tolist()))
    assert f.shape == fp.shape and rows(v) == rows(back)


# ---- 3. clusters
def test_linked_tori_are_two_clusters(A):
    x, y, z = np.meshgrid(np.arange(-9.0, 16.0), np.arange(-9.0, 10.0), np.arange(-9.0, 10.0), indexing="ij")
    d_a = (np.sqrt(x ** 2 + y ** 2) - 6.0) ** 2 + z ** 2                 # a ring in the xy plane round the origin
    d_b = (np.sqrt((x - 6.0) ** 2 + z ** 2) - 6.0) ** 2 + y ** 2         # a ring in the xz plane through the first one's hole
    occ = np.maximum(np.exp(-d_a / (2 * 1.3 ** 2)), np.exp(-d_b / (2 * 1.3 ** 2))).astype(np.float32)
    want = check_field("tori", occ, min_triangles=10)
    reps = sorted(set(want.rep.tolist()))
    assert len(reps) == 2 and reps[0] == 0
    assert all(n == 1 for n in S.edge_use(want.f).values())
    sizes = [int((want.rep == r).sum()) for r in reps]
    assert min(sizes) > 300                                             # both are whole rings, not fragments


def test_two_spheres_sharing_one_vertex_are_two_clusters(A):
    occ = blobs((11, 11, 11), [(5.0, 5.0, 5.0)], [2.2])
    v, f = S.extract(occ, 0.45)
    V, nf = v.shape[0], f.shape[0]
    second = f.astype(np.int64) + V
    second[second == V + 7] = 7                                         # vertex 7 of the second sphere becomes vertex 7 of the first
    faces = np.concatenate([f.astype(np.int64), second]).astype(np.int32)
    assert (faces[nf:] == 7).any() and not any((b, a) in S.edge_use(faces[:nf]) for (a, b) in S.edge_use(faces[nf:]))
    want_rep, want_size = S.clusters(faces)
    assert sorted(set(want_rep.tolist())) == [0, nf] and set(want_size.tolist()) == {nf}
    rep, size = F.surface_clusters(torch.from_numpy(faces).cuda())
    assert same(rep, want_rep) and same(size, want_size)


def test_only_the_small_blob_goes(A):
    occ = np.maximum(blobs((20, 12, 12), [(13.0, 5.5, 5.5)], [3.0]), blobs((20, 12, 12), [(3.0, 5.5, 5.5)], [1.2]))
    want = check_field("two", occ, min_triangles=100)
    reps = sorted(set(want.rep.tolist()))
    sizes = sorted(int((want.rep == r).sum()) for r in reps)
    assert len(reps) == 2 and sizes[0] < 90 and sizes[1] > 110
    assert want.clean[2].shape[0] == sizes[1] and want.clean[0].shape[0] < want.v.shape[0]


# ---- 4. the whole chain
class CopyCounter:
    """Counts device -> host copies of tensors above 64 bytes.  A hook on the Tensor methods that move data to the host (``cpu``,
    ``numpy``, ``tolist``, ``item``, ``to`` / ``type`` towards the CPU, ``__array__``); the library never copies on its own."""

    def __init__(self, monkeypatch):
        self.big = []
        for name in ("cpu", "numpy", "tolist", "item", "to", "__array__"):
            orig = getattr(torch.Tensor, name)

            def hook(t, *a, _orig=orig, _name=name, **k):
                to_host = _name != "to" or any(str(x).startswith("cpu") for x in list(a) + list(k.values()) if isinstance(x, (str, torch.device)))
                if t.is_cuda and to_host and t.numel() * t.element_size() > 64:
                    self.big.append((_name, tuple(t.shape)))
                return _orig(t, *a, **k)
            monkeypatch.setattr(torch.Tensor, name, hook)


def test_mesh_scene_end_to_end(A, monkeypatch):
    """The field of tests/golden/occupancy.npz stays below 0.026 (its sigma is within +-0.35), so it is empty at 0.45; the same seed
    and gain with ``sigma_bias`` 7.5 and ``sigma_gain`` 10 put sigma in about [4, 11] around the 6.96 that the level corresponds to."""
    with np.load(os.path.join(HERE, "golden", "occupancy.npz")) as z:
        G = {k: z[k] for k in z.files}
    models = [_gpu.model_from(O.make_weights(seed, 13, gain=float(G["gain_13"]), sigma_bias=7.5, sigma_gain=10.0), 13)
              for seed in (int(G["seed_13"]), int(G["seed_13"]) + 1)]
    models = (models[1], models[0])                                   # (coarse, fine): the fine one has the golden seed
    args = types.SimpleNamespace(perturb=False, N_importance=int(G["n_importance"]), N_samples=64, N_test=4096, near=float(G["near"]),
                                 far=float(G["far"]), is_train=False, N_ins=None)
    rng = np.random.default_rng(9)
    rgbs = rng.integers(0, 256, size=(20, 3))
    ins_map = {str(k): int(g) for k, g in zip(range(14), rng.permutation(20))}
    color_dict = {str(g): int(c) for g, c in zip(range(20), rng.permutation(20))}
    transform = np.asarray(G["transform"])
    with torch.no_grad():
        F.mesh_scene(models, transform, args, grid_dim=9, min_triangles=8, extents=G["extents"])      # warm-up: caches, lazy init
        torch.cuda.synchronize()
        counter = CopyCounter(monkeypatch)
        out = F.mesh_scene(models, transform, args, ins_rgbs=rgbs, color_dict=color_dict, ins_map=ins_map, grid_dim=33, min_triangles=8,
                           extents=G["extents"])
        torch.cuda.synchronize()
        big = list(counter.big)
        monkeypatch.undo()
        assert big == [], big
        V, Fk = out.vertices.shape[0], out.faces.shape[0]
        print(f"mesh_scene: raw V {out.vertices_raw.shape[0]} F {out.faces_raw.shape[0]}, cleaned V {V} F {Fk}")
        assert Fk > 100 and 0 < V and out.faces_raw.shape[0] > Fk       # not vacuous: a surface, and the cleaning removed something
        assert all(t.is_cuda for t in (out.vertices, out.faces, out.normals, out.labels, out.conf, out.colors, out.vertices_raw, out.faces_raw))
        assert out.normals.shape == (V, 3) and out.labels.shape == (V,) and out.conf.shape == (V,) and out.colors.shape == (V, 3)
        assert int(out.faces.min()) >= 0 and int(out.faces.max()) < V
        assert len(torch.unique(out.faces)) == V                        # every vertex is referenced
        label, conf = F.label_points(out.vertices, out.normals, models, args)
        assert torch.equal(out.labels, label) and torch.equal(out.conf, conf)
        assert torch.equal(out.colors, F.label_colors(label, rgbs, color_dict, ins_map))
        # the stages, by hand
        occ = F.occupancy_grid(models[1], transform, args, grid_dim=33, extents=G["extents"])
        v_idx, faces_raw = F.extract_surface(occ)
        v_raw = F.scene_vertices(v_idx, 33, transform, G["extents"])
        assert torch.equal(out.faces_raw, faces_raw) and torch.equal(out.vertices_raw, v_raw)
        cv, cn, cf, kept = F.clean_surface(v_raw, F.vertex_normals(v_raw, faces_raw, occ.shape), faces_raw, min_triangles=8)
        assert torch.equal(out.vertices, cv) and torch.equal(out.normals, cn) and torch.equal(out.faces, cf)
        assert torch.equal(out.vertices, v_raw[kept])
        lens = out.normals.norm(dim=1)
        assert bool(((lens - 1).abs() < 1e-5).all() | (lens == 0).all())


# ---- 5. arguments
def test_arguments_are_validated(A):
    lib, err = A.lib, A.L.last_error
    assert lib.dmnerf_surface_count(None, 4, 4, 4, 0.45, None, None, None) == -1 and "null" in err()
    assert lib.dmnerf_surface_count(None, 1, 4, 4, 0.45, None, None, None) == -1 and ">= 2" in err()
    assert lib.dmnerf_surface_count(None, 4, 4, 1, 0.45, None, None, None) == -1 and ">= 2" in err()
    assert lib.dmnerf_surface_count(None, 2048, 1024, 1024, 0.45, None, None, None) == -1 and "2^31" in err()
    assert lib.dmnerf_surface_emit(None, 4, 4, 4, 0.45, None, None, None, None, 3, 1, None, None, None) == -1 and "null" in err()
    assert lib.dmnerf_surface_emit(None, 4, 1, 4, 0.45, None, None, None, None, 3, 1, None, None, None) == -1 and ">= 2" in err()
    assert lib.dmnerf_surface_emit(None, 4, 4, 4, 0.45, None, None, None, None, 2 ** 31, 1, None, None, None) == -1 and "int32" in err()
    assert lib.dmnerf_surface_normals(None, 3, None, 1, None, None, None, None) == -1 and "null" in err()
    assert lib.dmnerf_surface_clusters(None, None, 5, None, None, None, None) == -1 and "null" in err()
    assert lib.dmnerf_surface_clean_mark(None, 5, 5, None, None, 400, None, None, None, None) == -1 and "null" in err()
    assert lib.dmnerf_surface_clean_compact(None, None, None, 5, 5, None, None, None, None, 6, 1, None, None, None, None, None) == -1
    assert lib.dmnerf_surface_clean_compact(None, None, None, 5, 5, None, None, None, None, 2, 1, None, None, None, None, None) == -1 and "null" in err()
    with pytest.raises(RuntimeError, match="CPU tensor"):
        F.extract_surface(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        F.vertex_normals(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="CPU tensor"):
        F.clean_surface(torch.zeros(3, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError):
        F.extract_surface(torch.zeros(4, 4, device="cuda"))
    with pytest.raises(RuntimeError, match=">= 2"):
        F.extract_surface(torch.zeros(4, 1, 4, device="cuda"))
    with pytest.raises(ValueError):
        F.surface_clusters(torch.zeros(2, 3, dtype=torch.int64, device="cuda"))
