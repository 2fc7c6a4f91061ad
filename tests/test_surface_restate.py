"""The numpy restatement of csrc/surface.hip (tests/_surface_restate.py) against scikit-image's own meshes stored in
tests/golden/surface.npz (tests/golden/make_golden_surface.py), hand cases, ``clean``, and the two host-side pieces of
``dm_nerf_amd.field``: ``scene_vertices`` and ``write_ply``.  No GPU."""
import os

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import _surface_restate as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface.npz")


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def lexsorted(v):
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]


def n_components(faces, n_vertices):
    """Connected components of the mesh over its vertices (every vertex here is referenced)."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]]])
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n_vertices, n_vertices))
    return connected_components(g, directed=False)[0]


def blob(shape, centre, radius, peak=1.0):
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    r2 = ((grid - np.asarray(centre, dtype=np.float64)) ** 2).sum(-1)
    return (peak * np.exp(-r2 / (2.0 * radius ** 2))).astype(np.float32)


NAMES = ["9x9x9_s0", "9x9x9_s1", "9x9x9_s2", "17x17x17_s0", "17x17x17_s1", "17x17x17_s2", "33x33x33_s0", "33x33x33_s1", "33x33x33_s2",
         "9x13x17_s0"]


def test_fixture_lists_the_fields(G):
    assert list(G["names"]) == NAMES and float(G["level"]) == 0.45


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_skimage(G, name):
    field = G[f"field_{name}"]
    v, f = S.extract(field, 0.45)
    lew_v, lew_f = G[f"lew_v_{name}"], G[f"lew_f_{name}"]
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert v.shape == lew_v.shape and f.shape == lew_f.shape
    d = float(np.abs(lexsorted(v).astype(np.float64) - lexsorted(lew_v).astype(np.float64)).max())
    print(f"{name}: max vertex difference {d:.3e}, tolerance {float(G[f'vertex_tol_{name}']):.3e}")
    assert d <= float(G[f"vertex_tol_{name}"])
    use = S.edge_use(f)
    assert all(n == 1 for n in use.values())                            # every directed edge once ...
    assert all((b, a) in use for (a, b) in use)                         # ... and its reverse too: two triangles, opposite directions
    assert n_components(f, v.shape[0]) == n_components(lew_f, lew_v.shape[0])
    vol, area = S.signed_volume(v, f), S.area(v, f)
    lew_vol, lor_vol = float(G[f"lew_vol_{name}"]), float(G[f"lor_vol_{name}"])
    lew_area, lor_area = float(G[f"lew_area_{name}"]), float(G[f"lor_area_{name}"])
    assert np.sign(vol) == np.sign(lew_vol) and vol != 0
    tol_v = max(4.0 * abs(lew_vol - lor_vol), 1e-5 * abs(lew_vol))
    tol_a = max(4.0 * abs(lew_area - lor_area), 1e-5 * abs(lew_area))
    print(f"{name}: volume {vol:.6f} (skimage {lew_vol:.6f} / {lor_vol:.6f}, tol {tol_v:.2e}), area {area:.6f} ({lew_area:.6f} / {lor_area:.6f})")
    assert min(abs(vol - lew_vol), abs(vol - lor_vol)) <= tol_v
    assert min(abs(area - lew_area), abs(area - lor_area)) <= tol_a
    # the classic table is the one behind method='lorensen': the same triangles, as sets of sorted vertex positions
    lor_v, lor_f = G[f"lor_v_{name}"], G[f"lor_f_{name}"]
    rank_of = {tuple(np.round(p, 3)): i for i, p in enumerate(lexsorted(v))}
    mine = sorted(tuple(sorted(rank_of[tuple(np.round(v[i], 3))] for i in tri)) for tri in f)
    theirs = sorted(tuple(sorted(rank_of[tuple(np.round(lor_v[i], 3))] for i in tri)) for tri in lor_f)
    assert mine == theirs


def test_one_corner_inside_gives_one_triangle():
    occ = np.zeros((2, 2, 2), np.float32)
    occ[1, 0, 1] = 1.0
    v, f = S.extract(occ, 0.45)
    assert v.shape == (3, 3) and f.shape == (1, 3) and sorted(f[0]) == [0, 1, 2]
    want = np.array([[0.45, 0, 1], [1, 0.55, 1], [1, 0, 0.45]], np.float32)     # the point (1, 0, 1) at 1, its neighbours at 0
    assert np.allclose(lexsorted(v), lexsorted(want), atol=1e-6)


def test_a_face_inside_gives_two_triangles():
    occ = np.zeros((2, 2, 2), np.float32)
    occ[0] = 1.0
    v, f = S.extract(occ, 0.45)
    assert v.shape == (4, 3) and f.shape == (2, 3)
    assert np.allclose(v[:, 0], 0.55, atol=1e-6)
    assert abs(S.area(v, f) - 1.0) < 1e-6


def test_nan_is_outside():
    occ = np.zeros((2, 2, 2), np.float32)
    occ[0, 0, 0] = 1.0
    nan = occ.copy()
    nan[1, 1, 1] = np.nan
    (v0, f0), (v1, f1) = S.extract(occ, 0.45), S.extract(nan, 0.45)
    assert np.array_equal(f0, f1) and np.array_equal(v0, v1) and f0.shape == (1, 3)
    allnan = np.full((3, 3, 3), np.nan, np.float32)
    assert S.extract(allnan, 0.45)[1].shape == (0, 3)


@pytest.mark.parametrize("value", [0.0, 1.0])
def test_uniform_grids_are_empty(value):
    v, f = S.extract(np.full((3, 4, 5), value, np.float32), 0.45)
    assert v.shape == (0, 3) and v.dtype == np.float32 and f.shape == (0, 3) and f.dtype == np.int32


def test_a_surface_cut_by_the_border_is_open():
    occ = blob((9, 9, 9), (0.0, 4.0, 4.0), 2.5)                        # half a ball against the i = 0 border
    v, f = S.extract(occ, 0.45)
    assert f.shape[0] > 20
    use = S.edge_use(f)
    assert all(n == 1 for n in use.values())
    border = [(a, b) for (a, b) in use if (b, a) not in use]
    assert len(border) >= 8
    for a, b in border:                                                 # used once: both ends lie on the border plane
        assert v[a, 0] == 0.0 and v[b, 0] == 0.0
    for (a, b) in use:                                                  # an edge off the plane is interior: used twice
        if v[a, 0] != 0.0 or v[b, 0] != 0.0:
            assert (b, a) in use


def test_clean_drops_the_small_cluster_and_reindexes():
    min_triangles = 100
    occ = np.maximum(blob((20, 12, 12), (13.0, 5.5, 5.5), 3.0), blob((20, 12, 12), (3.0, 5.5, 5.5), 1.2))
    v, f = S.extract(occ, 0.45)
    rep, size = S.clusters(f)
    reps = sorted(set(rep.tolist()))
    assert len(reps) == 2
    small, large = sorted(int(size[rep == r][0]) for r in reps)
    print(f"clusters of {small} and {large} triangles, threshold {min_triangles}")
    assert small < 0.9 * min_triangles and large > 1.1 * min_triangles            # never marginal
    assert small + large == f.shape[0] and rep[0] == 0                  # the small blob comes first: its triangles go from the front
    assert all(int(size[rep == r][0]) == int((rep == r).sum()) and r == int(np.nonzero(rep == r)[0][0]) for r in reps)
    n = S.vertex_normals(v, f)
    cv, cn, cf, kept = S.clean(v, n, f, min_triangles=min_triangles)
    keep = size >= min_triangles
    assert cf.shape == (large, 3) and cf.dtype == np.int32 and kept.dtype == np.int64
    assert np.array_equal(kept, np.unique(f[keep]))                     # ascending: the order is preserved
    assert np.array_equal(cv, v[kept]) and np.array_equal(cn, n[kept])
    assert np.array_equal(kept[cf], f[keep])                            # re-indexed faces name the same vertices, in the same order
    assert cf.max() == cv.shape[0] - 1 and len(np.unique(cf)) == cv.shape[0]
    sv, sn, sf, skept = S.clean(v, n, f, keep_single_cluster=True)
    assert np.array_equal(sf, cf) and np.array_equal(skept, kept)
    ev, en, ef, ekept = S.clean(v, n, f, min_triangles=10 ** 6)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ekept.shape == (0,)


def test_vertex_normals_point_down_the_gradient():
    """Area-weighted, unit length, and with the 'ascent' winding they point towards lower occupancy (out of the blob)."""
    occ = blob((11, 11, 11), (5.0, 5.0, 5.0), 2.5)
    v, f = S.extract(occ, 0.45)
    n = S.vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    radial = (v - 5.0) / np.linalg.norm(v - 5.0, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0.9).all()
    # a vertex nobody references keeps a zero normal
    n2 = S.vertex_normals(np.concatenate([v, np.ones((1, 3), np.float32)]), f)
    assert np.array_equal(n2[:-1], n) and (n2[-1] == 0).all()


def test_scene_vertices_against_the_reference_lines():
    from dm_nerf_amd import field as F
    rng = np.random.default_rng(3)
    v = (rng.uniform(0, 32, size=(500, 3))).astype(np.float32)
    a = rng.standard_normal((3, 3))
    q, _ = np.linalg.qr(a)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rng.uniform(-2, 2, size=3)
    extents = np.array([1.9, 7.0, 7.0])
    # mesh_generator.py:72-86 step by step, each step a homogeneous transform of the float64 vertices as trimesh applies it
    w = v.astype(np.float64) / (33 - 1)
    for M in (np.block([[np.eye(3), np.full((3, 1), -0.5)], [np.zeros((1, 3)), np.ones((1, 1))]]), np.diag([2.0, 2.0, 2.0, 1.0]),
              np.diag(list(extents / 2.0) + [1.0]), T):
        w = (M[:3, :3] @ w.T).T + M[:3, 3]
    want = w.astype(np.float32)
    got = F.scene_vertices(torch.from_numpy(v), 33, T, extents)
    assert got.dtype == torch.float32 and got.shape == (500, 3)
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(S.scene_vertices(v, 33, T, extents), want)
    assert F.scene_vertices(torch.zeros(0, 3), 33, T).shape == (0, 3)


def test_write_ply_round_trip(tmp_path):
    from dm_nerf_amd import field as F
    rng = np.random.default_rng(4)
    v = rng.standard_normal((5, 3)).astype(np.float32)
    n = rng.standard_normal((5, 3)).astype(np.float32)
    c = rng.integers(0, 256, size=(5, 3)).astype(np.uint8)
    f = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    path = str(tmp_path / "m.ply")
    F.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), normals=torch.from_numpy(n), colors=torch.from_numpy(c))
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n")[:-1] == [
        "ply", "format binary_little_endian 1.0", "element vertex 5", "property float x", "property float y", "property float z",
        "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
        "property uchar blue", "element face 2", "property list uchar int vertex_indices"]
    vt = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("i", "<i4", 3)])
    assert len(payload) == 5 * vt.itemsize + 2 * ft.itemsize == 5 * 27 + 2 * 13
    rows = np.frombuffer(payload[:5 * vt.itemsize], dtype=vt)
    tris = np.frombuffer(payload[5 * vt.itemsize:], dtype=ft)
    assert np.array_equal(rows["p"], v) and np.array_equal(rows["n"], n) and np.array_equal(rows["c"], c)
    assert (tris["k"] == 3).all() and np.array_equal(tris["i"], f)
    F.write_ply(path, v, f)                                             # positions and faces alone
    raw = open(path, "rb").read()
    assert b"nx" not in raw and b"red" not in raw and len(raw.split(b"end_header\n", 1)[1]) == 5 * 12 + 2 * 13
