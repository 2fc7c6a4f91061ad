"""GPU tests of ``field.object_surfaces`` / ``ObjectSurfaces`` (csrc/object_surface.hip).  The kernels claim the arithmetic and the
order of the loop over the labels round ``extract_surface`` (tests/_object_surface_restate.py), so every array of every label is
compared with ``torch.equal``.  (Where a case plants NaN values, a NaN must sit at the same place on both sides and everything else
must be equal: ``torch.equal`` itself calls no NaN equal to another.)"""
import os
import re

import numpy as np
import pytest
import torch

import _object_surface_restate as OS
import _surface_restate as S
from _gpu import A  # noqa: F401
from dm_nerf_amd import editing as E
from dm_nerf_amd import field as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL = 0.45


def tile():
    src = open(os.path.join(ROOT, "dm_nerf_amd", "csrc", "object_surface.hip")).read()
    m = re.search(r"constexpr int OS_TI = (\d+), OS_TJ = (\d+), OS_TK = (\d+);", src)
    return tuple(int(x) for x in m.groups())


def same(t, a):
    a = torch.from_numpy(np.ascontiguousarray(a))
    t = t.cpu()
    if t.dtype != a.dtype or t.shape != a.shape:
        return False
    if t.is_floating_point():
        return torch.equal(torch.isnan(t), torch.isnan(a)) and torch.equal(torch.nan_to_num(t, nan=7.0), torch.nan_to_num(a, nan=7.0))
    return torch.equal(t, a)


def grid_of(labels, C, cell=(0.5, 0.25, 0.125)):
    dims = np.asarray(labels.shape, dtype=np.float64)
    return F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), (0.0, 0.0, 0.0), tuple(dims * np.asarray(cell)), C)


def check(labels, value, C, level=LEVEL, closed=True, select=None, want=None):
    """One call against the referee: the five tensors and every label's slices -> ``(got, want)``."""
    if want is None:
        want = OS.object_surfaces(labels, value, C, level, closed, select=None if select is None else set(np.atleast_1d(select).tolist()))
    got = F.object_surfaces(grid_of(labels, C), torch.from_numpy(value).cuda(), level, labels=select, closed=closed)
    print(f"{labels.shape} C {C} closed {closed} select {select}: V {len(want.vertices)} F {len(want.faces)} "
          f"objects {sum(len(f) > 0 for _, f in want.objects)}")
    assert same(got.vertex_offset, want.vertex_offset) and same(got.face_offset, want.face_offset)
    assert same(got.vertices, want.vertices) and same(got.faces, want.faces) and same(got.vertex_cell, want.vertex_cell)
    for k in range(C):
        v, f = got.object(k)
        assert same(v, want.objects[k][0]) and same(f, want.objects[k][1]), k
    return got, want


_shared = {}


def voronoi14():
    """The C = 14 input and its closed referee, computed once and shared (read only)."""
    if "v14" not in _shared:
        labels, value = OS.voronoi((24, 20, 28), 14, 14, 1)
        _shared["v14"] = (labels, value, OS.object_surfaces(labels, value, 14, LEVEL, True))
    return _shared["v14"]


# ---- 1. shapes round the tile, closed and open
def shapes():
    ti, tj, tk = tile()
    return [(1, 1, 1), (2, 2, 2), (5, 7, 9), (ti + 1, tj + 1, tk + 1), (2 * ti + 1, tj + 2, tk + 2)]


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("n", range(5))
def test_shapes_round_the_tile(A, n, closed):
    shape = shapes()[n]
    labels, value = OS.voronoi(shape, 5, 4, 10 + n)
    if n < 2:
        labels[...], value[...] = 1, 0.9                                 # tiny volumes: all inside, so the surface is the border's
    _, want = check(labels, value, 5, closed=closed)
    assert (len(want.faces) > 0) == (closed or n >= 2)


# ---- 2. smooth field, Voronoi labels
def test_voronoi_14_objects(A):
    labels, value, want = voronoi14()
    check(labels, value, 14, want=want)
    assert all(len(f) > 0 for _, f in want.objects)
    check(labels, value, 14, closed=False)


def test_voronoi_94_labels_most_absent(A):
    labels, value = OS.voronoi((22, 18, 26), 94, 9, 2)
    _, want = check(labels, value, 94)
    assert sum(len(f) > 0 for _, f in want.objects) <= 9 < 94


# ---- 3. hand-placed cases
def hand_placed():
    C = 8
    labels = np.full((7, 7, 7), 255, dtype=np.uint8)
    value = np.zeros((7, 7, 7), dtype=np.float32)
    for c, (oi, oj, ok) in enumerate(S.CORNERS):                         # the cell at (1, 1, 1): 8 corners, 8 labels, all inside
        labels[1 + oi, 1 + oj, 1 + ok], value[1 + oi, 1 + oj, 1 + ok] = c, 0.5 + 0.05 * c
    labels[4:6, 4, 4], value[4:6, 4, 4] = (0, 1), (0.8, 0.7)             # two face-adjacent objects, both inside
    labels[4, 1, 5], value[4, 1, 5] = 2, np.float32(LEVEL)               # exactly at the level: outside
    labels[4, 1, 1:3], value[4, 1, 1:3] = 3, (0.9, np.nan)               # a NaN neighbour of the same label: outside, its NaN enters t
    labels[5, 1, 4], value[5, 1, 4] = 255, 50.0                          # owned by nobody, large values
    labels[5, 2, 4], value[5, 2, 4] = C + 1, 60.0
    labels[1, 4, 1:4], value[1, 4, 1:4] = 4, (0.2, 0.9, 0.3)             # same-label neighbours below the level: their real values enter
    labels[1, 5, 2], value[1, 5, 2] = 5, 0.4                             # ... and another label's below-level neighbour does not
    return labels, value, C


@pytest.mark.parametrize("closed", [True, False])
def test_hand_placed_cases(A, closed):
    labels, value, C = hand_placed()
    got, want = check(labels, value, C, closed=closed)
    assert all(len(want.objects[k][1]) >= 1 for k in range(C))           # the 8-label cell gives every object a triangle of its own
    assert np.isnan(want.objects[3][0]).any()
    v4 = want.objects[4][0]
    along_k = sorted(v[2] for v in v4 if v[0] == 1 and v[1] == 4)        # the planted run of label 4 along k: 0.2, 0.9, 0.3
    assert len(along_k) == 2 and abs(along_k[0] - (1 + 0.25 / 0.7)) < 1e-6 and along_k[1] == 2.75      # the real 0.2 and 0.3 (fill: 1.5, 2.5)
    along_j = sorted(v[1] for v in v4 if v[0] == 1 and v[2] == 2)
    assert along_j == [3.5, 4.5]                                         # towards label 5's 0.4: fill (its real value would give 4.9)
    assert not np.any((want.vertices[:, 0] > 4.5) & (want.vertices[:, 1] > 0.5) & (want.vertices[:, 1] < 2.5)
                      & (np.abs(want.vertices[:, 2] - 4) < 1))           # nothing round the 50.0 and the 60.0
    if closed:
        shared = [[v for v in want.objects[k][0] if 4 < v[0] < 5 and v[1] == 4 and v[2] == 4] for k in (0, 1)]
        assert len(shared[0]) == 1 and len(shared[1]) == 1               # two vertices on the shared grid edge, one per object


# ---- 4. labels= subsets and the empty volume
def test_label_subsets_and_the_empty_volume(A):
    labels, value, full = voronoi14()
    for select in ([2, 5, 13], 3, []):
        got, _ = check(labels, value, 14, select=select)
        vo, fo = got.vertex_offset.tolist(), got.face_offset.tolist()
        for k in range(14):
            if k in set(np.atleast_1d(select).tolist()):
                v, f = got.object(k)
                assert same(v, full.objects[k][0]) and same(f, full.objects[k][1])
            else:
                assert vo[k] == vo[k + 1] and fo[k] == fo[k + 1]
    got, _ = check(np.full((5, 6, 7), 255, dtype=np.uint8), np.ones((5, 6, 7), dtype=np.float32), 14)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.vertex_cell.shape == (0,)
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert not got.vertex_offset.any() and not got.face_offset.any() and got.vertex_offset.shape == (15,)
    # a plain LabelGrid without value: 1.0 everywhere, blocky surfaces half-way (level 0.5) between cells
    blocky = F.object_surfaces(grid_of(labels, 14), level=0.5)
    want = OS.object_surfaces(labels, np.ones(labels.shape, dtype=np.float32), 14, 0.5, True)
    assert same(blocky.vertices, want.vertices) and same(blocky.faces, want.faces) and same(blocky.vertex_offset, want.vertex_offset)
    assert set(np.unique(want.vertices * 2 % 2).tolist()) <= {0.0, 1.0}


# ---- 5. against the existing device code, object by object
def test_each_object_equals_extract_surface_on_its_padded_masked_volume(A):
    labels, value, _ = voronoi14()
    got = F.object_surfaces(grid_of(labels, 14), torch.from_numpy(value).cuda(), LEVEL)
    normals = got.normals()
    vo = got.vertex_offset.tolist()
    dl, dv = torch.from_numpy(labels).cuda(), torch.from_numpy(value).cuda()
    for k in range(14):
        padded = torch.nn.functional.pad(torch.where(dl == k, dv, torch.zeros_like(dv)), (1, 1, 1, 1, 1, 1), value=0.0).contiguous()
        v, f = F.extract_surface(padded, LEVEL)
        ov, of = got.object(k)
        assert torch.equal(v - 1.0, ov) and torch.equal(f, of), k
        assert torch.equal(F.vertex_normals(ov.contiguous(), of.contiguous()), normals[vo[k]:vo[k + 1]]), k


# ---- 6. measures
def test_measures_within_the_summation_order_bound_and_the_same_bits_twice(A):
    labels, value, want = voronoi14()
    grid = grid_of(labels, 14)
    got = F.object_surfaces(grid, torch.from_numpy(value).cuda(), LEVEL)
    m = got.measures()
    ref = OS.measures(want.objects, grid.cell.astype(np.float64))
    nf = np.diff(want.face_offset).astype(np.float64)
    for name in ("area", "volume"):
        g = m[name].cpu().numpy()
        assert g.dtype == np.float64 and g.shape == (14,)
        err, bound = np.abs(g - ref[name]), nf * 2.0 ** -52 * ref[name + "_abs"]
        print(name, "worst error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (name, err, bound)
        assert np.all(g > 0)
    again = F.object_surfaces(grid, torch.from_numpy(value).cuda(), LEVEL).measures()
    assert torch.equal(m["area"], again["area"]) and torch.equal(m["volume"], again["volume"])


# ---- 7. cleaned
def test_cleaned_equals_the_restated_clean_of_every_object(A):
    labels, value, C = OS.box_objects()
    labels[0, 6, 7], value[0, 6, 7] = 0, 0.9                             # a speck of object 0, apart from its block: 8 triangles
    want = OS.object_surfaces(labels, value, C, LEVEL, True)
    got = F.object_surfaces(grid_of(labels, C), torch.from_numpy(value).cuda(), LEVEL)
    m = 9                                                                # the speck and the one-cell object 2 go, the blocks stay
    clean = got.cleaned(min_triangles=m)
    vo_old = got.vertex_offset.tolist()
    vo, removed = clean.vertex_offset.tolist(), 0
    for k in range(C):
        v, f = want.objects[k]
        rv, rn, rf, rkept = S.clean(v, S.vertex_normals(v, f), f, min_triangles=m)
        cv, cf = clean.object(k)
        assert same(cv, rv.reshape(-1, 3)) and same(cf, rf), k
        assert same(clean.normals()[vo[k]:vo[k + 1]], rn.reshape(-1, 3)), k
        assert same(clean.kept_vertex_index[vo[k]:vo[k + 1]] - vo_old[k], rkept), k
        assert same(clean.vertex_cell[vo[k]:vo[k + 1]], want.vertex_cell[want.vertex_offset[k]:want.vertex_offset[k + 1]][rkept]), k
        removed += len(f) - len(rf)
    assert removed == 16 and len(clean.object(2)[1]) == 0 and len(clean.object(0)[1]) > 0


# ---- 8. end to end: a baked volume, one object moved by whole cells
def test_moved_object_keeps_its_surface_in_the_edited_volume(A):
    rng = np.random.default_rng(5)
    dims, C, voxel = (12, 11, 10), 6, 0.7
    labels = np.full(dims, 255, dtype=np.uint8)
    cells = np.zeros(dims + (4,), dtype=np.float32)
    labels[1:4, 1:5, 2:6] = 1                                            # the mover: constant sigma
    labels[6:10, 1:4, 1:5] = 2
    labels[2:9, 7:10, 6:9] = 4
    cells[..., :3] = rng.standard_normal(dims + (3,))
    cells[..., 3] = np.where(labels == 1, 2.0, np.where(labels == 255, 0.0, rng.uniform(0.3, 3.0, dims))).astype(np.float32)
    cell = 0.5
    hi = tuple(d * cell for d in dims)
    baked = F.BakedGrid.from_arrays(torch.from_numpy(labels).cuda(), torch.from_numpy(cells).cuda(), (0.0, 0.0, 0.0), hi, C)
    move = np.eye(4)
    move[:3, 3] = (-2 * cell, 0.0, -3 * cell)                            # a destination cell reads the source cell at + this
    edited = E.edit_volume(baked, [move], [1])["grid"]
    offset = (edited.stats()["lo_idx"][1] - baked.stats()["lo_idx"][1]).cpu()
    assert offset.abs().sum() == 5 and torch.equal(edited.stats()["count"], baked.stats()["count"])
    occ = 1.0 - torch.exp(-torch.relu(baked.cells[..., 3]) * voxel)
    level = float(occ[2, 2, 3]) / 2.0                                    # half the mover's value: t = 1 / 2 exactly, so i + t shifts exactly
    src, dst = F.object_surfaces(baked, voxel=voxel, level=level), F.object_surfaces(edited, voxel=voxel, level=level)
    for s, grid in ((src, baked), (dst, edited)):                        # both equal the referee on the device's own occupancy
        value = (1.0 - torch.exp(-torch.relu(grid.cells[..., 3]) * voxel)).cpu().numpy()
        want = OS.object_surfaces(grid.labels.cpu().numpy(), value, C, level, True)
        assert same(s.vertices, want.vertices) and same(s.faces, want.faces) and same(s.vertex_offset, want.vertex_offset)
        assert same(s.face_offset, want.face_offset) and same(s.vertex_cell, want.vertex_cell)
    for k in range(C):
        (sv, sf), (dv, df) = src.object(k), dst.object(k)
        shift = offset.float().cuda() if k == 1 else torch.zeros(3, device="cuda")
        assert torch.equal(sv + shift, dv) and torch.equal(sf, df), k
    assert len(src.object(1)[1]) > 0 and len(src.object(2)[1]) > 0 and len(src.object(4)[1]) > 0
    # the baked colour per vertex through vertex_cell: the mover's colours travel with it
    colour = lambda s, g: g.cells.reshape(-1, 4)[s.vertex_cell.long(), :3]
    v0, v1 = src.vertex_offset[1:3].tolist()
    assert torch.equal(colour(src, baked)[v0:v1], colour(dst, edited)[v0:v1])


# ---- 9. argument errors
def test_argument_errors(A, tmp_path):
    labels, value, C = OS.box_objects()
    grid, dv = grid_of(labels, C), torch.from_numpy(value).cuda()
    for level in (0.0, -0.1, float("inf"), float("nan"), 1e-60):
        with pytest.raises(ValueError, match="level"):
            F.object_surfaces(grid, dv, level)
    baked = F.BakedGrid.from_arrays(grid.labels, torch.zeros(labels.shape + (4,), device="cuda"), grid.lo, grid.hi, C)
    with pytest.raises(ValueError, match="voxel"):
        F.object_surfaces(baked)
    with pytest.raises(ValueError, match="value"):
        F.object_surfaces(grid, dv[:-1].contiguous())
    with pytest.raises(ValueError, match="value"):
        F.object_surfaces(grid, dv.double())
    with pytest.raises(RuntimeError, match="CPU"):
        F.object_surfaces(grid, torch.from_numpy(value))
    for bad in (C, -1, [0, C]):
        with pytest.raises(ValueError):
            F.object_surfaces(grid, dv, labels=bad)
    with pytest.raises(TypeError):
        F.object_surfaces(dv, dv)
    with pytest.raises(RuntimeError, match="CPU"):
        F.LabelGrid.from_labels(torch.from_numpy(labels), grid.lo, grid.hi, C)
    got = F.object_surfaces(grid, dv)
    with pytest.raises(ValueError):
        got.object(C)
    # the one host step: a file per non-empty object
    written = got.write(str(tmp_path / "object_{:03d}.ply"))
    assert [k for k, _ in written] == [0, 1, 2] and all(os.path.getsize(p) > 100 for _, p in written)
    w = got.world_vertices().cpu().numpy()
    assert np.array_equal(w, (grid.lo.astype(np.float64) + (got.vertices.cpu().numpy().astype(np.float64) + 0.5)
                              * grid.cell.astype(np.float64)).astype(np.float32))
