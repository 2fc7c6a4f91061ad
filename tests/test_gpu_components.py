"""GPU tests of the connected components of a label volume (csrc/components.hip; ``field.LabelGrid.components`` / ``cleaned``,
``field.Components``, ``field.SkipGrid.cleaned``): every array against its numpy statement (tests/_components_restate.py) with
``torch.equal``.  The shapes come from the kernel's tile ``(TI, TJ, TK)``: volumes smaller than a tile, one exact tile, two tiles along
every axis (so every face, edge and corner between tiles exists) and dims that are no multiple of the tile."""

import numpy as np
import pytest
import torch

import _components_restate as CR
import _gpu

pytestmark = pytest.mark.gpu

U = CR.UNLABELLED
BOX = ((-1.0, -0.8, -1.2), (1.1, 0.9, 1.3))
REF = {}                                                             # restated components, shared by the tests and never modified


@pytest.fixture(scope="module")
def A():
    ns = _gpu.namespace()
    TI, TJ, TK = ns.F.COMPONENTS_TILE
    ns.T, ns.two = (TI, TJ, TK), (2 * TI, 2 * TJ, 2 * TK)
    return ns


def grid_of(A, v, C, cells=None):
    lab = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    if cells is None:
        return A.F.LabelGrid.from_labels(lab, *BOX, C)
    return A.F.BakedGrid.from_arrays(lab, torch.from_numpy(cells).cuda(), *BOX, C)


def restated(v, C, connectivity):
    key = (v.shape, v.tobytes(), C, connectivity)
    if key not in REF:
        REF[key] = CR.components(v, C, connectivity)
    return REF[key]


def check(A, v, C, connectivity, what=None):
    """``components()`` of ``v`` equals the restatement -> the restated ``(root, size)``."""
    v = np.ascontiguousarray(v)
    root, size = restated(v, C, connectivity)
    comp = grid_of(A, v, C).components(connectivity)
    assert comp.connectivity == connectivity and comp.dims == v.shape and comp.C == C
    assert comp.root.dtype == torch.int32 and comp.size.dtype == torch.int32
    assert torch.equal(comp.root.cpu(), torch.from_numpy(root)), (what, v.shape, connectivity)
    assert torch.equal(comp.size.cpu(), torch.from_numpy(size)), (what, v.shape, connectivity)
    return root, size


def n_components(root):
    return int((root.reshape(-1) == np.arange(root.size)).sum())


# ---- 1. components against the restatement
@pytest.mark.parametrize("connectivity,total", [(6, 921), (26, 57)])
def test_anchor_volume(A, connectivity, total):
    root, _ = check(A, CR.anchor_volume(), 3, connectivity)          # 9 x 10 x 37: no multiple of the tile
    assert n_components(root) == total


@pytest.mark.parametrize("connectivity", [6, 26])
def test_degenerate_shapes(A, connectivity):
    TI, TJ, TK = A.T
    for s, dims in enumerate([(1, 1, 1), (1, 1, 2 * TK + 6), (3, 1, 1), A.T, A.two]):
        rng = np.random.RandomState(s)
        v = rng.randint(0, 2, size=dims).astype(np.uint8)
        v[rng.rand(*dims) >= 0.7] = U
        check(A, v, 2, connectivity, "random")
        check(A, np.zeros(dims, np.uint8), 1, connectivity, "full")


@pytest.mark.parametrize("mirrored", [False, True])
def test_long_chain(A, mirrored):
    v = CR.serpentine(A.two)
    if mirrored:                                                     # the smallest index at the far end of the chain
        v = v[::-1, ::-1, ::-1]
    root, size = check(A, v, 1, 6, "serpentine")
    assert n_components(root) == 1 and size.max() == int((v == 0).sum())
    check(A, v, 1, 26, "serpentine")


@pytest.mark.parametrize("connectivity", [6, 26])
def test_one_label_everywhere(A, connectivity):
    dims = (A.two[0] + 3, A.two[1] + 1, A.two[2] + 5)
    root, size = check(A, np.full(dims, 4, np.uint8), 5, connectivity)
    assert np.all(root == 0) and np.all(size == root.size)


def test_checkerboards(A):
    odd = np.indices(A.two).sum(0) % 2
    even_only = np.where(odd == 0, 0, U).astype(np.uint8)
    root, size = check(A, even_only, 1, 6)
    assert size.max() == 1
    root, size = check(A, even_only, 1, 26)
    assert n_components(root) == 1
    both = odd.astype(np.uint8)
    root, size = check(A, both, 2, 6)
    assert np.all(size == 1)
    root, size = check(A, both, 2, 26)
    assert n_components(root) == 2


def test_seams(A):
    TI, TJ, TK = A.T
    far = (TI - 1, TJ - 1, TK - 1)
    pairs = {"face": [(1, 0, 0), (0, 1, 0), (0, 0, 1)], "edge": [(1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 1, -1), (1, -1, 0), (1, 0, -1)],
             "corner": [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]}
    for kind, offsets in pairs.items():
        for off in offsets:
            # the first cell sits at the tile's far corner on the axes the offset raises, at the near face of the next tile where it lowers
            a = tuple(far[x] if off[x] >= 0 else far[x] + 1 for x in range(3))
            b = tuple(a[x] + off[x] for x in range(3))
            for other in (0, 1):
                v = np.full(A.two, U, np.uint8)
                v[a], v[b] = 0, other
                for connectivity in (6, 26):
                    root, size = check(A, v, 2, connectivity, (kind, off, other))
                    joined = other == 0 and (kind == "face" or connectivity == 26)
                    assert n_components(root) == (1 if joined else 2) and size.max() == (2 if joined else 1), (kind, off, other, connectivity)


def test_label_range(A):
    rng = np.random.RandomState(5)
    dims = (5, 9, 40)
    v = rng.randint(0, 6, size=dims).astype(np.uint8)
    v[rng.rand(*dims) < 0.2] = U
    for C in (1, 3):
        root, size = check(A, v, C, 6)
        assert np.all(root[v >= C] == -1) and np.all(size[v >= C] == 0)
    w = np.where(rng.rand(*dims) < 0.5, 127, rng.randint(100, 256, size=dims)).astype(np.uint8)
    root, _ = check(A, w, 128, 26)
    assert np.all(root[w == 127] >= 0) and np.all(root[w >= 128] == -1)


def test_two_calls_give_equal_outputs(A):
    g = grid_of(A, CR.anchor_volume(), 3)
    for connectivity in (6, 26):
        a, b = g.components(connectivity), g.components(connectivity)
        assert torch.equal(a.root, b.root) and torch.equal(a.size, b.size)


# ---- 2. the filter
def scene():
    """16 x 12 x 40, C = 4: label 1 with components of 12, 12 (a tie), 5 and 1 cells, label 2 a block and a stray, label 0 noise."""
    rng = np.random.RandomState(11)
    v = np.full((16, 12, 40), U, np.uint8)
    v[10:12, 2:4, 30:33] = 1                                         # 12 cells, across the tile seam in i... and the larger root
    v[1:3, 2:4, 3:6] = 1                                             # 12 cells, the smaller root
    v[6, 6, 10:15] = 1
    v[15, 11, 39] = 1
    v[4:9, 7:11, 20:36] = 2
    v[0, 0, 39] = 2
    noise = rng.rand(*v.shape) < 0.03
    v[noise & (v == U)] = 0
    v[13, 0, 0] = 9                                                  # >= C
    cells = rng.randn(*v.shape, 4).astype(np.float32)
    cells[v == U] = 0.0
    cells[1, 2, 3, 0] = np.float32(np.nan)
    return v, cells


def check_cleaned(A, v, C, cells=None, **kw):
    grid = grid_of(A, v, C, cells)
    got, info = grid.cleaned(**{("labels" if k == "which" else k): x for k, x in kw.items()})
    want, want_cells, removed, kept = CR.cleaned(v, C, cells=cells, **kw)
    assert type(got) is type(grid) and got.dims == grid.dims and got.C == C
    assert np.array_equal(got.lo, grid.lo) and np.array_equal(got.hi, grid.hi)
    assert got.labels.dtype == torch.uint8 and torch.equal(got.labels.cpu(), torch.from_numpy(want)), kw
    for k, w in (("removed", removed), ("kept", kept)):
        assert info[k].dtype == torch.int64 and torch.equal(info[k].cpu(), torch.from_numpy(w)), (kw, k, info[k], w)
    assert torch.equal(info["removed"] + info["kept"], grid.stats()["count"])
    if cells is not None:
        assert torch.equal(got.cells.cpu().view(torch.int32), torch.from_numpy(want_cells).view(torch.int32)), kw
        gone = torch.from_numpy((want != v))
        assert bool((got.cells.cpu()[gone] == 0).all())
        assert torch.equal(got.cells.cpu()[~gone].view(torch.int32), torch.from_numpy(cells)[~gone].view(torch.int32))
    return got, info, want


@pytest.mark.parametrize("connectivity", [6, 26])
def test_filter_thresholds(A, connectivity):
    v, _ = scene()
    for m in (4, 5, 6, 11, 12, 13):                                  # round the components of 5 and of 12 cells
        _, info, want = check_cleaned(A, v, 4, min_cells=m, connectivity=connectivity, which=[1])
        assert int((want == 1).sum()) == {4: 29, 5: 29, 6: 24, 11: 24, 12: 24, 13: 0}[m]


def test_largest_with_a_tie(A):
    v, _ = scene()
    _, info, want = check_cleaned(A, v, 4, keep="largest")
    assert np.array_equal(want == 1, np.pad(np.ones((2, 2, 3), bool), ((1, 13), (2, 8), (3, 34))))     # the smaller root of the two
    assert want[0, 0, 39] == U and int((want == 2).sum()) == 5 * 4 * 16 and want[13, 0, 0] == 9
    check_cleaned(A, v, 4, keep="largest", min_cells=13, connectivity=26)


def test_label_subset_and_defaults(A):
    v, cells = scene()
    _, _, want = check_cleaned(A, v, 4, min_cells=2, which=[2])
    assert np.array_equal(want[v != 2], v[v != 2]) and want[0, 0, 39] == U
    check_cleaned(A, v, 4, min_cells=2, which=2)
    check_cleaned(A, v, 4, min_cells=2, which=[])
    got, info, want = check_cleaned(A, v, 4)                          # the defaults reproduce the input
    assert np.array_equal(want, v) and int(info["removed"].sum()) == 0
    got, info, want = check_cleaned(A, v, 4, cells)
    assert torch.equal(got.cells.cpu().view(torch.int32), torch.from_numpy(cells).view(torch.int32))


@pytest.mark.parametrize("kw", [dict(min_cells=6), dict(keep="largest"), dict(min_cells=2, connectivity=26, which=[0, 2])])
def test_baked_volume(A, kw):
    v, cells = scene()
    check_cleaned(A, v, 4, cells, **kw)


def test_edited_volume_is_accepted(A):
    v, cells = scene()
    res = A.Ed.edit_volume(grid_of(A, v, 4, cells), [A.Ed.Remove()], [0])
    got, _ = res["grid"].cleaned(keep="largest")
    want, want_cells, _, _ = CR.cleaned(res["grid"].labels.cpu().numpy(), 4, keep="largest", cells=res["grid"].cells.cpu().numpy())
    assert isinstance(got, A.F.BakedGrid) and torch.equal(got.labels.cpu(), torch.from_numpy(want))
    assert torch.equal(got.cells.cpu().view(torch.int32), torch.from_numpy(want_cells).view(torch.int32))


def test_the_motivating_case(A):
    v = np.full((20, 18, 70), U, np.uint8)
    v[3:9, 4:10, 5:25] = 2
    block = v.copy()
    v[19, 17, 69] = 2                                                # one stray cell in the far corner
    dirty, alone = grid_of(A, v, 3), grid_of(A, block, 3)
    assert dirty.stats()["hi_idx"][2].tolist() == [20, 18, 70]
    clean, info = dirty.cleaned(keep="largest")
    assert info["removed"].tolist() == [0, 0, 1]
    got, want = clean.stats(), alone.stats()
    for k in want:                                                   # (the centre of a label without a cell is NaN in both)
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=got[k].dtype == torch.float64), k
    centre = A.Ed.object_centre(clean, 2)
    assert np.array_equal(centre, A.Ed.object_centre(alone, 2)) and not np.array_equal(centre, A.Ed.object_centre(dirty, 2))
    lo, cell = clean.lo.astype(np.float64), clean.cell.astype(np.float64)
    assert np.allclose(centre, lo + (np.array([5.5, 6.5, 14.5]) + 0.5) * cell, rtol=0, atol=1e-12)


def test_bad_arguments(A):
    v, cells = scene()
    g, b = grid_of(A, v, 4), grid_of(A, v, 4, cells)
    for bad in (5, 18, "6", None, True):
        with pytest.raises(ValueError):
            g.components(bad)
    for kw in (dict(min_cells=0), dict(min_cells=1.5), dict(min_cells=2 ** 31), dict(keep="biggest"), dict(connectivity=8), dict(labels=[4]),
               dict(labels=-1), dict(out=g), dict(out=b), dict(out=grid_of(A, v, 5)), dict(out=grid_of(A, v[:8], 4)),
               dict(out=A.F.LabelGrid.from_labels(g.labels, *BOX, 4))):
        with pytest.raises(ValueError):
            g.cleaned(**kw)
    with pytest.raises(ValueError):
        A.F.SkipGrid.full(*BOX, (4, 4, 4)).cleaned(0)


# ---- 3. largest(), table(), SkipGrid.cleaned
@pytest.mark.parametrize("connectivity", [6, 26])
def test_largest_and_table(A, connectivity):
    for v, C in ((scene()[0], 4), (CR.anchor_volume(), 3), (np.full((3, 3, 3), U, np.uint8), 2)):
        grid = grid_of(A, v, C)
        comp = grid.components(connectivity)
        root, size = restated(v, C, connectivity)
        best = comp.largest()
        want_root, want_size = CR.largest(v, C, root, size)
        assert best["root"].dtype == torch.int32 and best["size"].dtype == torch.int32
        assert torch.equal(best["root"].cpu(), torch.from_numpy(want_root)) and torch.equal(best["size"].cpu(), torch.from_numpy(want_size))
        got, want = comp.table(), CR.table(v, C, root, size, grid.lo, grid.cell)
        stats = grid.stats()
        assert set(got) == set(want) == set(stats) | {"id", "label", "root"}
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == torch.from_numpy(want[k]).dtype, k
            if k in stats:
                assert got[k].dtype == stats[k].dtype and got[k].shape[1:] == stats[k].shape[1:], k
            if got[k].dtype == torch.float64:
                assert torch.allclose(got[k].cpu(), torch.from_numpy(want[k]), rtol=1e-12, atol=1e-12), k
            else:
                assert torch.equal(got[k].cpu(), torch.from_numpy(want[k])), k
        r = got["root"].cpu()
        assert bool((r[1:] > r[:-1]).all())                          # the id ranks ascend with the root
        assert torch.equal(got["id"].reshape(-1)[got["root"].long()].cpu(), torch.arange(r.shape[0], dtype=torch.int32))


def test_table_of_one_label_is_stats(A):
    v = np.full((9, 7, 35), U, np.uint8)
    v[2:5, 1:4, 3:30] = 1
    grid = grid_of(A, v, 2)
    t, s = grid.components().table(), grid.stats()
    for k in s:
        assert torch.equal(t[k][0], s[k][1]), k


@pytest.mark.parametrize("connectivity", [26, 6])
def test_skip_grid_cleaned(A, connectivity):
    dims = (7, 5, 9)                                                 # 315 bits: no whole number of words
    occ = np.random.RandomState(2).rand(*dims) < 0.3
    grid = A.F.SkipGrid.from_bits(CR.pack_bits(occ), *BOX, dims, outside="empty")
    for m in (1, 2, 4):
        got = grid.cleaned(m, connectivity=connectivity)
        want, _, _, _ = CR.cleaned(np.where(occ, 0, U).astype(np.uint8), 1, connectivity=connectivity, min_cells=m)
        assert got.outside == "empty" and got.dims == dims and np.array_equal(got.lo, grid.lo) and np.array_equal(got.hi, grid.hi)
        assert torch.equal(got.bits.cpu(), torch.from_numpy(CR.pack_bits(want == 0).view(np.int32))), m
    assert torch.equal(grid.cleaned(1).bits, grid.bits)


# ---- 4. graph capture
def test_captured_clean_follows_the_labels(A):
    v, cells = scene()
    rng = np.random.RandomState(3)
    w = rng.randint(0, 4, size=v.shape).astype(np.uint8)
    w[rng.rand(*v.shape) >= 0.4] = U
    w_cells = rng.randn(*v.shape, 4).astype(np.float32)
    w_cells[w == U] = 0.0
    live = grid_of(A, v, 4, cells)
    kw = dict(min_cells=3, keep="largest", connectivity=26)
    out, info = live.cleaned(**kw)                                   # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                    # one stream, no parallel branches
        got, info = live.cleaned(out=out, **kw)
    assert got is out
    for labels, baked in ((w, w_cells), (v, cells)):
        live.labels.copy_(torch.from_numpy(labels))
        live.cells.copy_(torch.from_numpy(baked))
        out.labels.fill_(77)
        info["removed"].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        want, want_cells, removed, kept = CR.cleaned(labels, 4, cells=baked, **kw)
        assert torch.equal(out.labels.cpu(), torch.from_numpy(want))
        assert torch.equal(out.cells.cpu().view(torch.int32), torch.from_numpy(want_cells).view(torch.int32))
        assert torch.equal(info["removed"].cpu(), torch.from_numpy(removed)) and torch.equal(info["kept"].cpu(), torch.from_numpy(kept))
