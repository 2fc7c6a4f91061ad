"""tests/_components_restate.py, the numpy statement of the connected components of a label volume, against scipy.ndimage.label per
label (wherever scipy imports) and on cases small enough to do by hand.  No device."""
import numpy as np
import pytest

import _components_restate as CR

U = CR.UNLABELLED


def partition_of(root):
    """The components as a set of frozensets of cell indices."""
    flat = root.reshape(-1)
    return {frozenset(np.nonzero(flat == r)[0].tolist()) for r in np.unique(flat[flat >= 0])}


def check_canonical(labels, C, root, size):
    flat, r, s = labels.reshape(-1), root.reshape(-1), size.reshape(-1)
    assert root.dtype == np.int32 and size.dtype == np.int32 and root.shape == labels.shape == size.shape
    assert np.array_equal(r >= 0, flat < C) and np.array_equal(s > 0, flat < C)
    for part in partition_of(root):
        cells = sorted(part)
        assert np.all(r[cells] == cells[0]) and np.all(s[cells] == len(cells)) and len(set(flat[cells].tolist())) == 1


def test_predecessors():
    assert CR.predecessors(6) == [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    p = CR.predecessors(26)
    assert len(p) == 13 and all(o < (0, 0, 0) for o in p) and len(set(p)) == 13


@pytest.mark.parametrize("connectivity,rank,total", [(6, 1, 921), (26, 3, 57)])
def test_anchor_volume_against_scipy(connectivity, rank, total):
    ndimage = pytest.importorskip("scipy.ndimage")
    v = CR.anchor_volume()
    root, size = CR.components(v, 3, connectivity)
    check_canonical(v, 3, root, size)
    want, n = set(), 0
    for l in range(3):
        lab, k = ndimage.label(v == l, structure=ndimage.generate_binary_structure(3, rank))
        n += k
        flat = lab.reshape(-1)
        want |= {frozenset(np.nonzero(flat == q)[0].tolist()) for q in range(1, k + 1)}
    assert n == total
    got = partition_of(root)
    assert got == want                                               # the same partition, hence the same sizes
    assert sorted(int(size.reshape(-1)[min(p)]) for p in got) == sorted(len(p) for p in want)


@pytest.mark.parametrize("connectivity,total", [(6, 921), (26, 57)])
def test_anchor_counts_without_scipy(connectivity, total):
    v = CR.anchor_volume()
    root, _ = CR.components(v, 3, connectivity)
    assert int((root.reshape(-1) == np.arange(v.size)).sum()) == total


def test_hand_cases():
    # a 2 x 2 x 2 volume: label 0 on one diagonal of the cube, label 1 on a face diagonal
    v = np.full((2, 2, 2), U, np.uint8)
    v[0, 0, 0] = v[1, 1, 1] = 0
    v[0, 1, 0] = v[0, 0, 1] = 1
    r6, s6 = CR.components(v, 2, 6)
    assert r6.reshape(-1).tolist() == [0, 1, 2, -1, -1, -1, -1, 7] and s6.reshape(-1).tolist() == [1, 1, 1, 0, 0, 0, 0, 1]
    r26, s26 = CR.components(v, 2, 26)
    assert r26.reshape(-1).tolist() == [0, 1, 1, -1, -1, -1, -1, 0] and s26.reshape(-1).tolist() == [2, 2, 2, 0, 0, 0, 0, 2]
    # a label >= C is unlabelled; different labels never join
    r, s = CR.components(np.array([[[0, 0, 1, 1, 2, 255]]], np.uint8), 2, 26)
    assert r.reshape(-1).tolist() == [0, 0, 2, 2, -1, -1] and s.reshape(-1).tolist() == [2, 2, 2, 2, 0, 0]
    # no wrap-around: the two ends of a row
    r, _ = CR.components(np.array([[[0, 255, 0]]], np.uint8), 1, 26)
    assert r.reshape(-1).tolist() == [0, -1, 2]
    # checkerboards: singletons at 6; at 26 one component per label
    g = np.indices((4, 4, 4)).sum(0) % 2
    even = np.where(g == 0, 0, U).astype(np.uint8)
    r, s = CR.components(even, 1, 6)
    assert np.array_equal(r.reshape(-1)[even.reshape(-1) == 0], np.nonzero(even.reshape(-1) == 0)[0]) and s.max() == 1
    r, s = CR.components(even, 1, 26)
    assert set(np.unique(r).tolist()) == {-1, 0} and s.max() == 32
    r, s = CR.components(g.astype(np.uint8), 2, 26)
    assert set(np.unique(r).tolist()) == {0, 1} and np.all(s == 32)
    r, s = CR.components(g.astype(np.uint8), 2, 6)
    assert np.array_equal(r.reshape(-1), np.arange(64)) and np.all(s == 1)


def test_serpentine_is_one_chain():
    for dims in ((4, 4, 6), (16, 16, 64)):
        v = CR.serpentine(dims)
        root, size = CR.components(v, 1, 6)
        n = int((v == 0).sum())
        assert set(np.unique(root).tolist()) == {-1, 0} and size.max() == n
        # a chain: two ends with one neighbour, every other cell with two
        pad = np.pad(v == 0, 1)
        nb = sum(np.roll(pad, s, a) for a in range(3) for s in (-1, 1))[1:-1, 1:-1, 1:-1]
        assert sorted(np.bincount(nb[v == 0]).tolist()) == [0, 2, n - 2]
        m = v[::-1, ::-1, ::-1]
        root, size = CR.components(m, 1, 6)
        assert set(np.unique(root).tolist()) == {-1, int(np.nonzero(m.reshape(-1) == 0)[0][0])} and size.max() == n


def test_filter_largest_and_table():
    v = np.full((3, 4, 5), U, np.uint8)
    v[0, 0, 0:3] = 1                                                 # label 1: sizes 3 (root 0), 3 (root 40), 1 (root 59)
    v[2, 0, 0:3] = 1
    v[2, 3, 4] = 1
    v[1, 1:3, 1:3] = 0                                               # label 0: one block of 4
    v[0, 3, 4] = 7                                                   # >= C
    cells = np.arange(v.size * 4, dtype=np.float32).reshape(v.shape + (4,)) + 1
    root, size = CR.components(v, 2, 6)
    br, bs = CR.largest(v, 2, root, size)
    assert br.tolist() == [26, 0] and bs.tolist() == [4, 3]          # the tie of label 1 goes to the smaller root
    out, oc, removed, kept = CR.cleaned(v, 2, min_cells=1, keep="all", cells=cells)
    assert np.array_equal(out, v) and np.array_equal(oc, cells) and removed.tolist() == [0, 0] and kept.tolist() == [4, 7]
    for m, gone in ((2, 1), (3, 1), (4, 7)):
        out, oc, removed, kept = CR.cleaned(v, 2, min_cells=m, cells=cells)
        assert removed.tolist() == [0, gone] and kept.tolist() == [4, 7 - gone]
        assert np.all(oc[(v == 1) & (out == U)] == 0) and np.array_equal(oc[out == v], cells[out == v])
    out, _, removed, kept = CR.cleaned(v, 2, keep="largest")
    assert removed.tolist() == [0, 4] and np.array_equal(np.nonzero(out.reshape(-1) == 1)[0], [0, 1, 2]) and out[0, 3, 4] == 7
    out, _, removed, _ = CR.cleaned(v, 2, min_cells=5, which=[0])
    assert removed.tolist() == [4, 0] and np.array_equal(out == 1, v == 1)
    t = CR.table(v, 2, root, size, lo=(-1.0, 0.0, 1.0), cell=(0.5, 0.25, 2.0))
    assert t["root"].tolist() == [0, 26, 40, 59] and t["label"].tolist() == [1, 0, 1, 1] and t["count"].tolist() == [3, 4, 3, 1]
    assert t["id"][2, 0, 1] == 2 and t["id"][0, 3, 4] == -1 and t["id"][1, 2, 2] == 1
    assert t["index_sum"][1].tolist() == [4, 6, 6] and t["lo_idx"][1].tolist() == [1, 1, 1] and t["hi_idx"][1].tolist() == [2, 3, 3]
    assert np.allclose(t["centre"][1], [-1.0 + 1.5 * 0.5, 2.0 * 0.25, 1.0 + 2.0 * 2.0]) and t["volume"].tolist() == [0.75, 1.0, 0.75, 0.25]
    assert np.array_equal(CR.pack_bits(np.arange(40) % 3 == 0), np.array([0x49249249, 0x92], np.uint32))
