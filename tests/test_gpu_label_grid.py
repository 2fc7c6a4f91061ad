"""GPU tests of the label grid: the three kernels of csrc/label_grid.hip on crafted inputs, ``field.label_grid`` / ``LabelGrid`` end to
end, ``editing.object_centre`` and a graph capture.  Labels, sums, bounds and bits are integers: every comparison is ``torch.equal``
against the numpy restatement of tests/_label_grid_restate.py; only ``stats()["centre"]`` is float64 (1e-12 relative).

The end-to-end model: ``oracle.ref_cpu.make_weights(72, ins_num, gain=1.7, sigma_bias=0.0)``, box ``LO .. HI``, ``occ`` = the cells
where ``RandomState(5).rand(*dims) < 0.6``.  Seed and scaling were picked on the CPU with the oracle alone
(``manipulator_nerf`` at the restated label points, then the restated label rule): it puts sigma > 0 at 76 % / 81 % of the cells of
the two grids, so 47 % of the cells are labelled behind that ``occ`` at threshold 0 and 22 % / 30 % at the 0.05 of the second test.
The labels below ``C - 1`` are, on the small grid, 8 (94 cells), 11 (3), 3 and 12 (1 each) for ins_num 13 and 44, 52, 33, 8, 89
(6 - 43 cells each) and three more for ins_num 93; on the large grid 8, 12, 11, 3 (24 - 888 cells) and 44, 52, 33, 89, 48, 8, 64
(8 - 571 cells).  The rare labels of the small grid sit at least 0.01 above the thresholds in sigma and 0.006 in the logit gap, a
thousand times the f32 and f16x2 deviation.  (Seeds 71 and 73, and ``sigma_bias=0.3``, gave sigma > 0 everywhere or one dominant
label.)  The tests assert both conditions on what the GPU returns."""
import ctypes

import numpy as np
import pytest
import torch

import _label_grid_restate as LR
import _skip_restate as RS
from _gpu import A, model_from  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
LO, HI = (-1.5, -1.2, -1.0), (1.5, 1.3, 2.0)
GRIDS = ((5, 6, 7), (8, 8, 33))                 # 210 cells: 6 words and 18 bits; 2112 cells = 66 whole words, dz no multiple of 16


# ---- the kernels on crafted inputs
def cells_kernel(A, raw, C, thr=0.0):
    raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda()
    M = raw.shape[0]
    out = torch.full((M + 1,), 77, dtype=torch.uint8, device="cuda")          # one guard byte behind the labels
    A.L.check(A.lib.dmnerf_label_cells(A.L.ptr(raw), M, C, thr, A.L.ptr(out), A.L.stream()), "dmnerf_label_cells")
    assert int(out[M]) == 77
    return out[:M].cpu()


def crafted_rows(M, C, seed):
    """Random rows with, cyclically: a tie of two channels, the maximum in channel C - 1, sigma == threshold (0.5), a NaN sigma, a NaN
    in channel 0, NaNs in other channels, the empty row, a plain row."""
    rng = np.random.RandomState(seed)
    raw = rng.randn(M, 4 + C).astype(np.float32)
    raw[:, 3] = np.abs(raw[:, 3]) + 1.0
    for m in range(M):
        kind = m % 8
        if kind == 0 and C > 1:
            a, b = sorted(rng.choice(C, 2, replace=False))
            raw[m, 4 + a] = raw[m, 4 + b] = 9.0
        elif kind == 1:
            raw[m, 4 + C - 1] = 9.0
        elif kind == 2:
            raw[m, 3] = 0.5
        elif kind == 3:
            raw[m, 3] = NAN
        elif kind == 4:
            raw[m, 4] = NAN
        elif kind == 5 and C > 1:
            raw[m, 4 + rng.choice(np.arange(1, C), min(3, C - 1), replace=False)] = NAN
        elif kind == 6:
            raw[m] = 0.0
            raw[m, -1] = 1.0
    return raw


@pytest.mark.parametrize("C", [1, 14, 94, 128])
@pytest.mark.parametrize("M", [1, 31, 33, 257])
def test_label_cells_edges(A, C, M):
    raw = crafted_rows(M, C, 100 * C + M)
    want = LR.label_cells(raw, C, 0.5)
    got = cells_kernel(A, raw, C, 0.5)
    assert torch.equal(got, torch.from_numpy(want))
    if M >= 31:                                                               # the crafted kinds did what they are there for
        assert want[2] == want[3] == want[6] == 255 and want[4] == 0
        if C > 1:
            assert want[1] == C - 1 and want[0] < C - 1 and want[5] != 255


def test_label_cells_rules_one_by_one(A):
    C = 4
    rows = np.array([[0, 0, 0, 1.0, 0, 2, 2, 1],            # tie -> the first
                     [0, 0, 0, 1.0, 0, 0, 0, 5],            # channel C - 1 is kept as a label
                     [0, 0, 0, 0.5, 9, 0, 0, 0],            # sigma == threshold
                     [0, 0, 0, NAN, 9, 0, 0, 0],            # NaN sigma
                     [0, 0, 0, 1.0, NAN, 7, 8, 9],          # NaN in channel 0: never replaced
                     [0, 0, 0, 1.0, 1, NAN, 3, NAN],        # NaN elsewhere: never chosen
                     [0, 0, 0, 0.0, 0, 0, 0, 1]], np.float32)             # the empty row
    assert cells_kernel(A, rows, C, 0.5).tolist() == [1, 3, 255, 255, 0, 2, 255]
    assert cells_kernel(A, rows, C, 0.0).tolist() == [1, 3, 0, 255, 0, 2, 255]


def stats_kernel(A, labels, C):
    dims = tuple(labels.shape)
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(labels).cuda()
    count = torch.full((C + 1,), -7, dtype=torch.int64, device="cuda")        # poisoned, with a guard row each
    s = torch.full((C + 1, 3), -7, dtype=torch.int64, device="cuda")
    lo = torch.full((C + 1, 3), -7, dtype=torch.int32, device="cuda")
    hi = torch.full((C + 1, 3), -7, dtype=torch.int32, device="cuda")
    L = A.L
    L.check(L.load().dmnerf_label_stats(L.ptr(lab), *dims, C, L.ptr(count), L.ptr(s), L.ptr(lo), L.ptr(hi), L.stream()), "dmnerf_label_stats")
    for t in (count, s, lo, hi):
        assert bool((t[C] == -7).all())
    return [t[:C].cpu() for t in (count, s, lo, hi)]


def assert_stats(got, labels, C):
    for g, w in zip(got, LR.label_stats(labels, C)):
        assert g.dtype == torch.from_numpy(w).dtype and torch.equal(g, torch.from_numpy(w))


def test_label_stats_edges(A):
    dims = (3, 5, 70)
    empty = np.full(dims, 255, np.uint8)
    got = stats_kernel(A, empty, 14)
    assert_stats(got, empty, 14)
    assert got[0].tolist() == [0] * 14 and got[2].tolist() == [list(dims)] * 14 and got[3].tolist() == [[0, 0, 0]] * 14
    corner = empty.copy()
    corner[-1, -1, -1] = 13
    got = stats_kernel(A, corner, 14)
    assert_stats(got, corner, 14)
    assert got[0][13] == 1 and got[1][13].tolist() == [2, 4, 69] and got[2][13].tolist() == [2, 4, 69] and got[3][13].tolist() == [3, 5, 70]
    filled = np.full(dims, 6, np.uint8)
    got = stats_kernel(A, filled, 14)
    assert_stats(got, filled, 14)
    assert got[0][6] == 1050 and got[2][6].tolist() == [0, 0, 0] and got[3][6].tolist() == [3, 5, 70]
    assert_stats(stats_kernel(A, filled, 6), filled, 6)                       # labels >= C are ignored
    rng = np.random.RandomState(9)
    vol = rng.randint(0, 100, (7, 9, 33)).astype(np.uint8)                    # 0 .. 93 are labels, 94 .. 99 and 255 are not
    vol[rng.rand(7, 9, 33) < 0.2] = 255
    assert_stats(stats_kernel(A, vol, 94), vol, 94)
    assert_stats(stats_kernel(A, vol, 128), vol, 128)
    blobs = np.repeat(rng.randint(0, 5, (7, 9, 3)).astype(np.uint8), 11, axis=2)          # runs of equal labels along k
    assert_stats(stats_kernel(A, blobs, 14), blobs, 14)
    # a volume that does not start on a 16-byte boundary takes the byte loads
    buf = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), vol.reshape(-1)])).cuda()
    view = buf[3:].reshape(7, 9, 33)
    assert view.data_ptr() % 16 != 0
    assert_stats(stats_kernel(A, view, 94), vol, 94)
    twice = [stats_kernel(A, vol, 94) for _ in range(2)]                      # integer atomics: the same every run
    assert all(torch.equal(a, b) for a, b in zip(*twice))


def bits_kernel(A, labels, words4):
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)).cuda()
    n = lab.numel()
    n_words = (n + 31) // 32
    bits = torch.full((n_words + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")       # poisoned: every word must be written
    mask = (ctypes.c_uint32 * 4)(*words4)
    L = A.L
    L.check(L.load().dmnerf_skip_grid_from_labels(L.ptr(lab), n, mask, L.ptr(bits), L.stream()), "dmnerf_skip_grid_from_labels")
    assert int(bits[n_words]) == 0x5A5A5A5A
    return bits[:n_words].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 7 * 9 * 33])
def test_skip_grid_from_labels_edges(A, n):
    rng = np.random.RandomState(n)
    lab = rng.choice(np.array([0, 3, 31, 32, 63, 64, 93, 127, 128, 200, 255], np.uint8), n)
    lab[-1] = 127                                                             # the last cell is set under every mask that holds 127
    for words4 in ([0, 0, 0, 0], LR.mask_words(127), LR.mask_words([0, 32, 64, 93]), [0xffffffff] * 4):
        want = LR.skip_words(lab, words4)
        got = bits_kernel(A, lab, words4)
        assert np.array_equal(got, want)
        cells = RS.unpack_bits(got, (1, 1, n)).reshape(-1)
        assert not cells[lab >= 128].any()                                    # 128, 200 and 255 are never set
        if n & 31:
            assert int(got[-1]) >> (n & 31) == 0                              # the tail bits of the last word
    assert not bits_kernel(A, lab, [0, 0, 0, 0]).any()
    only127 = RS.unpack_bits(bits_kernel(A, lab, LR.mask_words(127)), (1, 1, n)).reshape(-1)
    assert np.array_equal(only127, lab == 127) and only127[-1]


# ---- end to end
_models = {}


def model(A, ins_num):
    if ins_num not in _models:
        _models[ins_num] = model_from(O.make_weights(72, ins_num, gain=1.7, sigma_bias=0.0), ins_num)
    return _models[ins_num]


def occ_cells(dims):
    return np.random.RandomState(5).rand(*dims) < 0.6


def occ_grid(A, dims, cells=None):
    return A.F.SkipGrid.from_bits(RS.pack_bits(occ_cells(dims) if cells is None else cells), LO, HI, dims)


def cell_rays(dims):
    return [torch.from_numpy(t).cuda() for t in LR.label_rays(LO, HI, dims)]


def assert_not_vacuous(labels, C):
    lab = labels.cpu().numpy().reshape(-1)
    frac = float((lab != 255).mean())
    objects = np.unique(lab[lab < C - 1])
    print(f"labelled {frac:.3f}, labels below C - 1: {objects.tolist()}")
    assert 0.10 <= frac <= 0.90, frac
    assert objects.size >= 2, objects


@pytest.mark.parametrize("split", [None, "f16x2"])
@pytest.mark.parametrize("ins_num", [13, 93])
@pytest.mark.parametrize("dims", GRIDS)
def test_label_grid_is_the_rule_on_the_network_rows(A, dims, ins_num, split):
    mf, C = model(A, ins_num), ins_num + 1
    occ = occ_grid(A, dims)
    with torch.no_grad():
        lg = A.F.label_grid(mf, occ, split=split, slab=3 * dims[1] * dims[2])             # more than one slab, a ragged last one
        o, d, z = cell_rays(dims)
        raw = A.R.run_network_skip(mf, o, d, z, occ, split=split)
    assert isinstance(lg, A.F.LabelGrid) and lg.dims == dims and lg.C == C and lg.labels.dtype == torch.uint8
    assert np.array_equal(lg.lo, occ.lo) and np.array_equal(lg.hi, occ.hi) and np.array_equal(lg.cell, occ.cell)
    want = LR.label_cells(raw.cpu().numpy().reshape(-1, 4 + C), C, 0.0).reshape(dims)
    assert torch.equal(lg.labels.cpu(), torch.from_numpy(want))
    assert_not_vacuous(lg.labels, C)
    with torch.no_grad():
        one = A.F.label_grid(mf, occ, split=split)                                        # one slab: the same labels
    assert torch.equal(one.labels, lg.labels)


@pytest.mark.parametrize("ins_num", [13, 93])
@pytest.mark.parametrize("dims", GRIDS)
def test_label_grid_select_wiring_against_the_dense_network(A, dims, ins_num):
    mf, C, thr = model(A, ins_num), ins_num + 1, 0.05
    occ = occ_grid(A, dims)
    with torch.no_grad():
        lg = A.F.label_grid(mf, occ, sigma_threshold=thr)
        dense = A.R.run_network(mf, *cell_rays(dims)).reshape(dims + (4 + C,))
        full = A.F.label_grid(mf, A.F.SkipGrid.full(LO, HI, dims), sigma_threshold=thr)
        none = A.F.label_grid(mf, A.F.SkipGrid.empty(LO, HI, dims), sigma_threshold=thr)
    above = dense[..., 3] > thr
    labelled = lg.labels != 255
    assert torch.equal(labelled, occ.unpack() & above)                        # selected rows are the dense rows bit for bit
    assert torch.equal(lg.labels[labelled].long(), dense[..., 4:].argmax(-1)[labelled])
    assert_not_vacuous(lg.labels, C)
    assert bool((none.labels == 255).all())
    assert torch.equal(full.labels != 255, above)
    assert torch.equal(full.labels[above].long(), dense[..., 4:].argmax(-1)[above])


@pytest.fixture(scope="module")
def labelled(A):
    dims = GRIDS[1]
    with torch.no_grad():
        return A.F.label_grid(model(A, 13), occ_grid(A, dims))


def test_skip_grid_of_labels(A, labelled):
    lab = labelled.labels
    present = [int(l) for l in torch.unique(lab).tolist() if l != 255]
    a, b = present[0], present[-1]
    assert a != b
    ga, gb = labelled.skip_grid(a), labelled.skip_grid(b)
    assert isinstance(ga, A.F.SkipGrid) and ga.dims == labelled.dims and ga.outside == "evaluate"
    assert torch.equal(ga.unpack(), lab == a) and torch.equal(gb.unpack(), lab == b)
    both = labelled.skip_grid([a, b], outside="empty")
    assert both.outside == "empty" and torch.equal(both.bits, (ga | gb).bits)
    assert torch.equal(labelled.skip_grid(iter((b, a))).bits, both.bits)
    absent = next(l for l in range(14) if l not in present)
    assert not bool(labelled.skip_grid(absent).unpack().any())
    assert torch.equal(labelled.skip_grid(a, dilate=1).bits, ga.dilated(1).bits)
    assert torch.equal(labelled.skip_grid(range(14)).unpack(), lab != 255)
    for bad in (14, -1, [a, 14]):
        with pytest.raises(ValueError):
            labelled.skip_grid(bad)


def test_stats_and_object_centre(A, labelled):
    C = labelled.C
    st = labelled.stats()
    lab = labelled.labels.cpu().numpy()
    ints = LR.label_stats(lab, C)
    for key, want in zip(("count", "index_sum", "lo_idx", "hi_idx"), ints):
        assert torch.equal(st[key].cpu(), torch.from_numpy(want)), key
    want = LR.derived(*ints, LO, HI, labelled.dims)
    have = ints[0] > 0
    assert have.sum() >= 3 and not have.all()
    for key in ("centre", "box_lo", "box_hi", "volume"):
        got = st[key].cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want[key].shape
        rows = have if key == "centre" else slice(None)
        assert np.allclose(got[rows], want[key][rows], rtol=1e-12, atol=0), key
    assert np.isnan(st["centre"].cpu().numpy()[~have]).all()
    k = int(np.nonzero(have)[0][0])
    for source in (labelled, st):
        c = A.Ed.object_centre(source, k)
        assert isinstance(c, np.ndarray) and c.dtype == np.float64 and c.shape == (3,)
        assert np.allclose(c, want["centre"][k], rtol=1e-12, atol=0)
    assert np.all(c > want["box_lo"][k]) and np.all(c < want["box_hi"][k])
    absent = int(np.nonzero(~have)[0][0])
    with pytest.raises(ValueError, match="owns no cell"):
        A.Ed.object_centre(labelled, absent)
    given = A.F.LabelGrid.from_labels(labelled.labels.clone(), LO, HI)        # a given volume: every label below 128 counts
    assert given.C == 128 and torch.equal(given.stats()["count"][:C], st["count"])
    with pytest.raises(ValueError):
        A.F.LabelGrid.from_labels(labelled.labels.float(), LO, HI)


def test_capture_follows_the_bits(A):
    dims = GRIDS[0]
    mf = model(A, 13)
    first, second = occ_cells(dims), np.random.RandomState(6).rand(*dims) < 0.5
    occ = occ_grid(A, dims, first)
    with torch.no_grad():
        eager = [A.F.label_grid(mf, occ_grid(A, dims, c)) for c in (first, second)]       # (also the warm-up: blob, empty row, kernels)
        eager_stats = [e.stats() for e in eager]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            lg = A.F.label_grid(mf, occ)                                      # dims[0] planes fit one slab
            st = lg.stats()
    assert not torch.equal(eager[0].labels, eager[1].labels)
    for cells, e, es in ((second, eager[1], eager_stats[1]), (first, eager[0], eager_stats[0])):
        occ.bits.copy_(occ_grid(A, dims, cells).bits)                         # in place: the capture holds the pointer
        lg.labels.fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lg.labels, e.labels)
        for key in ("count", "index_sum", "lo_idx", "hi_idx"):
            assert torch.equal(st[key], es[key]), key
        assert torch.equal(torch.nan_to_num(st["centre"], nan=-1.0), torch.nan_to_num(es["centre"], nan=-1.0))
