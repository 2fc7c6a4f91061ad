"""The numpy restatement of the skip grid (tests/_skip_restate.py) against hand-built cases: the GPU tests compare the kernels with
it, so it is checked on its own first."""
import numpy as np

import _skip_restate as R


def cells(words, dims):
    return {tuple(int(v) for v in c) for c in np.argwhere(R.unpack_bits(words, dims))}


def box(c, d, dims):
    return {(i, j, k) for i in range(max(c[0] - d, 0), min(c[0] + d, dims[0] - 1) + 1)
            for j in range(max(c[1] - d, 0), min(c[1] + d, dims[1] - 1) + 1)
            for k in range(max(c[2] - d, 0), min(c[2] + d, dims[2] - 1) + 1)}


def test_single_cell_dilation_at_a_face_and_a_corner():
    dims = (5, 6, 7)
    for c in ((2, 0, 3), (0, 0, 0), (4, 5, 6), (2, 3, 3)):           # a face, two corners, the interior
        sigma = np.zeros(dims, dtype=np.float32)
        sigma[c] = 1.0
        for d, n_interior in ((0, 1), (1, 27), (2, 125)):
            got = cells(R.build(sigma, 0.0, d), dims)
            assert got == box(c, d, dims)
            if c == (2, 3, 3) and d < 2:
                assert len(got) == n_interior
    sigma = np.zeros(dims, dtype=np.float32)
    sigma[0, 0, 0] = 1.0
    assert len(cells(R.build(sigma, 0.0, 1), dims)) == 8 and len(cells(R.build(sigma, 0.0, 2), dims)) == 27   # clipped at the corner


def test_threshold_is_strict_and_nan_is_occupied():
    sigma = np.array([[[0.5, 0.5000001, np.nan, -1.0, 0.0]]], dtype=np.float32)
    assert R.unpack_bits(R.build(sigma, 0.5, 0), sigma.shape).reshape(-1).tolist() == [False, True, True, False, False]
    assert R.unpack_bits(R.build(sigma, 0.0, 0), sigma.shape).reshape(-1).tolist() == [True, True, True, False, False]


def test_bit_packing_with_a_partly_used_last_word():
    dims = (3, 5, 7)                                                # 105 cells: 3 full words + 9 bits
    occ = np.zeros(dims, dtype=bool)
    occ[0, 0, 0] = occ[0, 4, 3] = occ[2, 4, 6] = True               # g = 0, 31, 104
    occ[0, 4, 4] = True                                             # g = 32: bit 0 of word 1
    w = R.pack_bits(occ)
    assert w.dtype == np.uint32 and w.shape == (4,)
    assert w.tolist() == [1 | (1 << 31), 1, 0, 1 << 8]
    assert np.array_equal(R.unpack_bits(w, dims), occ)
    full = R.pack_bits(np.ones(dims, dtype=bool))
    assert full.tolist() == [0xFFFFFFFF] * 3 + [(1 << 9) - 1]        # the unused bits stay 0


def test_fast_dilation_equals_the_loops():
    rng = np.random.RandomState(3)
    for dims in ((5, 7, 9), (1, 4, 2), (6, 1, 1)):
        occ = rng.rand(*dims) < 0.08
        for d in (0, 1, 2):
            assert np.array_equal(R.dilate_clipped_fast(occ, d), R.dilate_clipped(occ, d))


def test_select_boundaries_policies_and_nan():
    dims = (4, 4, 4)
    lo, hi = (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)                       # cell 0.5: every product below is exact
    occ = np.zeros(dims, dtype=bool)
    occ[1, 0, 0] = occ[3, 3, 3] = True
    w = R.pack_bits(occ)
    o = np.array([[0.0, 0.25, 0.25],                                # along +x through cells (0..3, 0, 0)
                  [0.0, 0.25, 0.25],
                  [np.nan, 0.0, 0.0],
                  [1.75, 1.75, 1.75]], dtype=np.float32)
    d = np.array([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.25, 0.25, 0.25]], dtype=np.float32)
    z = np.array([[0.25, 0.5, 0.75, 1.0],      # x = .25 (cell 0), .5 (exactly on the boundary: cell 1), .75 (cell 1), 1.0 (cell 2)
                  [-0.25, 1.99, 2.0, 3.0],     # x < lo (outside), cell 3, exactly on hi (outside), beyond
                  [0.0, 1.0, 2.0, 3.0],        # NaN point: outside
                  [0.0, 0.5, 1.0, 2.0]],       # (1.75..)=cell 3,3,3; 1.875; 2.0 exactly on hi: outside; 2.25 outside
                 dtype=np.float32)
    flag, sel, count = R.select(o, d, z, w, lo, hi, dims, "evaluate")
    assert flag.tolist() == [[0, 1, 1, 0], [1, 0, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert sel.dtype == np.int32 and sel.tolist() == [1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15] and count == 13
    flag, sel, count = R.select(o, d, z, w, lo, hi, dims, "empty")
    assert flag.tolist() == [[0, 1, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]]
    assert sel.tolist() == [1, 2, 12, 13] and count == 4
    assert np.all(np.diff(sel) > 0)


def test_cell_centres_and_masking():
    c = R.cell_centres((-1.0, 0.0, 2.0), (1.0, 4.0, 3.0), (2, 4, 1))
    assert c.dtype == np.float32 and c.shape == (8, 3)
    assert c[0].tolist() == [-0.5, 0.5, 2.5] and c[-1].tolist() == [0.5, 3.5, 2.5] and c[1].tolist() == [-0.5, 1.5, 2.5]
    rows = np.arange(12, dtype=np.float32).reshape(2, 2, 3) + 1
    got = R.mask_rows(rows, np.array([[1, 0], [0, 1]], dtype=np.uint8))
    assert got[0, 0].tolist() == [1, 2, 3] and got[1, 1].tolist() == [10, 11, 12] and not got[0, 1].any() and not got[1, 0].any()
