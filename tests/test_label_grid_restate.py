"""CPU tests of the label grid: the numpy restatement (tests/_label_grid_restate.py) against hand-computed cases, ``editing.about``
against the written-out numpy expression, and the argument checks that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _label_grid_restate as LR
import _skip_restate as RS

NAN = float("nan")


# ---- the restatement against cases worked out by hand
def test_label_row_by_hand():
    C = 4
    row = lambda sigma, *logits: np.array([0.1, 0.2, 0.3, sigma, *logits], dtype=np.float32)
    assert LR.label_row(row(1.0, 0.0, 2.0, 2.0, 1.0), C, 0.0) == 1            # a tie: the first of the two
    assert LR.label_row(row(1.0, 0.0, 0.0, 0.0, 5.0), C, 0.0) == 3            # the last channel is a label like any other
    assert LR.label_row(row(0.5, 9.0, 0.0, 0.0, 0.0), C, 0.5) == 255          # sigma == threshold: not above it
    assert LR.label_row(row(0.0, 0.0, 0.0, 0.0, 1.0), C, 0.0) == 255          # the empty row
    assert LR.label_row(row(NAN, 9.0, 0.0, 0.0, 0.0), C, 0.0) == 255          # NaN sigma
    assert LR.label_row(row(1.0, NAN, 7.0, 8.0, 9.0), C, 0.0) == 0            # NaN in channel 0 is never replaced
    assert LR.label_row(row(1.0, 1.0, NAN, 0.5, 0.0), C, 0.0) == 0            # NaN elsewhere is never chosen
    assert LR.label_row(row(1.0, 1.0, NAN, 3.0, NAN), C, 0.0) == 2
    assert LR.label_row(row(1.0, -np.inf, -np.inf, -np.inf, -np.inf), C, 0.0) == 0
    assert LR.label_row(np.array([0, 0, 0, 2.0, -3.0], np.float32), 1, 0.0) == 0       # C = 1
    got = LR.label_cells(np.stack([row(1.0, 0, 2, 2, 1), row(0.0, 0, 0, 0, 1)]), C)
    assert got.dtype == np.uint8 and got.tolist() == [1, 255]


def test_label_stats_by_hand():
    lab = np.full((2, 3, 4), 255, np.uint8)
    lab[0, 1, 2] = 1
    lab[1, 2, 3] = 1
    lab[1, 0, 0] = 0
    lab[0, 0, 0] = 5                                                          # >= C: ignored
    count, s, lo, hi = LR.label_stats(lab, 3)
    assert count.tolist() == [1, 2, 0]
    assert s.tolist() == [[1, 0, 0], [1, 3, 5], [0, 0, 0]]
    assert lo.tolist() == [[1, 0, 0], [0, 1, 2], [2, 3, 4]]                   # a label without a cell keeps dims ...
    assert hi.tolist() == [[2, 1, 1], [2, 3, 4], [0, 0, 0]]                   # ... and 0
    d = LR.derived(count, s, lo, hi, (0.0, 0.0, 0.0), (2.0, 3.0, 4.0), (2, 3, 4))        # unit cells
    assert d["centre"][0].tolist() == [1.5, 0.5, 0.5] and d["centre"][1].tolist() == [1.0, 2.0, 3.0]
    assert np.isnan(d["centre"][2]).all()
    assert d["box_lo"][1].tolist() == [0.0, 1.0, 2.0] and d["box_hi"][1].tolist() == [2.0, 3.0, 4.0]
    assert d["volume"].tolist() == [1.0, 2.0, 0.0]
    d = LR.derived(count, s, lo, hi, (-1.0, 0.0, 2.0), (0.0, 6.0, 3.0), (2, 3, 4))       # cells 0.5 x 2 x 0.25
    assert d["centre"][1].tolist() == [-0.5, 4.0, 2.75] and d["volume"][1] == 0.5


def test_skip_words_by_hand():
    assert LR.mask_words(3) == [8, 0, 0, 0] and LR.mask_words([0, 33, 127]) == [1, 2, 0, 1 << 31]
    lab = np.array([3, 255, 127, 3, 0] + [255] * 28 + [3], np.uint8)          # 34 cells: two words
    assert LR.skip_words(lab, LR.mask_words(3)).tolist() == [0b1001, 0b10]
    assert LR.skip_words(lab, LR.mask_words([127, 0])).tolist() == [0b10100, 0]
    assert LR.skip_words(lab, [0, 0, 0, 0]).tolist() == [0, 0]
    assert LR.skip_words(lab, [0xffffffff] * 4).tolist() == [0b11101, 0b10]   # 255 is never set


def test_label_rays_by_hand():
    o, d, z = LR.label_rays((0.0, 0.0, 0.0), (2.0, 3.0, 4.0), (2, 3, 4))
    assert o.shape == (6, 3) and o[0].tolist() == [0.5, 0.5, 0.5] and o[5].tolist() == [1.5, 2.5, 0.5]
    assert d.tolist() == [[0.0, 0.0, 1.0]] * 6 and z.tolist() == [[0.0, 1.0, 2.0, 3.0]] * 6
    o1, _, _ = LR.label_rays((0.0, 0.0, 0.0), (2.0, 3.0, 4.0), (2, 3, 4), 1, 2)
    assert np.array_equal(o1, o[3:])
    for lo, hi, dims in (((-1.3, 0.2, -2.0), (1.1, 1.9, 0.7), (5, 6, 7)), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (8, 8, 33))):
        o, d, z = LR.label_rays(lo, hi, dims)                                 # (asserts that every point lies in its cell)
        centres = RS.cell_centres(lo, hi, dims).reshape(dims + (3,))
        assert np.array_equal(o, centres[:, :, 0, :].reshape(-1, 3))
    with pytest.raises(AssertionError):                                       # f32 cannot resolve half a cell this far out
        LR.label_rays((1e8, 0.0, 0.0), (1e8 + 64, 1.0, 1.0), (64, 2, 2))


# ---- editing.about
def r_z(t):
    return np.array([[np.cos(t), -np.sin(t), 0, 0], [np.sin(t), np.cos(t), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def written_out(matrix, centre):
    """tools/pose_generator.py:67-77 written out: float32 translations, float64 product."""
    t = np.eye(4, 4, dtype=np.float32)
    t[:3, -1] = -1 * np.array(centre)
    t_inv = np.eye(4, 4, dtype=np.float32)
    t_inv[:3, -1] = -1 * t[:3, -1]
    return t_inv @ matrix @ t


def test_about_matches_the_written_out_expression():
    from dm_nerf_amd import editing as Ed
    centre = [0.779178, 1.05247, 0.380208]
    r = r_z(90 * np.pi / 180)
    s = np.diag([1.2, 1.2, 1.2, 1.0])
    t = np.array([[1, 0, 0, 0], [0, 1, 0, -0.25], [0, 0, 1, 0], [0, 0, 0, 1]])
    for m in (r, s, s @ r @ t):                                               # rotation, scale, the reference's "multi"
        got = Ed.about(m, centre)
        assert got.dtype == np.float64 and got.shape == (4, 4)
        assert np.array_equal(got, written_out(m, centre))
    c32 = np.asarray(centre, np.float32).astype(np.float64)                   # the centre is rounded to f32: it is the fixed point
    assert np.allclose(Ed.about(r, centre) @ np.append(c32, 1.0), np.append(c32, 1.0), rtol=0, atol=1e-15)
    assert np.array_equal(Ed.about(np.eye(4), centre), np.eye(4))
    assert np.array_equal(Ed.about(torch.eye(4).numpy() * 2, np.zeros(3)), np.diag([2.0, 2.0, 2.0, 2.0]))
    for bad_m, bad_c in ((np.eye(3), centre), (np.eye(4), [0.0, 1.0])):
        with pytest.raises(ValueError, match="about"):
            Ed.about(bad_m, bad_c)


def test_object_centre_reads_a_stats_dict():
    from dm_nerf_amd import editing as Ed
    stats = {"count": torch.tensor([2, 0]), "centre": torch.tensor([[1.0, 2.0, 3.0], [NAN, NAN, NAN]], dtype=torch.float64)}
    got = Ed.object_centre(stats, 0)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="owns no cell"):
        Ed.object_centre(stats, 1)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="outside"):
            Ed.object_centre(stats, bad)


# ---- argument checks that run before anything touches a device
def test_entries_validate_arguments():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                                   # never dereferenced: every call below is refused
    mask = (ctypes.c_uint32 * 4)()
    for C in (0, 129):
        assert lib.dmnerf_label_cells(p, 4, C, 0.0, p, None) == -1 and "C=" in _lib.last_error()
        assert lib.dmnerf_label_stats(p, 2, 2, 2, C, p, p, p, p, None) == -1 and "C=" in _lib.last_error()
    assert lib.dmnerf_label_cells(p, -1, 14, 0.0, p, None) == -1
    for thr in (-1.0, NAN):
        assert lib.dmnerf_label_cells(p, 4, 14, thr, p, None) == -1 and "sigma_threshold" in _lib.last_error()
    assert lib.dmnerf_label_cells(None, 4, 14, 0.0, p, None) == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_label_cells(None, 0, 14, 0.0, None, None) == 0          # nothing to do
    assert lib.dmnerf_label_stats(p, 0, 2, 2, 14, p, p, p, p, None) == -1 and "dims" in _lib.last_error()
    assert lib.dmnerf_label_stats(p, 2048, 2048, 512, 14, p, p, p, p, None) == -1 and "int32" in _lib.last_error()
    assert lib.dmnerf_label_stats(p, 2, 2, 2, 14, p, None, p, p, None) == -1 and "null" in _lib.last_error()
    for n in (0, 1 << 31):
        assert lib.dmnerf_skip_grid_from_labels(p, n, mask, p, None) == -1 and "n_cells" in _lib.last_error()
    assert lib.dmnerf_skip_grid_from_labels(p, 8, None, p, None) == -1 and "null" in _lib.last_error()


def test_python_layer_validates_arguments():
    from dm_nerf_amd import field as F
    for thr in (-0.5, NAN):
        with pytest.raises(ValueError, match="sigma_threshold"):
            F.label_grid(None, None, sigma_threshold=thr)
    with pytest.raises(TypeError, match="SkipGrid"):
        F.label_grid(None, "grid")
    assert F.label_mask_words(3, 14) == LR.mask_words(3) and F.label_mask_words([0, 33, 127], 128) == LR.mask_words([0, 33, 127])
    assert F.label_mask_words([], 14) == [0, 0, 0, 0]
    for bad in (14, -1, [2, 14], 1.5):
        with pytest.raises(ValueError):
            F.label_mask_words(bad, 14)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # tensors live on the device, as everywhere in the package
        F.LabelGrid.from_labels(torch.zeros(2, 2, 2, dtype=torch.uint8), (0, 0, 0), (1, 1, 1))
