"""The numpy statement of csrc/field_edit.hip (tests/_field_edit_restate.py) held against hand-built cases, a float64 referee of the
owner, and plain Python loops for the selection and the kept counts.  No GPU: tests/test_gpu_field_edit.py holds the kernels against
the same statement bit for bit."""
import numpy as np
import pytest

import _field_edit_restate as R
import _volume_edit_restate as V
from dm_nerf_amd.editing import FIELD_POLICIES, Copy, Remove, edit_kind, edit_label_sets, field_edit_masks

f32 = np.float32
BOX16 = ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))                      # 16^3, cell 1.0: every whole-cell map is exact
DIMS16 = (16, 16, 16)


def consts16():
    lo, cell, inv_cell = V.grid_consts(*BOX16, DIMS16)
    assert np.all(cell == 1.0) and np.all(inv_cell == 1.0)
    return lo, inv_cell


def x_rays(y, zc, x0=-7.5, n=1):
    """``n`` rays along +x through the centres of the cells (., y, zc)."""
    o = np.tile(np.array([[x0, y + 0.5 - 8.0, zc + 0.5 - 8.0]], dtype=f32), (n, 1))
    d = np.tile(np.array([[1.0, 0.0, 0.0]], dtype=f32), (n, 1))
    return o, d


# ---- hand-built cases
def test_whole_cell_translation_carries_the_ray_back_exactly():
    lo, inv_cell = consts16()
    src = np.zeros(DIMS16, dtype=np.uint8)
    src[4:7, 5, 5] = 1                                             # entry 0 owns three cells of the row (., 5, 5)
    shift = np.array([3.0, -2.0, 1.0])
    entries = [(R.MOVE, 3, V.translation(shift))]
    o, d = x_rays(5, 5)
    z = np.arange(16, dtype=f32)[None]                              # p_x = -7.5 + s: the centre of cell s
    out = R.select(src, lo, inv_cell, entries, o, d, z)
    want = np.zeros(16, dtype=np.uint8)
    want[4:7] = 1
    assert np.array_equal(out["owner"], want)
    assert out["count"] == 16 and np.array_equal(out["sel"], np.arange(16))
    mine = want == 1
    assert np.array_equal(out["o_w"][mine], np.tile(o[0] + shift.astype(f32), (3, 1)))      # exact: everything is dyadic
    assert np.array_equal(out["d_w"][mine], np.tile(d[0], (3, 1)))                          # no translation of the direction
    assert np.array_equal(out["o_w"][~mine].view(np.uint32), np.tile(o[0], (13, 1)).view(np.uint32))
    # the carried-back point is M p: the cell of o_w + d_w z is the cell of p shifted by (3, -2, 1)
    inside, g = R.cells_f32(out["o_w"][mine], out["d_w"][mine], z[0, mine][:, None], lo, inv_cell, DIMS16)
    assert inside.all() and np.array_equal(g[:, 0], [((s + 3) * 16 + 3) * 16 + 6 for s in (4, 5, 6)])


def test_a_sample_exactly_on_a_face_belongs_to_the_upper_cell():
    lo, inv_cell = consts16()
    src = np.zeros(DIMS16, dtype=np.uint8)
    src[3, 5, 5] = R.NOBODY                                         # the cell [-5, -4) is nobody's; [-6, -5) is its own
    o, d = x_rays(5, 5)
    below = np.nextafter(np.nextafter(f32(2.5), f32(0)), f32(0))     # (two steps: one step below 2.5 still sums to -5.0 in f32)
    z = np.array([[2.5, below, 3.5, 15.5]], dtype=f32)              # p_x = -5.0 exactly, just below, -4.0, 8.0
    out = R.select(src, lo, inv_cell, [], o, d, z, unowned=R.EMPTY, outside=R.EMPTY)
    assert out["owner"].tolist() == [R.NOBODY, 0, 0, R.NOBODY]      # -5.0 -> cell 3; below -> cell 2; -4.0 -> cell 4; 8.0 = hi: outside
    ref, face = R.owner_referee(src, *BOX16, [], o, d, z, unowned=R.EMPTY, outside=R.EMPTY)
    assert np.array_equal(ref, out["owner"]) and face[0] == 0.0 and face[2] == 0.0


@pytest.mark.parametrize("outside", [R.EVALUATE, R.EMPTY])
@pytest.mark.parametrize("unowned", [R.EVALUATE, R.EMPTY])
def test_outside_and_unowned_samples_under_both_policies(outside, unowned):
    lo, inv_cell = consts16()
    src = np.zeros(DIMS16, dtype=np.uint8)
    src[2, 5, 5] = R.NOBODY
    src[3, 5, 5] = 1
    entries = [(R.COPY, 2, V.translation([1.0, 0.0, 0.0]))]
    o, d = x_rays(5, 5, x0=-9.5)
    z = np.array([[0.0, 1.0, 4.0, 5.0, 6.0, 18.0]], dtype=f32)     # x = -9.5 out, -8.5 out, -5.5 cell 2, -4.5 cell 3, -3.5 cell 4, 8.5 out
    rows = np.full((6, 6), 7.0, dtype=f32)
    out = R.select(src, lo, inv_cell, entries, o, d, z, outside=outside, unowned=unowned, rows=rows, fill_row=R.empty_row(2))
    po, pu = (0 if outside == R.EVALUATE else 255), (0 if unowned == R.EVALUATE else 255)
    want = [po, po, pu, 1, 0, po]
    assert out["owner"].tolist() == want
    ev = np.array(want) != 255
    assert out["count"] == ev.sum() and np.array_equal(out["sel"], np.nonzero(ev)[0])
    assert np.all(out["rows"][ev] == 7.0) and np.array_equal(out["rows"][~ev], np.tile(R.empty_row(2), ((~ev).sum(), 1)))
    assert np.isnan(out["o_w"][~ev]).all() and not np.isnan(out["o_w"][ev]).any()


def test_a_remove_owned_byte_and_a_byte_past_the_list_read_as_unowned():
    lo, inv_cell = consts16()
    src = np.zeros(DIMS16, dtype=np.uint8)
    src[2, 5, 5], src[3, 5, 5], src[4, 5, 5], src[5, 5, 5] = 1, 2, 3, 254     # entry 0 (REMOVE), entry 1 (MOVE), past E = 2, past E
    entries = [(R.REMOVE, 1, None), (R.MOVE, 0, V.translation([0.0, 1.0, 0.0]))]
    o, d = x_rays(5, 5)
    z = np.array([[2.0, 3.0, 4.0, 5.0, 6.0]], dtype=f32)
    for unowned, u in ((R.EVALUATE, 0), (R.EMPTY, 255)):
        out = R.select(src, lo, inv_cell, entries, o, d, z, unowned=unowned)
        assert out["owner"].tolist() == [u, 2, u, u, 0]
    assert np.array_equal(out["o_w"][1], o[0] + np.array([0.0, 1.0, 0.0], dtype=f32))


def test_nan_rays_are_outside():
    lo, inv_cell = consts16()
    src = np.ones(DIMS16, dtype=np.uint8)
    entries = [(R.MOVE, 0, V.translation([1.0, 0.0, 0.0]))]
    o, d = x_rays(5, 5, n=4)
    o[1, 1] = np.nan
    d[2, 2] = np.inf                                                # inf * 0 = NaN at z = 0, inf elsewhere
    d[3, 0] = np.nan
    z = np.tile(np.array([[0.0, 3.0]], dtype=f32), (4, 1))
    ev = R.select(src, lo, inv_cell, entries, o, d, z, outside=R.EVALUATE)
    em = R.select(src, lo, inv_cell, entries, o, d, z, outside=R.EMPTY)
    assert ev["owner"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and em["owner"].tolist() == [1, 1] + [255] * 6
    assert ev["count"] == 8 and em["count"] == 2 and em["sel"].tolist() == [0, 1]
    # a sample evaluated on its own ray keeps that ray bit for bit, NaN included
    assert np.array_equal(ev["o_w"][2:].view(np.uint32), np.repeat(o[1:], 2, axis=0).view(np.uint32))
    assert np.array_equal(ev["d_w"][2:].view(np.uint32), np.repeat(d[1:], 2, axis=0).view(np.uint32))


@pytest.mark.parametrize("C", [2, 14, 128])
def test_filter_ties_nan_logits_and_masks(C):
    entries = [(R.MOVE, C - 1, None), (R.COPY, 0, None), (R.REMOVE, 1 % C, None)]
    masks = R.accept_masks(C, entries)
    gone = {C - 1, 1 % C}
    assert [bool(V._in_mask(l, masks[0])) for l in range(C)] == [l not in gone for l in range(C)]
    assert [l for l in range(C) if V._in_mask(l, masks[1])] == [C - 1] and [l for l in range(C) if V._in_mask(l, masks[2])] == [0]
    assert not masks[3].any()
    raw = np.zeros((8, 4 + C), dtype=f32)
    raw[:, :4] = np.arange(32, dtype=f32).reshape(8, 4) + 1.0
    raw[0, 4:] = 2.0                                               # all equal: the first, label 0
    raw[1, 4 + C - 1] = 5.0                                        # label C - 1
    raw[2, 4:] = np.nan                                            # NaN in channel 0 is never replaced: label 0
    raw[3, 4 + C - 1] = np.nan                                     # a NaN in a later channel is never chosen: label 0 (ties)
    raw[4, 4 + C - 1] = 5.0                                        # label C - 1, owner 1: accepted
    raw[5, 4 + C - 1] = 5.0                                        # label C - 1, owner 2: not label 0
    raw[6, 4 + C - 1] = 5.0                                        # owner 255: left alone whatever it holds
    raw[7, 4] = 1.0                                                # label 0, owner 3 (the REMOVE entry): accepts nothing
    owner = np.array([0, 0, 0, 0, 1, 2, 255, 3], dtype=np.uint8)
    assert R.labels_of(raw).tolist() == [0, C - 1, 0, 0, C - 1, C - 1, C - 1, 0]
    fill = R.empty_row(C)
    out, kept = R.filter_rows(raw, owner, masks, fill)
    filled = [1, 5, 7]                                             # label C - 1 moved away; not the copy's label; nothing accepted
    for m in range(8):
        if m in filled:
            assert np.array_equal(out[m], fill), m
        else:
            assert np.array_equal(out[m].view(np.uint32), raw[m].view(np.uint32)), m
    assert kept.tolist() == [3, 1, 0, 0] and kept.tolist() == R.brute_kept(raw, owner, masks)
    # keep_labels: every set is intersected with it
    masks_k = R.accept_masks(C, entries, keep=[0])
    assert [l for l in range(C) if V._in_mask(l, masks_k[0])] == ([0] if 0 not in gone else [])
    assert not masks_k[1].any() or C == 1


# ---- the product's host side: the policies and the accept masks editing.FieldEdit hands to the filter
def test_policy_constants_are_the_products():
    assert FIELD_POLICIES == {"evaluate": R.EVALUATE, "empty": R.EMPTY}


@pytest.mark.parametrize("C", [2, 14, 128])
@pytest.mark.parametrize("keep", [None, "some"])
def test_product_masks_equal_the_restatement_and_say_what_the_issue_says(C, keep):
    m = np.eye(4)
    trans = [m, Copy(m), Remove(), Copy(m), m]
    labels = [C - 1, 0, 1 % C, C // 2, 0]
    kinds = [edit_kind(t) for t in trans]
    assert kinds == [R.MOVE, R.COPY, R.REMOVE, R.COPY, R.MOVE]
    keep = None if keep is None else sorted({0, C - 1, C // 2})
    entries = list(zip(kinds, labels, [None] * 5))
    words = field_edit_masks(C, labels, kinds, keep)
    assert words == R.accept_masks(C, entries, keep).ravel().tolist()
    # stated from the issue, not from either implementation: owner 0 accepts keep minus the labels of MOVE and REMOVE entries;
    # owner 1 + e accepts {target_labels[e]} & keep (a REMOVE entry owns nothing)
    allowed = set(range(C)) if keep is None else set(keep)
    moved_or_removed = {labels[0], labels[2], labels[4]}
    want = [allowed - moved_or_removed] + [({l} & allowed) if k != R.REMOVE else set() for l, k in zip(labels, kinds)]
    rows = np.asarray(words, dtype=np.uint32).reshape(6, 4)
    for w, accept in enumerate(want):
        assert {l for l in range(128) if V._in_mask(l, rows[w])} == accept, w
    own, per_entry = edit_label_sets(C, labels, kinds, keep)
    assert set(own) == want[0] and [set(s) for s in per_entry] == want[1:]


# ---- the float64 referee
@pytest.mark.parametrize("dims", [(7, 5, 9), (19, 17, 23)])
def test_owner_against_the_float64_referee(dims):
    """The f32 owner may differ from the float64 one only where the float64 point lies within 1e-4 cells of a face, and such samples
    may be at most 0.5 % of all.  Observed with these seeded rays (1031 rays x 64 samples, 65 984 samples): 7 x 5 x 9: 36 samples
    (0.0546 %) within 1e-4 of a face, 0 owners differ; 19 x 17 x 23: 41 samples (0.0621 %), 0 owners differ -- under either policy pair."""
    lo, cell, inv_cell = V.grid_consts(*R.BOX, dims)
    E = 3
    entries = V.random_entries(E, 14, seed=8, lo=R.BOX[0], hi=R.BOX[1])
    src = R.random_source(dims, E, seed=21)
    o, d, z = R.random_rays(1031, 64, seed=4)
    for outside, unowned in ((R.EVALUATE, R.EMPTY), (R.EMPTY, R.EVALUATE)):
        got = R.select(src, lo, inv_cell, entries, o, d, z, outside=outside, unowned=unowned)["owner"]
        ref, face = R.owner_referee(src, *R.BOX, entries, o, d, z, outside=outside, unowned=unowned)
        near = face < 1e-4
        print(f"dims {dims}: {near.sum()} of {near.size} samples ({100.0 * near.mean():.4f} %) within 1e-4 of a face, "
              f"{(got != ref).sum()} owners differ")
        assert near.mean() <= 0.005
        assert not ((got != ref) & ~near).any()
    assert len(set(got.tolist())) >= 4                              # own, an entry, nobody: the rays do meet the volume


# ---- plain loops
@pytest.mark.parametrize("E", [0, 1, 3, 32])
def test_selection_and_kept_counts_against_plain_loops(E):
    dims, C = (7, 5, 9), 14
    lo, cell, inv_cell = V.grid_consts(*R.BOX, dims)
    entries = V.random_entries(E, C, seed=5 + E, lo=R.BOX[0], hi=R.BOX[1])
    src = R.random_source(dims, E, seed=3 + E)
    o, d, z = R.random_rays(37, 7, seed=9)
    rng = np.random.RandomState(E)
    raw = rng.randn(37 * 7, 4 + C).astype(f32)
    out = R.select(src, lo, inv_cell, entries, o, d, z, unowned=R.EMPTY, rows=raw, fill_row=R.empty_row(C))
    sel, count = R.brute_sel(out["owner"])
    assert out["count"] == count and out["sel"].tolist() == sel and 0 < count < 37 * 7
    assert all(int(b) == 255 or (int(b) <= E and (b == 0 or entries[b - 1][0] != R.REMOVE)) for b in out["owner"])
    masks = R.accept_masks(C, entries, keep=None if E != 3 else [0, 1, 5, 7, 13])
    filt, kept = R.filter_rows(out["rows"], out["owner"], masks, R.empty_row(C))
    assert kept.tolist() == R.brute_kept(out["rows"], out["owner"], masks)
    assert kept.sum() + np.all(filt == R.empty_row(C), axis=1).sum() >= 37 * 7       # every row is kept, filled, or was empty already
