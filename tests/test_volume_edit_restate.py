"""``tests/_volume_edit_restate.py`` (the numpy statement of csrc/volume_edit.hip, which tests/test_gpu_volume_edit.py holds the kernel
to bit for bit) against plain array operations, a brute-force count in Python and its float64 referee -- and the argument checks of
``editing.edit_volume``, which come before anything touches a device.  No GPU.

Grids are 16^3 over [-8, 8)^3: cell 1.0, every centre and every whole-cell map dyadic, so f32 and float64 agree exactly there.
"""
import math

import numpy as np
import pytest

import _volume_edit_restate as V
from dm_nerf_amd import _lib, editing
from dm_nerf_amd.editing import edit_volume                       # (every test here needs the feature: the module does not import without it)

ENTRY = _lib.SIGNATURES["dmnerf_volume_edit"]
# the restatement speaks the product's numbers: the kinds of an entry, the rules, the limit of one call
assert [editing.edit_kind(t) for t in (np.eye(4), editing.Copy(np.eye(4)), editing.Remove())] == [V.MOVE, V.COPY, V.REMOVE]
assert editing.VOLUME_RULES == {"first": 0, "densest": 1} and editing.MAX_VOLUME_EDITS == 32

DIMS, LO, HI = V.SCENE_DIMS, V.SCENE_LO, V.SCENE_HI
CONSTS = V.grid_consts(LO, HI, DIMS)
C = 14
ALL = V.mask_words(range(C), C)
NAN = float("nan")


def run(labels, entries, cells=None, keep=ALL, rule=0, referee=False, Cn=C):
    return (V.referee if referee else V.edit)(labels, cells, *CONSTS, Cn, keep, entries, rule)


def brute(labels, sigma, Cn, keep, entries, rule):
    """The rules of the issue in plain Python over whole-cell shifts: an entry is ``(kind, label, (si, sj, sk))`` and reads the source cell
    ``destination + shift``.  -> labels, source, won, claimed, hits, and the winner's source cell per destination cell."""
    dims = labels.shape
    E = len(entries)
    out_l, out_s = np.full(dims, 255, np.uint8), np.full(dims, 255, np.uint8)
    src_of = {}
    won, claimed, hits = [0] * (1 + E), [0] * E, [[0] * Cn for _ in range(E)]
    gone = {l for k, l, _ in entries if k != V.COPY}
    for d in np.ndindex(*dims):
        cands = []
        l0 = int(labels[d])
        if l0 < Cn and l0 in keep and l0 not in gone:
            cands.append((0, l0, d))
        for e, (kind, label, shift) in enumerate(entries):
            s = tuple(d[a] + shift[a] for a in range(3))
            if kind != V.REMOVE and all(0 <= s[a] < dims[a] for a in range(3)) and int(labels[s]) == label and label in keep:
                cands.append((1 + e, label, s))
                claimed[e] += 1
        if not cands:
            continue
        best = cands[0]
        if rule == 1:
            for c in cands[1:]:
                s, b = float(sigma[c[2]]), float(sigma[best[2]])
                if not math.isnan(s) and (math.isnan(b) or s > b):
                    best = c
        out_l[d], out_s[d], src_of[d] = best[1], best[0], best[2]
        won[best[0]] += 1
        if len(cands) >= 2:
            for c in cands:
                if c[0] >= 1:
                    for b in cands:
                        if b[0] != c[0]:
                            hits[c[0] - 1][b[1]] += 1
    return out_l, out_s, np.array(won), np.array(claimed), np.array(hits).reshape(E, Cn), src_of


@pytest.mark.parametrize("kind", [V.MOVE, V.COPY])
def test_whole_cell_shift_equals_the_shifted_slice(kind):
    labels, _ = V.scene()
    move = (3, -2, 1)                                              # the object goes there: the map reads destination - move
    out = run(labels, [(kind, 3, V.translation([-3.0, 2.0, -1.0]))])
    want = labels.copy()
    if kind == V.MOVE:
        want[6:9, 5:9, 6:10] = 255
    block = labels[6:9, 5:9, 6:10]
    dest = want[6 + move[0]:9 + move[0], 5 + move[1]:9 + move[1], 6 + move[2]:10 + move[2]]
    dest[...] = np.where(dest == 255, block, dest)                 # ("first": what stands there stays)
    assert np.array_equal(out["labels"], want)
    assert out["claimed"][0] == block.size and out["won"].sum() + (out["labels"] == 255).sum() == labels.size
    moved = np.zeros(DIMS, bool)
    moved[6 + move[0]:9 + move[0], 5 + move[1]:9 + move[1], 6 + move[2]:10 + move[2]] = True
    assert np.array_equal(out["source"] == 1, moved)


def test_quarter_turn_about_a_cell_corner_equals_rot90():
    labels = np.full(DIMS, 255, dtype=np.uint8)
    labels[5:8, 6:11, 3:9] = 2                                     # asymmetric inside the 8 x 8 columns round the centre
    labels[9, 4, 2] = 2
    R = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    out = run(labels, [(V.MOVE, 2, editing.about(R, [0.0, 0.0, 0.0]))])
    want = np.full(DIMS, 255, dtype=np.uint8)
    # destination (x, y) reads the source at (-y, x): dest[a, b] = src[n - 1 - b, a] = rot90(src, -1)[a, b]
    want[4:12, 4:12, :] = np.rot90(labels[4:12, 4:12, :], -1, axes=(0, 1))
    assert np.array_equal(out["labels"], want)
    assert out["claimed"][0] == out["won"][1] == (labels == 2).sum() and not out["hits"].any()
    # about another cell-aligned centre: the same turn of the columns round it
    out = run(labels, [(V.MOVE, 2, editing.about(R, [-1.0, 1.0, 3.0]))])
    want = np.full(DIMS, 255, dtype=np.uint8)
    want[2:12, 4:14, :] = np.rot90(labels[2:12, 4:14, :], -1, axes=(0, 1))
    assert np.array_equal(out["labels"], want)


@pytest.mark.parametrize("scale", [2.0, 0.5])
def test_scale_about_a_cell_corner_equals_the_referee(scale):
    labels, cells = V.scene()
    m = editing.about(np.diag([scale, scale, scale, 1.0]), [-1.0, 0.0, 1.0])
    for kind in (V.MOVE, V.COPY):
        got, want = run(labels, [(kind, 3, m)], cells), run(labels, [(kind, 3, m)], cells, referee=True)
        for k in ("labels", "source", "won", "claimed", "hits"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["cells"].view(np.uint32), want["cells"].view(np.uint32))
        assert got["claimed"][0] > 0


def test_identity_and_no_edits():
    labels, cells = V.random_volume(DIMS, C, seed=1, baked=True)
    out = run(labels, [(V.MOVE, 3, np.eye(4))], cells)
    kept = np.where(labels < C, labels, 255)                       # (labels >= C are nobody's: they leave)
    assert np.array_equal(out["labels"], kept)
    assert np.array_equal(out["source"] == 1, labels == 3) and np.array_equal(out["source"] == 0, (kept != 255) & (labels != 3))
    assert np.array_equal(out["cells"].view(np.uint32), np.where((kept != 255)[..., None], cells.view(np.uint32), 0))
    keep = [0, 3, 13]
    out = run(labels, [], cells, keep=V.mask_words(keep, C))
    assert np.array_equal(out["labels"], np.where(np.isin(labels, keep), labels, 255))
    assert out["won"].tolist() == [int(np.isin(labels, keep).sum())] and out["claimed"].shape == (0,) and out["hits"].shape == (0, C)
    assert np.array_equal(out["source"], np.where(np.isin(labels, keep), 0, 255))


def test_remove_vacates_the_label_and_nothing_else():
    labels, cells = V.random_volume(DIMS, C, seed=2, baked=True)
    plain = run(labels, [], cells)
    out = run(labels, [(V.REMOVE, 5, None)], cells)
    gone = labels == 5
    assert (out["labels"][gone] == 255).all() and not out["cells"][gone].view(np.uint32).any() and (out["source"][gone] == 255).all()
    for k in ("labels", "source"):
        assert np.array_equal(out[k][~gone], plain[k][~gone])
    assert np.array_equal(out["cells"][~gone].view(np.uint32), plain["cells"][~gone].view(np.uint32))
    assert out["claimed"].tolist() == [0] and not out["hits"].any() and out["won"].tolist() == [plain["won"][0] - gone.sum(), 0]


@pytest.mark.parametrize("entries", V.COLLISIONS)
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("keep", [None, (1, 3, 5)])
def test_colliding_entries_pick_and_count_as_a_brute_force_count(entries, rule, keep):
    labels, cells = V.scene()
    entries = [(k, l, s if s is not None else (0, 0, 0)) for k, l, s in entries]
    keep_set = set(range(C)) if keep is None else set(keep)
    out = run(labels, V.shift_entries(entries), cells, keep=V.mask_words(sorted(keep_set), C), rule=rule)
    want_l, want_s, won, claimed, hits, src_of = brute(labels, cells[..., 3], C, keep_set, entries, rule)
    assert np.array_equal(out["labels"], want_l) and np.array_equal(out["source"], want_s)
    assert np.array_equal(out["won"], won) and np.array_equal(out["claimed"], claimed) and np.array_equal(out["hits"], hits)
    assert out["won"].sum() + (out["labels"] == 255).sum() == labels.size
    want_c = np.zeros(DIMS + (4,), np.float32)
    for d, s in src_of.items():
        want_c[d] = cells[s]
    assert np.array_equal(out["cells"].view(np.uint32), want_c.view(np.uint32))
    if keep is None:
        assert hits.any() and (np.array(claimed) > 0).sum() >= 3    # (the case does collide)


def test_densest_on_equal_and_nan_sigma():
    """Two copies land on one cell that keeps its own content: three candidates, every order of (number, equal, NaN)."""
    for sig, winner in (((1.0, 2.0, 3.0), 2), ((3.0, 3.0, 3.0), 0), ((1.0, 3.0, 3.0), 1), ((NAN, NAN, NAN), 0), ((NAN, NAN, 2.0), 2),
                        ((NAN, 1.0, 2.0), 2), ((2.0, NAN, 2.0), 0), ((1.0, NAN, 0.5), 0), ((-1.0, NAN, -0.5), 2), ((NAN, -2.0, NAN), 1)):
        labels = np.full(DIMS, 255, dtype=np.uint8)
        cells = np.zeros(DIMS + (4,), dtype=np.float32)
        labels[8, 8, 8], labels[2, 8, 8], labels[12, 8, 8] = 0, 1, 2
        for n, at in enumerate(((8, 8, 8), (2, 8, 8), (12, 8, 8))):
            cells[at] = (n + 1.0, 0.0, 0.0, sig[n])
        entries = [(V.COPY, 1, V.translation([-6.0, 0.0, 0.0])), (V.COPY, 2, V.translation([4.0, 0.0, 0.0]))]
        out = run(labels, entries, cells, rule=1)
        assert out["source"][8, 8, 8] == winner and out["labels"][8, 8, 8] == winner and out["cells"][8, 8, 8, 0] == winner + 1.0, sig
        assert run(labels, entries, cells, rule=0)["source"][8, 8, 8] == 0
        assert out["hits"].tolist() == [[1, 0, 1] + [0] * (C - 3), [1, 1, 0] + [0] * (C - 3)]


def test_bad_numbers_give_no_candidate_and_no_exception():
    labels, cells = V.random_volume(DIMS, C, seed=4, baked=True)
    plain = run(labels, [(V.REMOVE, 3, None)], cells)
    bad = np.eye(4)
    bad[0, 0], bad[1, 3], bad[2, 2] = NAN, np.inf, -np.inf
    far = V.translation([1e30, -1e38, 3e9])
    huge = np.eye(4) * 3e38
    for m in (bad, far, huge, np.full((4, 4), NAN), np.full((4, 4), np.inf)):
        for rule in (0, 1):
            out = run(labels, [(V.MOVE, 3, m)], cells, rule=rule)
            assert out["claimed"].tolist() == [0] and not out["hits"].any()
            assert np.array_equal(out["labels"], plain["labels"])
            ref = run(labels, [(V.MOVE, 3, m)], cells, rule=rule, referee=True)
            assert np.array_equal(ref["labels"], out["labels"])


def test_a_generic_rotation_differs_from_the_referee_only_at_cell_faces():
    """0.3 rad about an oblique axis through a centre that is no cell corner, on a dense random volume (so that a wrong source cell
    shows as a wrong label almost always).  Cap: 0.5 % of the cells; every differing cell's float64 source point lies within 1e-4 cells
    of a face.  (f32 places a point of this box to about 16 x 2^-24 = 1e-6 cells, so 1e-4 is generous and 0.5 % far above the
    ~ 3 x 2 x 1e-6 of the cells one expects within reach of a face: this rotation gives 0 differing cells.)"""
    labels, cells = V.random_volume(DIMS, C, seed=5, empty=0.1, baked=True)
    m = editing.about(V.rotation([0.3, -0.5, 0.8], 0.3), [0.37, -1.21, 0.55])
    differ = np.zeros(labels.size, bool)
    for label in (0, 3, 9):
        got = run(labels, [(V.MOVE, label, m)], cells)
        want = run(labels, [(V.MOVE, label, m)], cells, referee=True)
        assert want["claimed"][0] > 20
        d = (got["labels"] != want["labels"]).reshape(-1) | (got["source"] != want["source"]).reshape(-1)
        assert (want["face"][d] <= 1e-4).all()
        differ |= d
    print("differing cells:", int(differ.sum()), "of", labels.size)
    assert differ.sum() <= 0.005 * labels.size


# ---- editing.edit_volume: what is refused before anything touches a device (the volume here is never read)
def _fake_grid(baked):
    from dm_nerf_amd import field
    g = object.__new__(field.BakedGrid if baked else field.LabelGrid)
    g.C, g.dims = C, DIMS
    g.lo, g.hi = np.asarray(LO, np.float32), np.asarray(HI, np.float32)
    g.cell, g.inv_cell = CONSTS[1], CONSTS[2]
    g.labels = g.cells = None                                      # anything that touched them would raise AttributeError / TypeError
    return g


@pytest.mark.parametrize("baked", [False, True])
def test_edit_volume_refuses_before_the_device(monkeypatch, baked):
    calls = []
    monkeypatch.setattr(_lib, "launch", lambda *a: calls.append(a))
    g = _fake_grid(baked)
    eye = np.eye(4)
    with pytest.raises(ValueError, match="image row"):
        edit_volume(g, [editing.Deform("sin")], [1])
    with pytest.raises(ValueError, match="image row"):
        edit_volume(g, [eye, editing.Copy(editing.Deform("ex"))], [1, 2])
    with pytest.raises(ValueError, match="at most 32"):
        edit_volume(g, [eye] * 33, [1] * 33)
    for bad in (-1, C, 255):
        with pytest.raises(ValueError, match="outside"):
            edit_volume(g, [eye], [bad])
        with pytest.raises(ValueError, match="outside"):
            edit_volume(g, [editing.Remove()], [1], keep_labels=[0, bad])
    with pytest.raises(ValueError, match="target labels for"):
        edit_volume(g, [eye, eye], [1])
    with pytest.raises(ValueError, match="rule"):
        edit_volume(g, [eye], [1], rule="nearest")
    with pytest.raises(ValueError, match="4 x 4"):
        edit_volume(g, [np.eye(3)], [1])
    if not baked:
        with pytest.raises(ValueError, match="densest"):
            edit_volume(g, [eye], [1], rule="densest")
    with pytest.raises(ValueError, match="out"):
        edit_volume(g, [eye], [1], out=g)
    assert not calls


def test_the_entry_refuses_bad_arguments_before_any_launch():
    """Host-side checks of ``dmnerf_volume_edit``: every call returns DMNERF_E_ARG before a launch (the addresses are never read)."""
    import ctypes
    lib = _lib.load()
    assert lib.dmnerf_volume_edit.argtypes == ENTRY[1] and len(ENTRY[1]) == 18
    f3 = lambda v: (ctypes.c_float * 3)(*v)
    keep = (ctypes.c_uint32 * 4)(*ALL)
    ent = (_lib.VolumeEditEntry * 2)()
    ent[0].kind, ent[0].label, ent[1].kind, ent[1].label = 0, 3, 2, 5
    p = lambda n: ctypes.c_void_p(0x10000 + 0x100000 * n)           # distinct, 16-byte aligned, far apart

    def call(dims=DIMS, Cn=C, E=2, rule=0, labels=p(1), cells=None, out_labels=p(3), out_cells=None, source=p(5), won=p(6), claimed=p(7),
             hits=p(8), entries=ent):
        return lib.dmnerf_volume_edit(labels, cells, f3(CONSTS[0]), f3(CONSTS[1]), f3(CONSTS[2]), (ctypes.c_int * 3)(*dims), Cn, keep, entries, E,
                                      rule, out_labels, out_cells, source, won, claimed, hits, None)

    for kw, word in ((dict(dims=(0, 4, 4)), "dims"), (dict(dims=(2048, 2048, 512)), "int32"), (dict(Cn=0), "C="), (dict(Cn=129), "C="),
                     (dict(E=33), "E="), (dict(E=-1), "E="), (dict(entries=None), "null entries"), (dict(rule=2), "rule"),
                     (dict(rule=1), "needs d_cells"), (dict(labels=None), "null"), (dict(hits=None), "null"), (dict(claimed=None), "null"),
                     (dict(cells=p(2)), "go together"), (dict(out_cells=p(4)), "go together"),
                     (dict(cells=ctypes.c_void_p(0x200008), out_cells=p(4)), "aligned"), (dict(out_labels=p(1)), "overlaps"), (dict(source=p(3)), "overlaps"), (dict(won=p(3)), "overlaps"), (dict(hits=p(6)), "overlaps"),
                     (dict(claimed=p(5)), "overlaps"),
                     (dict(source=ctypes.c_void_p(0x10000 + 0x100000 + 4095)), "overlaps"), (dict(cells=p(2), out_cells=ctypes.c_void_p(0x210000 + 65520)), "overlaps")):
        assert call(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    ent[1].kind = 3
    assert call() == -1 and "kind" in _lib.last_error()
    ent[1].kind, ent[1].label = 2, C
    assert call() == -1 and "label" in _lib.last_error()
