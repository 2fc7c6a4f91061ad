"""csrc/volume_edit.hip in numpy: ``edit`` states the kernel bit for bit (float32, one numpy operation per f32 operation of the kernel,
in its order), ``referee`` finds every destination cell's source point and source cell in float64 and applies the same candidate,
winner and count rules to them.  The two share ``_resolve`` -- everything behind the source cells is integer work and comparisons of
the volume's own sigmas -- so where they differ, they differ in a source cell, and ``referee`` reports how close each source point lies
to a cell face.

An entry is ``(kind, label, m)``: kind 0 MOVE / 1 COPY / 2 REMOVE (``networks.manipulator``), ``m`` anything whose first three rows
are the 3 x 4 map (ignored for REMOVE).  The matrix maps the centre of a DESTINATION cell to its source point.
"""
import numpy as np

from _grid_restate import _in_mask, grid_consts, mask_words

f32 = np.float32
UNLABELLED = 255
MOVE, COPY, REMOVE = 0, 1, 2


def matrix_f32(m):
    """Rows 0..2 of a matrix, rounded to float32 once: the twelve floats of an entry."""
    return np.asarray(m, dtype=np.float64).astype(f32)[:3, :4]


def _indices(dims):
    """``(i, j, k)`` int64 [n] of every cell in the kernel's order, k fastest."""
    i, j, k = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    return [i.reshape(-1), j.reshape(-1), k.reshape(-1)]


def source_cells_f32(dims, lo, cell, inv_cell, m):
    """The kernel's arithmetic -> ``(inside [n] bool, flat source index [n] int64 (0 where outside))``."""
    idx = _indices(dims)
    m = matrix_f32(m)
    with np.errstate(all="ignore"):
        p = [(((idx[a].astype(f32) + f32(0.5)).astype(f32) * cell[a]).astype(f32) + lo[a]).astype(f32) for a in range(3)]
        inside = np.ones(idx[0].shape[0], dtype=bool)
        c = []
        for a in range(3):
            t = ((m[a, 0] * p[0]).astype(f32) + (m[a, 1] * p[1]).astype(f32)).astype(f32)
            t = (t + (m[a, 2] * p[2]).astype(f32)).astype(f32)
            q = (t + m[a, 3]).astype(f32)
            f = np.floor(((q - lo[a]).astype(f32) * inv_cell[a]).astype(f32))
            ok = (f >= 0) & (f < dims[a])                        # (false for NaN; f is integral, dims exact: the kernel's integer test)
            inside &= ok
            c.append(np.where(ok, f, 0).astype(np.int64))
    return inside, np.where(inside, (c[0] * dims[1] + c[1]) * dims[2] + c[2], 0)


def source_cells_f64(dims, lo, cell, inv_cell, m):
    """The same map in float64 (the box and the matrix are the kernel's f32 values taken to float64; the cell is found by a division, not
    by the rounded reciprocal) -> ``(inside, flat source index, face [n])``: ``face`` is the distance of the source point to the
    nearest cell face in cell units, the smallest over the axes (NaN / inf points: 0.5)."""
    idx = _indices(dims)
    m = matrix_f32(m).astype(np.float64)
    lo, cell = np.asarray(lo, np.float64), np.asarray(cell, np.float64)
    with np.errstate(all="ignore"):
        p = [(idx[a] + 0.5) * cell[a] + lo[a] for a in range(3)]
        inside = np.ones(idx[0].shape[0], dtype=bool)
        face = np.full(idx[0].shape[0], 0.5)
        c = []
        for a in range(3):
            q = m[a, 0] * p[0] + m[a, 1] * p[1] + m[a, 2] * p[2] + m[a, 3]
            u = (q - lo[a]) / cell[a]
            f = np.floor(u)
            ok = (f >= 0) & (f < dims[a])
            inside &= ok
            c.append(np.where(ok, f, 0).astype(np.int64))
            dist = np.abs(u - np.round(u))
            face = np.where(np.isfinite(dist), np.minimum(face, dist), face)
    return inside, np.where(inside, (c[0] * dims[1] + c[1]) * dims[2] + c[2], 0), face


def _resolve(labels, cells, C, keep_words, entries, rule, sources):
    """Candidates, winner, outputs and counts from the source cells of the MOVE / COPY entries (``sources[e]`` = ``(inside, index)``,
    ``None`` for the others): the kernel's sequence, candidate by candidate in ascending number."""
    labels = np.asarray(labels, dtype=np.uint8)
    dims = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    n, E = flat.shape[0], len(entries)
    baked = cells is not None
    assert rule in (0, 1) and (baked or rule == 0) and E <= 32
    words = np.asarray(cells, dtype=f32).reshape(-1, 4).view(np.uint32) if baked else None
    sigma = words.view(f32)[:, 3] if baked else None
    gone = mask_words({int(l) for k, l, _ in entries if k != COPY}, C)
    cand = np.zeros((1 + E, n), dtype=bool)
    cand[0] = (flat < C) & _in_mask(flat, keep_words) & ~_in_mask(flat, gone)
    win = np.where(cand[0], 0, -1).astype(np.int64)
    win_label = np.where(cand[0], flat, UNLABELLED)
    win_src = np.arange(n)
    win_sigma = np.where(cand[0], sigma, f32(0)).astype(f32) if rule == 1 else None
    for e, (kind, label, _) in enumerate(entries):
        assert kind in (MOVE, COPY, REMOVE) and 0 <= label < C
        if kind == REMOVE or not bool(_in_mask(label, keep_words)):
            continue
        inside, src = sources[e]
        ok = inside & (flat[src] == label)
        cand[1 + e] = ok
        take = win < 0
        if rule == 1:
            with np.errstate(invalid="ignore"):
                s = sigma[src]
                take = take | (s > win_sigma) | ((win_sigma != win_sigma) & (s == s))
            win_sigma = np.where(ok & take, s, win_sigma)
        take = ok & take
        win = np.where(take, 1 + e, win)
        win_label = np.where(take, label, win_label)
        win_src = np.where(take, src, win_src)
    out = {"labels": win_label.astype(np.uint8).reshape(dims), "source": np.where(win < 0, UNLABELLED, win).astype(np.uint8).reshape(dims),
           "won": np.array([(win == w).sum() for w in range(1 + E)], dtype=np.int64), "claimed": cand[1:].sum(axis=1).astype(np.int64),
           "cand": cand, "win_src": win_src}
    if baked:
        out["cells"] = np.where((win >= 0)[:, None], words[win_src], np.uint32(0)).view(f32).reshape(dims + (4,))
    hits = np.zeros((E, C), dtype=np.int64)
    multi = cand.sum(axis=0) >= 2
    for e in range(E):
        in_e = multi & cand[1 + e]
        np.add.at(hits[e], flat[in_e & cand[0]], 1)
        for b in range(E):
            if b != e:
                hits[e, entries[b][1]] += int((in_e & cand[1 + b]).sum())
    out["hits"] = hits
    return out


def edit(labels, cells, lo, cell, inv_cell, C, keep_words, entries, rule=0):
    """The kernel -> ``labels`` uint8, ``cells`` f32 (baked only, bit for bit: NaN payloads survive), ``source`` uint8, ``won [1 + E]``,
    ``claimed [E]``, ``hits [E, C]`` int64 (and ``cand [1 + E, n]``, the candidates, for the tests' own counts)."""
    dims = np.asarray(labels).shape
    sources = [None if k == REMOVE else source_cells_f32(dims, lo, cell, inv_cell, m) for k, _, m in entries]
    return _resolve(labels, cells, C, keep_words, entries, rule, sources)


def referee(labels, cells, lo, cell, inv_cell, C, keep_words, entries, rule=0):
    """The same rules on float64 source cells; ``face [n]``: the smallest face distance of a cell's source points over the entries."""
    dims = np.asarray(labels).shape
    sources, face = [], np.full(int(np.prod(dims)), 0.5)
    for k, _, m in entries:
        if k == REMOVE:
            sources.append(None)
            continue
        inside, src, f = source_cells_f64(dims, lo, cell, inv_cell, m)
        sources.append((inside, src))
        face = np.minimum(face, f)
    out = _resolve(labels, cells, C, keep_words, entries, rule, sources)
    out["face"] = face
    return out


# ---- the inputs both test files use
def translation(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def rotation(axis, angle):
    """Rodrigues' matrix, 4 x 4 float64."""
    axis = np.asarray(axis, dtype=np.float64)
    x, y, z = axis / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return m


def random_volume(dims, C, seed, empty=0.4, baked=False):
    """Random labels ``0 .. C + 1`` (two values >= C where they fit a byte) with ``empty`` of the cells 255; ``baked``: also cells with
    colour logits N(0, 3) and densities with exact zeros, ties (a few repeated values), negatives and NaNs."""
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, min(C + 2, 255), size=dims).astype(np.uint8)
    labels[rng.rand(*dims) < empty] = UNLABELLED
    labels.reshape(-1)[:3] = (UNLABELLED, C, min(C + 1, 254))      # whatever the draw: a 255 and two values >= C
    if not baked:
        return labels, None
    cells = np.empty(tuple(dims) + (4,), dtype=f32)
    cells[..., :3] = rng.randn(*dims, 3) * 3.0
    sigma = rng.exponential(6.0, size=dims)
    pick = rng.rand(*dims)
    sigma[pick < 0.10] = 0.0
    sigma[(pick >= 0.10) & (pick < 0.25)] = 2.5                   # ties
    sigma[(pick >= 0.25) & (pick < 0.30)] = -3.0
    sigma[(pick >= 0.30) & (pick < 0.40)] = np.nan
    cells[..., 3] = sigma
    return labels, cells


def random_entries(E, C, seed, lo, hi):
    """E entries mixing MOVE / COPY / REMOVE over few labels (so that labels repeat): whole-cell and fractional shifts, small rotations
    about points of the box, a scale, and one matrix with NaN / inf entries."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    pool = sorted({0, 1 % C, C - 1, (C // 2)})
    out = []
    for e in range(E):
        kind = (MOVE, COPY, REMOVE, COPY, MOVE)[e % 5]
        label = int(pool[rng.randint(0, len(pool))]) if e != 2 else out[0][1]      # (entry 2 removes what entry 0 moves)
        how = e % 4
        if how == 0:
            m = translation(np.round(rng.uniform(-3, 3, 3)) * (hi - lo) / 16.0)
        elif how == 1:
            m = translation(rng.uniform(-0.2, 0.2, 3) * (hi - lo))
        elif how == 2:
            centre = rng.uniform(lo, hi)
            m = translation(centre) @ rotation(rng.randn(3), rng.uniform(-0.6, 0.6)) @ translation(-centre)
        else:
            m = np.diag([1.5, 0.75, 1.25, 1.0])
        if e == 7:
            m = m.copy()
            m[0, 0], m[1, 3], m[2, 2] = np.nan, np.inf, -np.inf
        out.append((kind, label, None if kind == REMOVE else m))
    return out


# ---- the 16^3 scene over [-8, 8)^3 (cell 1.0: every centre and every whole-cell map is dyadic)
SCENE_DIMS = (16, 16, 16)
SCENE_LO, SCENE_HI = (-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)


def scene(seed=3):
    """A few boxes well inside a 16^3 volume (labels 1, 3, 5, 7) -> labels, cells; the densities repeat, with NaNs."""
    rng = np.random.RandomState(seed)
    labels = np.full(SCENE_DIMS, 255, dtype=np.uint8)
    labels[2:5, 3:7, 4:6] = 1
    labels[6:9, 5:9, 6:10] = 3
    labels[10:13, 9:12, 3:8] = 5
    labels[4:6, 11:14, 10:13] = 7
    cells = np.zeros(SCENE_DIMS + (4,), dtype=np.float32)
    on = labels != 255
    cells[on, :3] = rng.randn(int(on.sum()), 3)
    cells[on, 3] = rng.choice([1.0, 2.5, 2.5, 6.0, np.nan], size=int(on.sum()))
    return labels, cells


def shift_entries(entries):
    """``brute``'s entries as the restatement's: the map of a whole-cell shift is a translation by ``shift`` cells (cell 1.0)."""
    return [(k, l, None if k == REMOVE else translation(np.asarray(s, np.float64))) for k, l, s in entries]


COLLISIONS = [
    # object 3 onto object 5 (it stays: candidate 0), object 1 onto the same cells, a copy of 7 onto 3's old place, a removal
    [(MOVE, 3, (-4, -4, 1)), (COPY, 1, (-8, -6, 0)), (COPY, 7, (-2, 6, 3)), (REMOVE, 1, None)],
    # the same label twice, to the same cells from two places; a move of 5 half out of the box
    [(COPY, 3, (-1, 0, 0)), (COPY, 3, (1, 0, 0)), (MOVE, 5, (-5, 0, 0)), (COPY, 5, (-3, -3, 0))],
]
