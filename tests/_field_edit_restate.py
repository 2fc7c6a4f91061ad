"""csrc/field_edit.hip in numpy: ``select`` and ``filter_rows`` state the two kernels bit for bit (float32, one numpy operation per f32
operation of the kernel, in its order); ``owner_referee`` finds every sample's cell in float64 and reports how close the point lies to
a cell face; ``brute_*`` are plain Python loops over the samples for the integer work (the selection, its length, the kept counts).

An entry is ``(kind, label, m)`` as in tests/_volume_edit_restate.py: kind 0 MOVE / 1 COPY / 2 REMOVE, ``m`` anything whose first three
rows are the 3 x 4 map (ignored for REMOVE).  Policies: 0 EVALUATE (owner 0), 1 EMPTY (owner 255).
"""
import numpy as np

import _volume_edit_restate as V
from _grid_restate import cells_f32

f32 = np.float32
NOBODY = 255
MOVE, COPY, REMOVE = V.MOVE, V.COPY, V.REMOVE
EVALUATE, EMPTY = 0, 1


def empty_row(C):
    """``(0, 0, 0, 0 | 0, .., 0, 1)``: ``render.empty_row``."""
    row = np.zeros(4 + C, dtype=f32)
    row[-1] = 1.0
    return row


def accept_masks(C, entries, keep=None):
    """The ``(1 + E) x 4`` words of ``editing.FieldEdit``: owner 0 accepts ``keep`` without the labels of MOVE and REMOVE entries, owner
    ``1 + e`` accepts ``{label_e} & keep`` (a REMOVE entry owns nothing: no label)."""
    keep = set(range(C)) if keep is None else {int(l) for l in keep}
    gone = {int(l) for k, l, _ in entries if k != COPY}
    rows = [V.mask_words(sorted(keep - gone), C)]
    for k, l, _ in entries:
        rows.append(V.mask_words([int(l)] if (k != REMOVE and int(l) in keep) else [], C))
    return np.asarray(rows, dtype=np.uint32).reshape(1 + len(entries), 4)


def owners(source, inside, g, entries, outside, unowned):
    """The owner byte of every sample from its cell: the kernel's sequence."""
    E = len(entries)
    b = np.asarray(source, dtype=np.uint8).reshape(-1)[g].astype(np.int64)
    evaluable = np.zeros(256, dtype=bool)
    evaluable[0] = True
    for e, (k, _, _) in enumerate(entries):
        evaluable[1 + e] = k != REMOVE
    b = np.where((b > E) | ~evaluable[b], NOBODY, b)
    pol = lambda p: 0 if p == EVALUATE else NOBODY
    own = np.where(b == NOBODY, pol(unowned), b)
    return np.where(inside, own, pol(outside)).astype(np.uint8)


def select(source, lo, inv_cell, entries, rays_o, rays_d, z, outside=EVALUATE, unowned=EVALUATE, rows=None, fill_row=None):
    """``dmnerf_field_edit_select`` -> ``owner [M]`` uint8, ``o_w, d_w [M,3]`` f32 (rows of samples nobody evaluates: NaN, the kernel
    leaves them alone), ``sel`` int32 ascending, ``count``, and ``rows`` with ``fill_row`` in the rows of owner 255 (a copy)."""
    dims = np.asarray(source).shape
    o, d, z = np.asarray(rays_o, f32), np.asarray(rays_d, f32), np.asarray(z, f32)
    N, S = z.shape
    inside, g = cells_f32(o, d, z, lo, inv_cell, dims)
    own = owners(source, inside, g, entries, outside, unowned).reshape(-1)
    n_of = np.repeat(np.arange(N), S)
    om, dm = o[n_of], d[n_of]
    o_w, d_w = om.copy(), dm.copy()
    with np.errstate(all="ignore"):
        for e, (k, _, m) in enumerate(entries):
            if k == REMOVE:
                continue
            mine = own == 1 + e
            if not mine.any():
                continue
            q = V.matrix_f32(m)
            for a in range(3):
                t = ((q[a, 0] * om[:, 0]).astype(f32) + (q[a, 1] * om[:, 1]).astype(f32)).astype(f32)
                t = (t + (q[a, 2] * om[:, 2]).astype(f32)).astype(f32)
                o_w[:, a] = np.where(mine, (t + q[a, 3]).astype(f32), o_w[:, a])
                t = ((q[a, 0] * dm[:, 0]).astype(f32) + (q[a, 1] * dm[:, 1]).astype(f32)).astype(f32)
                d_w[:, a] = np.where(mine, (t + (q[a, 2] * dm[:, 2]).astype(f32)).astype(f32), d_w[:, a])
    ev = own != NOBODY
    o_w[~ev], d_w[~ev] = np.nan, np.nan
    out = {"owner": own, "o_w": o_w, "d_w": d_w, "sel": np.nonzero(ev)[0].astype(np.int32), "count": int(ev.sum())}
    if rows is not None:
        rows = np.array(rows, dtype=f32, copy=True).reshape(N * S, -1)
        rows[~ev] = np.asarray(fill_row, dtype=f32)
        out["rows"] = rows
    return out


def labels_of(raw):
    """``dmnerf_label_cells``' argmax without the sigma threshold: best = 0; channel c > 0 replaces it iff ``x[c] > x[best]``."""
    x = np.asarray(raw, f32)[:, 4:]
    best = np.zeros(x.shape[0], dtype=np.int64)
    bv = x[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for c in range(1, x.shape[1]):
            take = x[:, c] > bv
            bv = np.where(take, x[:, c], bv)
            best = np.where(take, c, best)
    return best


def filter_rows(raw, owner, masks, fill_row):
    """``dmnerf_field_edit_filter`` -> ``(raw [M, 4 + C] (a copy), kept [1 + E] int64)``."""
    raw = np.array(raw, dtype=f32, copy=True)
    owner = np.asarray(owner, dtype=np.int64)
    masks = np.asarray(masks, dtype=np.uint32).reshape(-1, 4)
    E = masks.shape[0] - 1
    label = labels_of(raw)
    active = owner <= E
    word = masks[np.where(active, owner, 0), label >> 5]
    ok = active & (((word >> (label & 31).astype(np.uint32)) & 1) != 0)
    raw[active & ~ok] = np.asarray(fill_row, dtype=f32)
    return raw, np.array([(ok & (owner == w)).sum() for w in range(1 + E)], dtype=np.int64)


# ---- the float64 referee of the owner
def owner_referee(source, lo, hi, entries, rays_o, rays_d, z, outside=EVALUATE, unowned=EVALUATE):
    """The owner from the cell of ``o + d z`` in float64 (the box is the kernel's f32 ``lo`` and ``cell`` taken to float64; the cell is
    found by a division, not by the rounded reciprocal) -> ``(owner [M] uint8, face [M])``: ``face`` is the distance of the point to
    the nearest cell face in cell units, the smallest over the axes (a NaN / inf point: 0.5)."""
    dims = np.asarray(source).shape
    lo32, cell32, _ = V.grid_consts(lo, hi, dims)
    lo64, cell64 = lo32.astype(np.float64), cell32.astype(np.float64)
    o, d, z = (np.asarray(t, f32).astype(np.float64) for t in (rays_o, rays_d, z))
    inside = np.ones(z.shape, dtype=bool)
    g = np.zeros(z.shape, dtype=np.int64)
    face = np.full(z.shape, 0.5)
    with np.errstate(all="ignore"):
        for a in range(3):
            u = (o[:, a:a + 1] + d[:, a:a + 1] * z - lo64[a]) / cell64[a]
            c = np.floor(u)
            inside &= (c >= 0) & (c < dims[a])
            g = g * dims[a] + np.where(inside, c, 0).astype(np.int64)
            dist = np.abs(u - np.round(u))
            face = np.where(np.isfinite(dist), np.minimum(face, dist), face)
    return owners(source, inside, np.where(inside, g, 0), entries, outside, unowned).reshape(-1), face.reshape(-1)


# ---- plain loops
def brute_sel(owner):
    sel = []
    for m, b in enumerate(owner):
        if int(b) != NOBODY:
            sel.append(m)
    return sel, len(sel)


def brute_kept(raw, owner, masks):
    masks = np.asarray(masks, dtype=np.uint32).reshape(-1, 4)
    kept = [0] * masks.shape[0]
    for m, b in enumerate(owner):
        b = int(b)
        if b >= masks.shape[0]:
            continue
        x = raw[m, 4:]
        best = 0
        for c in range(1, x.shape[0]):
            if x[c] > x[best]:
                best = c
        if (int(masks[b, best >> 5]) >> (best & 31)) & 1:
            kept[b] += 1
    return kept


# ---- inputs both test files use
BOX = ((-1.0, -0.8, -1.2), (1.1, 0.9, 1.3))                        # nothing dyadic: the f32 roundings matter


def random_source(dims, E, seed, unowned=0.3):
    """Bytes ``0 .. E`` with ``unowned`` of the cells 255, plus a byte ``E + 1`` (> E) and, where it fits, 254."""
    rng = np.random.RandomState(seed)
    src = rng.randint(0, E + 1, size=dims).astype(np.uint8)
    src[rng.rand(*dims) < unowned] = NOBODY
    src.reshape(-1)[:3] = (NOBODY, E + 1, 254)
    return src


def random_rays(N, S, seed, box=BOX, nan_rays=True):
    """Rays that start around the box and cross it, depths in ``[0, 2.5]`` ascending: most samples inside, some outside; with
    ``nan_rays`` ray 1 has a NaN origin and ray 2 an inf direction (where N allows)."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    o = (rng.uniform(lo - 0.4, hi + 0.4, size=(N, 3))).astype(f32)
    tgt = rng.uniform(lo, hi, size=(N, 3))
    d = tgt - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.3, size=(N, 1))).astype(f32)
    z = np.sort(rng.uniform(0.0, 2.5, size=(N, S)), axis=1).astype(f32)
    if nan_rays and N > 2:
        o[1, 0] = np.nan
        d[2, 1] = np.inf
    return o, d, z
