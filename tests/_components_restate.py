"""The connected components of a label volume (csrc/components.hip, field.LabelGrid.components / cleaned, field.Components) in plain numpy.

The contract is canonical: ``labels`` uint8 ``[dx, dy, dz]``, cell ``g = (i dy + j) dz + k``; a cell is labelled iff ``labels[g] < C``; two
labelled cells are adjacent iff they carry the same label and differ by exactly one in one axis (connectivity 6) or by at most one in
every axis without being the same cell (26), no wrap-around; components are the classes of adjacency; ``root`` is the smallest index of
the cell's component (-1 unlabelled), ``size`` its number of cells (0).  Here: a sequential union-find over the pairs (cell,
predecessor), the smaller root always the parent."""
import numpy as np

UNLABELLED = 255


def predecessors(connectivity):
    """The offsets to the adjacent cells with a smaller index: 3 at connectivity 6, 13 at 26."""
    if connectivity not in (6, 26):
        raise ValueError(connectivity)
    offs = [(di, dj, dk) for di in (-1, 0, 1) for dj in (-1, 0, 1) for dk in (-1, 0, 1) if (di, dj, dk) < (0, 0, 0)]
    return [o for o in offs if connectivity == 26 or sum(map(abs, o)) == 1]


def components(labels, C, connectivity):
    """-> ``(root, size)`` int32 ``[dx, dy, dz]``."""
    labels = np.asarray(labels)
    dx, dy, dz = labels.shape
    n = labels.size
    lab = np.where(labels < C, labels, UNLABELLED).astype(np.int64)
    index = np.arange(n, dtype=np.int64).reshape(labels.shape)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for di, dj, dk in predecessors(connectivity):
        # cells [a0, a1) per axis whose neighbour at the offset exists
        here = tuple(slice(max(0, -o), d - max(0, o)) for o, d in zip((di, dj, dk), (dx, dy, dz)))
        there = tuple(slice(max(0, o), d - max(0, -o)) for o, d in zip((di, dj, dk), (dx, dy, dz)))
        same = (lab[here] == lab[there]) & (lab[here] != UNLABELLED)
        for g, h in zip(index[here][same].tolist(), index[there][same].tolist()):
            a, b = find(g), find(h)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.array([find(g) for g in range(n)], dtype=np.int64)
    root[lab.reshape(-1) == UNLABELLED] = -1
    counts = np.bincount(root[root >= 0], minlength=n)
    size = np.where(root >= 0, counts[np.maximum(root, 0)], 0)
    return root.astype(np.int32).reshape(labels.shape), size.astype(np.int32).reshape(labels.shape)


def largest(labels, C, root, size):
    """-> ``(root [C], size [C])`` int32 of every label's largest component, the smallest root on equal sizes; -1 / 0 without a cell."""
    best_root, best_size = np.full(C, -1, np.int32), np.zeros(C, np.int32)
    flat, r, s = np.asarray(labels).reshape(-1), root.reshape(-1), size.reshape(-1)
    for g in np.nonzero(r == np.arange(r.size))[0]:                  # ascending roots: a later one must be strictly larger
        if s[g] > best_size[flat[g]]:
            best_root[flat[g]], best_size[flat[g]] = g, s[g]
    return best_root, best_size


def cleaned(labels, C, connectivity=6, min_cells=1, keep="all", which=None, cells=None):
    """-> ``(labels, cells or None, removed [C], kept [C])``: ``which`` = the labels the filter looks at (default: all ``< C``)."""
    labels = np.asarray(labels)
    root, size = components(labels, C, connectivity)
    best_root, _ = largest(labels, C, root, size)
    looked = np.zeros(256, bool)
    looked[list(range(C) if which is None else [which] if isinstance(which, int) else which)] = True
    counted = labels < C
    ok = size >= min_cells
    if keep == "largest":
        ok &= root == best_root[np.where(counted, labels, 0)]
    elif keep != "all":
        raise ValueError(keep)
    drop = counted & looked[labels] & ~ok
    out = np.where(drop, UNLABELLED, labels).astype(np.uint8)
    out_cells = None
    if cells is not None:
        out_cells = cells.copy()
        out_cells[drop] = 0.0
    removed = np.bincount(labels[drop], minlength=C)[:C].astype(np.int64)
    kept = np.bincount(labels[counted & ~drop], minlength=C)[:C].astype(np.int64)
    return out, out_cells, removed, kept


def table(labels, C, root, size, lo, cell):
    """``Components.table()``: one row per component in ascending root; the float64 columns with ``LabelGrid.stats()``'s definitions."""
    labels = np.asarray(labels)
    r = root.reshape(-1)
    roots = np.nonzero(r == np.arange(r.size))[0]
    K = roots.size
    rank = np.full(r.size, -1, np.int64)
    rank[roots] = np.arange(K)
    cell_id = np.where(r >= 0, rank[np.maximum(r, 0)], -1).astype(np.int32).reshape(labels.shape)
    ijk = np.stack(np.unravel_index(np.arange(r.size), labels.shape), axis=-1).astype(np.int64)
    index_sum = np.zeros((K, 3), np.int64)
    lo_idx = np.zeros((K, 3), np.int32)
    hi_idx = np.zeros((K, 3), np.int32)
    for q in range(K):
        mine = ijk[cell_id.reshape(-1) == q]
        index_sum[q], lo_idx[q], hi_idx[q] = mine.sum(0), mine.min(0), mine.max(0) + 1
    count = size.reshape(-1)[roots].astype(np.int64)
    lo, cell = np.asarray(lo, np.float32).astype(np.float64), np.asarray(cell, np.float32).astype(np.float64)
    n = count.astype(np.float64)
    return {"id": cell_id, "label": labels.reshape(-1)[roots].astype(np.uint8), "root": roots.astype(np.int32), "count": count,
            "index_sum": index_sum, "lo_idx": lo_idx, "hi_idx": hi_idx,
            "centre": (index_sum.astype(np.float64) / n[:, None] + 0.5) * cell + lo,
            "box_lo": lo_idx.astype(np.float64) * cell + lo, "box_hi": hi_idx.astype(np.float64) * cell + lo,
            "volume": n * float(cell[0] * cell[1] * cell[2])}


def pack_bits(cells):
    """A bool array -> the uint32 words of a SkipGrid: cell g is bit g & 31 of word g >> 5."""
    words = np.packbits(np.asarray(cells).reshape(-1), bitorder="little")
    return np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)


def anchor_volume():
    """The volume of the issue's anchor: 921 components at connectivity 6 and 57 at 26, summed over its three labels."""
    rng = np.random.RandomState(0)
    v = rng.randint(0, 3, size=(9, 10, 37)).astype(np.uint8)
    v[rng.rand(9, 10, 37) >= 0.6] = UNLABELLED
    return v


def serpentine(dims):
    """One 6-connected chain of label 0 through the whole volume, separated from itself by unlabelled cells: every second row of every
    second plane, neighbouring rows joined at alternating ends, neighbouring planes joined where the plane's walk ends."""
    dx, dy, dz = dims
    v = np.full(dims, UNLABELLED, np.uint8)
    rows, at = list(range(0, dy, 2)), 0
    for p, i in enumerate(range(0, dx, 2)):
        order = rows if p % 2 == 0 else rows[::-1]
        for q, j in enumerate(order):
            v[i, j, :] = 0
            at = dz - 1 - at                                         # the walk is now at the row's other end
            if q + 1 < len(order):
                v[i, (j + order[q + 1]) // 2, at] = 0
        if i + 2 < dx:
            v[i + 1, order[-1], at] = 0
    return v
