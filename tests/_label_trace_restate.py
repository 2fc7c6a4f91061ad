"""csrc/label_trace.hip in numpy float32, statement for statement, and a float64 referee written differently on purpose.

``trace_sets`` is the kernel: every f32 operation is one numpy operation on float32 arrays (one rounding each), minimum and maximum
are the kernel's comparisons (``nan_min`` / ``nan_max`` hand a NaN on), the walk is the kernel's counted loop with the rays that are
still walking as a mask.  ``referee`` sorts plane crossings in float64 and looks at interval midpoints: no stepping at all.
"""
import numpy as np

import _grid_restate as G
from _grid_restate import _in_mask, mask_words

f32 = np.float32
UNLABELLED = 255
INF = f32(np.inf)


def grid_consts(lo, hi, dims):
    """``_grid_restate.grid_consts`` and ``dims`` as a tuple of ints: the four things a trace case carries around."""
    dims = tuple(int(d) for d in dims)
    return (*G.grid_consts(lo, hi, dims), dims)


def nan_min(x, y):
    return np.where((x < y) | (x != x), x, y)


def nan_max(x, y):
    return np.where((x > y) | (x != x), x, y)


def plane_of(lo_a, cell_a, b):
    return (lo_a + (b.astype(f32) * cell_a).astype(f32)).astype(f32)


def trace_one(labels, lo, cell, inv_cell, C, o, d, words, t_near, t_far):
    """One ray set: ``o, d [N, 3]`` float32 -> ``hit [N] bool, label [N], t [N] f32, cell [N]`` (the kernel's body of the set loop)."""
    labels = np.asarray(labels, dtype=np.uint8)
    dims = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    o, d = np.asarray(o, dtype=f32), np.asarray(d, dtype=f32)
    N = o.shape[0]
    with np.errstate(all="ignore"):
        t_enter = np.full(N, t_near, dtype=f32)
        t_exit = np.full(N, t_far, dtype=f32)
        miss = np.zeros(N, dtype=bool)
        inv = []
        hi = [plane_of(lo[a], cell[a], np.array(dims[a])) for a in range(3)]
        for a in range(3):
            zero = d[:, a] == 0
            miss |= zero & ~((lo[a] <= o[:, a]) & (o[:, a] < hi[a]))
            inv_a = (f32(1.0) / d[:, a]).astype(f32)
            t0 = ((lo[a] - o[:, a]).astype(f32) * inv_a).astype(f32)
            t1 = ((hi[a] - o[:, a]).astype(f32) * inv_a).astype(f32)
            t_enter = np.where(zero, t_enter, nan_max(t_enter, nan_min(t0, t1))).astype(f32)
            t_exit = np.where(zero, t_exit, nan_min(t_exit, nan_max(t0, t1))).astype(f32)
            inv.append(inv_a)
        walking = ~miss & (t_enter < t_exit)
        c, up = [], []
        for a in range(3):
            p = (o[:, a] + (d[:, a] * t_enter).astype(f32)).astype(f32)
            f = np.floor(((p - lo[a]).astype(f32) * inv_cell[a]).astype(f32))
            ca = np.where(f >= 0, np.where(f < f32(dims[a]), f, f32(dims[a] - 1)), f32(0))          # (a NaN: 0)
            c.append(np.where(walking, ca, 0).astype(np.int64))
            up.append((d[:, a] > 0).astype(np.int64))
        t = t_enter.copy()
        hit = np.zeros(N, dtype=bool)
        out_l = np.full(N, UNLABELLED, dtype=np.int64)
        out_t = np.full(N, INF, dtype=f32)
        out_c = np.full(N, -1, dtype=np.int64)
        for _ in range(dims[0] + dims[1] + dims[2] + 1):
            if not walking.any():
                break
            g = (c[0] * dims[1] + c[1]) * dims[2] + c[2]
            assert (g[walking] >= 0).all() and (g[walking] < flat.shape[0]).all()       # what keeps the kernel's load in bounds
            l = flat[np.where(walking, g, 0)]
            accept = walking & (l < C) & _in_mask(l, words)
            hit |= accept
            out_l[accept], out_t[accept], out_c[accept] = l[accept], t[accept], g[accept]
            walking = walking & ~accept
            tm = [np.where(d[:, a] == 0, INF, ((plane_of(lo[a], cell[a], c[a] + up[a]) - o[:, a]).astype(f32) * inv[a]).astype(f32))
                  for a in range(3)]
            axis = np.zeros(N, dtype=np.int64)
            best = tm[0]
            s = tm[1] < best
            axis, best = np.where(s, 1, axis), np.where(s, tm[1], best)
            s = tm[2] < best
            axis, best = np.where(s, 2, axis), np.where(s, tm[2], best)
            walking = walking & (best < t_exit)
            t = np.where(walking, np.where(best > t, best, t), t).astype(f32)
            for a in range(3):
                c[a] = np.where(walking & (axis == a), c[a] + np.where(up[a] == 1, 1, -1), c[a])
            inside = np.ones(N, dtype=bool)
            for a in range(3):
                inside &= (c[a] >= 0) & (c[a] < dims[a])
            walking = walking & inside
    return hit, out_l, out_t, out_c


def trace_sets(labels, lo, cell, inv_cell, C, rays, masks, t_near, t_far):
    """The kernel: ``rays [R, 2, N, 3]``, ``masks`` R lists of four words -> ``label [N] uint8, t [N] f32, cell [N] int32, source [N]
    uint8``; the smallest t over the sets, the lowest set on equal t; (255, inf, -1, 255) where every set misses."""
    rays = np.asarray(rays, dtype=f32)
    R, _, N, _ = rays.shape
    assert len(masks) == R
    label = np.full(N, UNLABELLED, dtype=np.uint8)
    t = np.full(N, INF, dtype=f32)
    cell_out = np.full(N, -1, dtype=np.int32)
    source = np.full(N, UNLABELLED, dtype=np.uint8)
    for r in range(R):
        hit, l, tr, g = trace_one(labels, lo, cell, inv_cell, C, rays[r, 0], rays[r, 1], masks[r], f32(t_near), f32(t_far))
        better = hit & (tr < t)
        label[better], t[better], cell_out[better], source[better] = l[better], tr[better], g[better], r
    return label, t, cell_out, source


def trace(labels, lo, cell, inv_cell, C, o, d, words, t_near, t_far):
    """``R = 1``: the plain trace -> ``label, t, cell``."""
    return trace_sets(labels, lo, cell, inv_cell, C, np.stack([o, d])[None], [words], t_near, t_far)[:3]


# ---- the float64 referee: crossings sorted, midpoints looked up
def referee_walk(dims, lo, cell, o, d, t_near, t_far):
    """The cells one ray visits, in float64 -> a list of ``(t_start, flat cell index)``, empty if the ray misses the box.  The planes are
    the kernel's f32 values taken to float64 (the box is the same box); everything behind them is float64: the box interval by slabs,
    all plane crossings inside it, sorted, and the cell of every interval's midpoint found by counting the planes below it."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    planes = [plane_of(lo[a], cell[a], np.arange(dims[a] + 1)).astype(np.float64) for a in range(3)]
    a0, a1 = float(t_near), float(t_far)
    for a in range(3):
        if d[a] == 0:
            if not planes[a][0] <= o[a] < planes[a][-1]:
                return []
            continue
        ta, tb = sorted(((planes[a][0] - o[a]) / d[a], (planes[a][-1] - o[a]) / d[a]))
        a0, a1 = max(a0, ta), min(a1, tb)
    if not a0 < a1:
        return []
    cuts = [a0, a1]
    for a in range(3):
        if d[a] != 0:
            tc = (planes[a][1:-1] - o[a]) / d[a]
            cuts.extend(tc[(tc > a0) & (tc < a1)].tolist())
    cuts = sorted(cuts)
    walk = []
    for s, e in zip(cuts[:-1], cuts[1:]):
        if e == s:
            continue
        p = o + d * (0.5 * (s + e))
        idx = [int(np.searchsorted(planes[a], p[a], side="right")) - 1 for a in range(3)]
        if all(0 <= i < dims[a] for a, i in enumerate(idx)):
            walk.append((s, (idx[0] * dims[1] + idx[1]) * dims[2] + idx[2]))
    return walk


def referee(labels, walks, C, accepted):
    """The first accepted cell of every walk -> ``label [N] uint8, t [N] float64, cell [N] int32``; (255, inf, -1) on a miss."""
    flat = np.asarray(labels).reshape(-1)
    accepted = set(int(l) for l in accepted)
    N = len(walks)
    label, t, cell = np.full(N, UNLABELLED, np.uint8), np.full(N, np.inf), np.full(N, -1, np.int32)
    for n, walk in enumerate(walks):
        for s, g in walk:
            l = int(flat[g])
            if l < C and l in accepted:
                label[n], t[n], cell[n] = l, s, g
                break
    return label, t, cell


# ---- the inputs both test files use
LO, HI = (-1.5, -1.2, -1.0), (1.5, 1.3, 2.0)
GRIDS = ((5, 6, 7), (8, 8, 33))
C_TEST = 14
NAN = float("nan")


def random_volume(dims, seed, C=C_TEST, empty=0.4):
    """Random labels ``0 .. C + 1`` (two of them >= C: never accepted) with ``empty`` of the cells unlabelled (255)."""
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, C + 2, size=dims).astype(np.uint8)
    labels[rng.rand(*dims) < empty] = UNLABELLED
    return labels


def random_rays(n, seed, lo=LO, hi=HI):
    """``o, d [n, 3]`` float32: the first half starts on a sphere round the box and aims at a point inside it (unnormalised directions
    of length 0.5 .. 2), the second half starts inside the box and goes anywhere."""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    k = n // 2
    u = rng.randn(k, 3)
    o_out = centre + 4.0 * u / np.linalg.norm(u, axis=1, keepdims=True)
    aim = centre + (rng.rand(k, 3) * 2 - 1) * half
    d_out = aim - o_out
    d_out *= (rng.uniform(0.5, 2.0, size=(k, 1)) / np.linalg.norm(d_out, axis=1, keepdims=True))
    o_in = centre + (rng.rand(n - k, 3) * 2 - 1) * half * 0.999
    d_in = rng.randn(n - k, 3)
    d_in *= (rng.uniform(0.5, 2.0, size=(n - k, 1)) / np.linalg.norm(d_in, axis=1, keepdims=True))
    return np.concatenate([o_out, o_in]).astype(f32), np.concatenate([d_out, d_in]).astype(f32)


def crafted_rays(lo, cell, dims):
    """Named rays at the kernel's edges -> ``(names, o [n, 3], d [n, 3])`` float32: the guarded inputs (NaN origin, zero direction,
    infinite direction, NaN direction, denormal direction), one zero component inside and outside that slab, a start inside the box,
    a ray that misses the box, one that points away from it, one along a cell edge and one through a corner of the box."""
    lo64, cell64 = lo.astype(np.float64), cell.astype(np.float64)
    hi64 = lo64 + cell64 * np.asarray(dims)
    mid = (lo64 + hi64) / 2
    inside = lo64 + cell64 * (np.asarray(dims) // 2 + 0.25)
    rows = [
        ("nan_origin", (NAN, mid[1], mid[2]), (1, 0.2, 0.1)),
        ("zero_direction", inside, (0, 0, 0)),
        ("zero_direction_outside", lo64 - 1, (0, 0, 0)),
        ("inf_direction", lo64 - 1, (np.inf, 1, 1)),
        ("nan_direction", lo64 - 1, (1, NAN, 1)),
        ("denormal_direction", (lo64[0] - 1, mid[1], mid[2]), (1, 1e-42, 0)),
        ("inf_origin", (np.inf, mid[1], mid[2]), (-1, 0, 0)),
        ("zero_x_inside", (inside[0], lo64[1] - 1, inside[2]), (0, 1, 0.01)),
        ("zero_x_outside", (hi64[0] + 0.5, lo64[1] - 1, inside[2]), (0, 1, 0.01)),
        ("zero_x_on_upper_face", (hi64[0], lo64[1] - 1, inside[2]), (0, 1, 0.01)),
        ("zero_x_on_lower_face", (lo64[0], lo64[1] - 1, inside[2]), (0, 1, 0.01)),
        ("start_inside", inside, (0.3, -0.5, 0.8)),
        ("start_inside_negative", inside, (-1, -1, -1)),
        ("misses_box", (lo64[0] - 1, hi64[1] + 1, mid[2]), (1, 0.01, 0)),
        ("points_away", lo64 - 1, (-1, -1, -1)),
        ("along_cell_edge", (lo64[0] - 1, lo64[1] + cell64[1], lo64[2] + cell64[2]), (1, 0, 0)),
        ("through_corner", lo64 - 1, (1, 1, 1)),
        ("diagonal_back", hi64 + 1, (-1, -1, -1)),
        ("minus_zero_component", (inside[0], inside[1], lo64[2] - 1), (-0.0, 0.0, 2)),
    ]
    names = [r[0] for r in rows]
    return names, np.array([r[1] for r in rows], dtype=f32), np.array([r[2] for r in rows], dtype=f32)


def column_rays(lo, cell, dims):
    """``field.label_rays`` without its depths, in numpy: one ray per (i, j) column, o = the centre of cell (i, j, 0) as
    ``cell_centres`` computes it, d = (0, 0, cell_z)."""
    ax = [((np.arange(n, dtype=f32) + f32(0.5)) * cell[a] + lo[a]).astype(f32) for a, n in enumerate((dims[0], dims[1], 1))]
    o = np.stack([np.repeat(ax[0], dims[1]), np.tile(ax[1], dims[0]), np.full(dims[0] * dims[1], ax[2][0], f32)], -1).astype(f32)
    d = np.zeros_like(o)
    d[:, 2] = cell[2]
    return o, d
