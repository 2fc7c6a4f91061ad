"""csrc/baked.hip in numpy float32, statement for statement in the walk and the merge, and a float64 referee of the compositing.

``segments`` is ``_label_trace_restate.trace_one``'s walker (the same clip, start cell and step, built from the same ``plane_of`` /
``nan_min`` / ``nan_max`` / ``_in_mask``) that does not stop at its first counted cell: it lists every counted cell of one ray set with
``t_in``, ``t_out``.  ``merge`` puts the lists of the R sets into the kernel's order: ascending ``t_in``, the lowest set first on equal
``t_in``, the walk's order within a set (a stable sort of the lists laid end to end in set order).  ``render`` composites that order in
float32, one numpy operation per f32 operation of the kernel; ``referee`` composites THE SAME segment list in float64.
"""
import numpy as np

import _label_trace_restate as T

f32 = np.float32
UNLABELLED = 255
INF = f32(np.inf)


def segments(labels, lo, cell, inv_cell, C, o, d, words, t_near, t_far):
    """One ray set -> ``(count [N], t_in [N, S], t_out [N, S], g [N, S], label [N, S])`` with ``S = dx + dy + dz + 1`` columns, the first
    ``count[n]`` of ray n filled in walk order."""
    labels = np.asarray(labels, dtype=np.uint8)
    dims = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    o, d = np.asarray(o, dtype=f32), np.asarray(d, dtype=f32)
    N = o.shape[0]
    S = dims[0] + dims[1] + dims[2] + 1
    count = np.zeros(N, dtype=np.int64)
    seg_in, seg_out = np.zeros((N, S), dtype=f32), np.zeros((N, S), dtype=f32)
    seg_g, seg_l = np.zeros((N, S), dtype=np.int64), np.full((N, S), UNLABELLED, dtype=np.int64)
    rows = np.arange(N)
    with np.errstate(all="ignore"):
        t_enter = np.full(N, t_near, dtype=f32)
        t_exit = np.full(N, t_far, dtype=f32)
        miss = np.zeros(N, dtype=bool)
        inv = []
        hi = [T.plane_of(lo[a], cell[a], np.array(dims[a])) for a in range(3)]
        for a in range(3):
            zero = d[:, a] == 0
            miss |= zero & ~((lo[a] <= o[:, a]) & (o[:, a] < hi[a]))
            inv_a = (f32(1.0) / d[:, a]).astype(f32)
            t0 = ((lo[a] - o[:, a]).astype(f32) * inv_a).astype(f32)
            t1 = ((hi[a] - o[:, a]).astype(f32) * inv_a).astype(f32)
            t_enter = np.where(zero, t_enter, T.nan_max(t_enter, T.nan_min(t0, t1))).astype(f32)
            t_exit = np.where(zero, t_exit, T.nan_min(t_exit, T.nan_max(t0, t1))).astype(f32)
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
        for _ in range(S):
            if not walking.any():
                break
            g = (c[0] * dims[1] + c[1]) * dims[2] + c[2]
            assert (g[walking] >= 0).all() and (g[walking] < flat.shape[0]).all()       # what keeps the kernel's loads in bounds
            l = flat[np.where(walking, g, 0)]
            counted = walking & (l < C) & T._in_mask(l, words)
            tm = [np.where(d[:, a] == 0, INF, ((T.plane_of(lo[a], cell[a], c[a] + up[a]) - o[:, a]).astype(f32) * inv[a]).astype(f32))
                  for a in range(3)]
            axis = np.zeros(N, dtype=np.int64)
            best = tm[0]
            s = tm[1] < best
            axis, best = np.where(s, 1, axis), np.where(s, tm[1], best)
            s = tm[2] < best
            axis, best = np.where(s, 2, axis), np.where(s, tm[2], best)
            on = best < t_exit
            k = count[counted]
            seg_in[rows[counted], k] = t[counted]
            seg_out[rows[counted], k] = np.where(on, best, t_exit)[counted]
            seg_g[rows[counted], k], seg_l[rows[counted], k] = g[counted], l[counted]
            count[counted] += 1
            walking = walking & on
            t = np.where(walking, np.where(best > t, best, t), t).astype(f32)
            for a in range(3):
                c[a] = np.where(walking & (axis == a), c[a] + np.where(up[a] == 1, 1, -1), c[a])
            inside = np.ones(N, dtype=bool)
            for a in range(3):
                inside &= (c[a] >= 0) & (c[a] < dims[a])
            walking = walking & inside
    return count, seg_in, seg_out, seg_g, seg_l


def norm_of(d):
    """``sqrtf(d0 d0 + d1 d1 + d2 d2)`` summed in that order, float32."""
    d = np.asarray(d, dtype=f32)
    with np.errstate(all="ignore"):
        sq = [(d[:, a] * d[:, a]).astype(f32) for a in range(3)]
        return np.sqrt(((sq[0] + sq[1]).astype(f32) + sq[2]).astype(f32)).astype(f32)


def merge(labels, lo, cell, inv_cell, C, rays, masks, t_near, t_far):
    """The segment list of every pixel in the kernel's order -> a dict of ``[N, R S]`` arrays ``t_in, t_out`` (f32), ``g, label, set``
    (int64), ``norm`` (f32, the set's ``|d|``) and ``count [N]``: the first ``count[n]`` columns are pixel n's segments."""
    rays = np.asarray(rays, dtype=f32)
    R, _, N, _ = rays.shape
    assert len(masks) == R
    cols = {k: [] for k in ("valid", "t_in", "t_out", "g", "label", "set", "norm")}
    for r in range(R):
        count, t_in, t_out, g, l = segments(labels, lo, cell, inv_cell, C, rays[r, 0], rays[r, 1], masks[r], f32(t_near), f32(t_far))
        S = t_in.shape[1]
        cols["valid"].append(np.arange(S)[None, :] < count[:, None])
        cols["t_in"].append(t_in)
        cols["t_out"].append(t_out)
        cols["g"].append(g)
        cols["label"].append(l)
        cols["set"].append(np.full((N, S), r, dtype=np.int64))
        cols["norm"].append(np.repeat(norm_of(rays[r, 1])[:, None], S, axis=1))
    cat = {k: np.concatenate(v, axis=1) for k, v in cols.items()}
    key = np.where(cat["valid"], cat["t_in"], INF)                # (a segment's t_in is below its t_exit: never +inf itself)
    assert not np.isnan(key).any()
    order = np.argsort(key, axis=1, kind="stable")                # ties: the column order = set order, then walk order
    out = {k: np.take_along_axis(v, order, axis=1) for k, v in cat.items()}
    out["count"] = cat["valid"].sum(axis=1)
    assert (out["valid"] == (np.arange(key.shape[1])[None, :] < out["count"][:, None])).all()
    return out


def _composite(seg, cells, stop, ft):
    """The kernel's compositing loop over ``merge``'s list in the float type ``ft``, one operation at a time."""
    cells = np.asarray(cells, dtype=f32).reshape(-1, 4).astype(ft)
    N, S = seg["t_in"].shape
    one, zero = ft(1.0), ft(0.0)
    T_ = np.ones(N, dtype=ft)
    rgb, depth, acc = np.zeros((N, 3), dtype=ft), np.zeros(N, dtype=ft), np.zeros(N, dtype=ft)
    best_w, second_w = np.zeros(N, dtype=ft), np.full(N, -np.inf, dtype=ft)
    label, source = np.full(N, UNLABELLED, dtype=np.uint8), np.full(N, UNLABELLED, dtype=np.uint8)
    nseg = np.zeros(N, dtype=np.int32)
    positive = np.zeros(N, dtype=bool)                             # a segment with sigma > 0: the weights are not all exactly 0
    top = np.full(N, -np.inf, dtype=ft)
    going = np.ones(N, dtype=bool)
    stop = ft(stop)
    with np.errstate(all="ignore"):
        for j in range(S):
            a = going & seg["valid"][:, j]
            if not a.any():
                break
            c = cells[seg["g"][:, j]]
            t_in, t_out = seg["t_in"][:, j].astype(ft), seg["t_out"][:, j].astype(ft)
            length = ((t_out - t_in).astype(ft) * seg["norm"][:, j].astype(ft)).astype(ft)
            sigma = np.where(c[:, 3] > 0, c[:, 3], zero).astype(ft)                 # (a NaN: 0)
            alpha = (one - np.exp(-(sigma * length).astype(ft)).astype(ft)).astype(ft)
            w = (T_ * alpha).astype(ft)
            T_ = np.where(a, (T_ * (one - alpha).astype(ft)).astype(ft), T_)
            for k in range(3):
                sig = (one / (one + np.exp(-c[:, k]).astype(ft)).astype(ft)).astype(ft)
                rgb[:, k] = np.where(a, (rgb[:, k] + (w * sig).astype(ft)).astype(ft), rgb[:, k])
            depth = np.where(a, (depth + (w * t_in).astype(ft)).astype(ft), depth)
            acc = np.where(a, (acc + w).astype(ft), acc)
            nseg[a] += 1
            positive |= a & (sigma > 0)
            second_w = np.where(a, np.where(w > top, top, np.where(w > second_w, w, second_w)), second_w)
            top = np.where(a & (w > top), w, top)
            better = a & (w > best_w)
            best_w = np.where(better, w, best_w)
            label[better], source[better] = seg["label"][better, j], seg["set"][better, j]
            going = going & ~(a & (T_ < stop))
    return {"rgb": rgb, "depth": depth, "acc": acc, "label": label, "source": source, "nseg": nseg, "w1": top, "w2": second_w,
            "positive": positive}


def render(labels, cells, lo, cell, inv_cell, C, rays, masks, t_near, t_far, stop=0.0, seg=None):
    """The kernel in float32 -> ``rgb [N, 3], depth, acc`` f32, ``label, source`` uint8, ``nseg`` int32 (and the two largest weights)."""
    seg = merge(labels, lo, cell, inv_cell, C, rays, masks, t_near, t_far) if seg is None else seg
    return _composite(seg, cells, stop, np.float32)


def referee(labels, cells, lo, cell, inv_cell, C, rays, masks, t_near, t_far, stop=0.0, seg=None):
    """The same segment list (cells, ``t_in``, ``t_out``, set) composited in float64."""
    seg = merge(labels, lo, cell, inv_cell, C, rays, masks, t_near, t_far) if seg is None else seg
    return _composite(seg, cells, stop, np.float64)


def bounds(got32, want64):
    """The tests' bound per output: 4 x the largest deviation of the float32 restatement from the float64 referee on the same inputs
    (the margin covers expf / sqrtf differences between the device and numpy)."""
    return {k: 4.0 * float(np.max(np.abs(got32[k].astype(np.float64) - want64[k]), initial=0.0)) for k in ("rgb", "depth", "acc")}


def ambiguous(want64, bound):
    """Pixels whose label the weights do not settle: a segment with positive density, and the two largest weights (0 standing in for a
    missing second: ``best_w`` starts there) closer than ``bound``."""
    second = np.maximum(want64["w2"], 0.0)
    return want64["positive"] & (want64["w1"] - second < bound)


# ---- the inputs both test files use
DIMS = (16, 12, 20)
LO, HI = T.LO, T.HI
VIEW = (50, 60)                 # rows, columns: 3000 rays, 46 full waves and a ragged one
NEAR, FAR = 0.0, 20.0
NAN = float("nan")


def volume(C, seed=7, empty=0.45):
    """Random labels ``0 .. C + 1`` (two of them >= C) with ``empty`` unlabelled, and cells: colour logits N(0, 3), densities 0 .. 40 with
    some exact zeros, negative values and NaNs."""
    rng = np.random.RandomState(seed + C)
    labels = rng.randint(0, C + 2, size=DIMS).astype(np.uint8)
    labels[rng.rand(*DIMS) < empty] = UNLABELLED
    cells = np.empty(DIMS + (4,), dtype=f32)
    cells[..., :3] = rng.randn(*DIMS, 3) * 3.0
    sigma = rng.exponential(6.0, size=DIMS)
    pick = rng.rand(*DIMS)
    sigma[pick < 0.05] = 0.0
    sigma[(pick >= 0.05) & (pick < 0.10)] = -3.0
    sigma[(pick >= 0.10) & (pick < 0.13)] = NAN
    sigma[(pick >= 0.13) & (pick < 0.16)] = 400.0                 # opaque
    cells[..., 3] = sigma
    return labels, cells


def view_rays(consts):
    """``o, d [3000, 3]`` f32: a 60 x 50 pinhole view of the box from outside, its first rows replaced by the crafted rays of
    ``_label_trace_restate`` (axis-parallel, a zero component inside and outside the box, an origin inside, NaN / inf / zero rays)."""
    lo, cell, inv_cell, dims = consts
    rows, colsn = VIEW
    centre = (np.asarray(LO, np.float64) + np.asarray(HI, np.float64)) / 2
    eye = centre + np.array([2.5, -3.0, 4.0])
    fwd = (centre - eye) / np.linalg.norm(centre - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    v, u = np.meshgrid((np.arange(rows) + 0.5) / rows - 0.5, (np.arange(colsn) + 0.5) / colsn - 0.5, indexing="ij")
    d = fwd[None, :] + 0.9 * u.reshape(-1, 1) * right[None, :] + 0.9 * v.reshape(-1, 1) * upv[None, :]
    o = np.repeat(eye[None, :], rows * colsn, axis=0)
    o, d = o.astype(f32), d.astype(f32)
    _, co, cd = T.crafted_rays(lo, cell, dims)
    o[:len(co)], d[:len(cd)] = co, cd
    return o, d


def ray_sets(consts, R):
    """``rays [R, 2, 3000, 3]``: set 0 the view, set r > 0 the view shifted and stretched (an affine map of set 0, as a target ray is)."""
    o, d = view_rays(consts)
    sets = [np.stack([o, d])]
    for r in range(1, R):
        sets.append(np.stack([o + np.asarray([0.2 * r, -0.15 * r, 0.1 * r], f32), (d * f32(1.0 + 0.25 * r)).astype(f32)]))
    return np.stack(sets)


def label_sets(C, R, overlapping):
    """R label sets over ``[0, C)``; for C = 128 they reach the fourth mask word."""
    top = C - 1
    if overlapping:
        sets = [list(range(C)), [0, 2, top], list(range(0, C, 2)), [1, top]]
    else:
        sets = [[l for l in range(C) if l % 4 == r] for r in range(4)]
        if R < 4:
            sets[R - 1] = [l for s in sets[R - 1:] for l in s]
    return sets[:R]


CASES = [(C, R, overlapping, stop) for C in (5, 128) for R, overlapping in ((1, False), (2, False), (2, True), (4, False), (4, True))
         for stop in (0.0, 0.05)]
