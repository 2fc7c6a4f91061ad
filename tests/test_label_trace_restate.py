"""The numpy restatement of csrc/label_trace.hip (tests/_label_trace_restate.py) against a float64 referee, on exact cases, and the
merge over ray sets.  CPU only: what the GPU tests compare the kernel with, bit for bit, is checked here first.

The referee sorts the float64 parameters of all plane crossings inside the clipped interval and looks the midpoint of every interval up
by counting planes: no stepping, no cell arithmetic of the kernel's.  The two may name different cells only where a ray passes within
f32 rounding of a cell edge (two crossings swap order) or starts within rounding of a plane; the share of such rays is capped at 0.5 %,
and on every other ray the hit's t agrees to ``4e-6 (1 + |t64|)``, a few f32 roundings of a plane crossing.

Observed on the inputs below (1500 rays per grid, seeds 11 and 12 -- the first ones tried -- three masks each, 9000 comparisons):
the restatement and the referee name another cell or label on 0 of them (0 %, cap 0.5 %); the largest ``|t - t64| / (1 + |t64|)`` on
the agreeing hits is 1.13e-7 (bound 4e-6).  Between 39 and 1042 of the 1500 rays of a case miss."""
import numpy as np
import pytest

import _label_trace_restate as T

f32 = np.float32
C = T.C_TEST
NEAR, FAR = 0.0, 20.0
N_RANDOM = 1500
KEEP = (1, 4, 9, 13)
MASKS = {"all": tuple(range(C)), "one": (3,), "keep": KEEP}


@pytest.fixture(scope="module", params=[0, 1], ids=["5x6x7", "8x8x33"])
def case(request):
    dims = T.GRIDS[request.param]
    lo, cell, inv_cell, dims = T.grid_consts(T.LO, T.HI, dims)
    labels = T.random_volume(dims, 40 + request.param)
    o, d = T.random_rays(N_RANDOM, 11 + request.param)
    walks = [T.referee_walk(dims, lo, cell, o[n], d[n], NEAR, FAR) for n in range(o.shape[0])]
    return dict(dims=dims, lo=lo, cell=cell, inv_cell=inv_cell, labels=labels, o=o, d=d, walks=walks)


def run(case, o, d, accepted, near=NEAR, far=FAR, labels=None):
    labels = case["labels"] if labels is None else labels
    return T.trace(labels, case["lo"], case["cell"], case["inv_cell"], C, o, d, T.mask_words(accepted, C), near, far)


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_restatement_against_the_float64_referee(case, mask):
    accepted = MASKS[mask]
    label, t, cell = run(case, case["o"], case["d"], accepted)
    label64, t64, cell64 = T.referee(case["labels"], case["walks"], C, accepted)
    differ = (label != label64) | (cell != cell64)
    share = differ.mean()
    agree_hit = ~differ & (cell64 >= 0)
    err = np.abs(t[agree_hit].astype(np.float64) - t64[agree_hit]) / (1 + np.abs(t64[agree_hit]))
    print(f"{case['dims']} {mask}: {differ.sum()} of {differ.size} rays differ ({share:.4%}), {agree_hit.sum()} agreeing hits, "
          f"{(cell64 < 0).sum()} misses, max t error {err.max():.3g}")
    assert agree_hit.sum() > 100 and (cell64 < 0).sum() > 10          # the inputs exercise hits and misses
    assert share <= 0.005
    assert (err <= 4e-6).all()
    miss = ~differ & (cell64 < 0)
    assert (label[miss] == 255).all() and np.isinf(t[miss]).all() and (t[miss] > 0).all()


def test_axis_aligned_columns(case):
    """Down the columns of ``field.label_rays``: the first accepted k, at the t the formula gives."""
    lo, cell, dims = case["lo"], case["cell"], case["dims"]
    o, d = T.column_rays(lo, cell, dims)
    for accepted in (tuple(range(C)), KEEP):
        label, t, g = run(case, o, d, accepted, near=0.0, far=1e9)
        cols = case["labels"].reshape(-1, dims[2])
        ok = (cols < C) & np.isin(cols, accepted)
        first = np.where(ok.any(1), ok.argmax(1), -1)
        want_cell = np.where(first >= 0, np.arange(cols.shape[0]) * dims[2] + first, -1)
        assert np.array_equal(g, want_cell.astype(np.int32))
        assert np.array_equal(label, np.where(first >= 0, cols[np.arange(cols.shape[0]), np.maximum(first, 0)], 255).astype(np.uint8))
        # k = 0: t_near; k > 0: the crossing of plane k, (plane_z(k) - o_z) * (1 / d_z), each operation rounded on its own
        inv = f32(1.0) / cell[2]
        plane = (lo[2] + (np.maximum(first, 0).astype(f32) * cell[2]).astype(f32)).astype(f32)
        want_t = np.where(first > 0, ((plane - o[:, 2]).astype(f32) * inv).astype(f32), f32(0.0))
        want_t = np.where(first >= 0, want_t, f32(np.inf)).astype(f32)
        assert np.array_equal(t.view(np.int32), want_t.view(np.int32))
        assert (first > 0).any() and (first == 0).any()


def crafted(case):
    names, o, d = T.crafted_rays(case["lo"], case["cell"], case["dims"])
    return {n: i for i, n in enumerate(names)}, o, d


def test_guarded_inputs_miss(case):
    idx, o, d = crafted(case)
    full = np.zeros(case["dims"], np.uint8)                         # every cell accepted: a ray that enters the walk at all hits
    label, t, g = run(case, o, d, tuple(range(C)), near=0.0, far=1e30, labels=full)
    for name in ("nan_origin", "zero_direction_outside", "inf_direction", "nan_direction", "inf_origin", "misses_box", "points_away",
                 "zero_x_outside", "zero_x_on_upper_face"):
        i = idx[name]
        assert (label[i], g[i]) == (255, -1) and t[i] == np.inf, name
    for name in ("start_inside", "start_inside_negative", "zero_x_inside", "zero_x_on_lower_face", "through_corner", "diagonal_back",
                 "along_cell_edge", "denormal_direction", "minus_zero_component"):
        assert label[idx[name]] == 0 and g[idx[name]] >= 0, name
    # a zero direction inside the box never leaves its cell: it hits it if accepted, and misses within the bound if not
    i = idx["zero_direction"]
    assert label[i] == 0 and t[i] == 0
    none = np.full(case["dims"], 255, np.uint8)
    label, t, g = run(case, o, d, tuple(range(C)), near=0.0, far=1e30, labels=none)
    assert (label == 255).all() and (g == -1).all() and np.isinf(t).all()


def test_nan_bounds_miss(case):
    idx, o, d = crafted(case)
    full = np.zeros(case["dims"], np.uint8)
    for near, far in ((T.NAN, 20.0), (0.0, T.NAN), (5.0, 5.0), (6.0, 5.0)):
        label, t, g = run(case, o, d, (0,), near=near, far=far, labels=full)
        assert (label == 255).all() and (g == -1).all()


def test_start_inside_hits_its_own_cell_at_t_near(case):
    idx, o, d = crafted(case)
    lo, inv_cell, dims = case["lo"], case["inv_cell"], case["dims"]
    full = np.zeros(dims, np.uint8)
    for name in ("start_inside", "start_inside_negative"):
        i = idx[name]
        for near in (0.0, 0.01):
            label, t, g = run(case, o[i:i + 1], d[i:i + 1], (0,), near=near, far=20.0, labels=full)
            p = (o[i] + (d[i] * f32(near)).astype(f32)).astype(f32)
            c = np.floor(((p - lo).astype(f32) * inv_cell).astype(f32)).astype(int)
            assert t[0] == f32(near) and g[0] == (c[0] * dims[1] + c[1]) * dims[2] + c[2]


def test_one_zero_component(case):
    """d_x == 0: the ray stays in its x slab; inside the slab it walks, outside (or on the upper face) it misses."""
    idx, o, d = crafted(case)
    dims = case["dims"]
    label, t, g = run(case, o, d, tuple(range(C)), near=0.0, far=1e9)
    i = idx["zero_x_inside"]
    walk = T.referee_walk(dims, case["lo"], case["cell"], o[i], d[i], 0.0, 1e9)
    l64, t64, g64 = T.referee(case["labels"], [walk], C, range(C))
    assert (label[i], g[i]) == (l64[0], g64[0])
    if g[i] >= 0:
        assert g[i] // (dims[1] * dims[2]) == dims[0] // 2 and abs(t[i] - t64[0]) <= 4e-6 * (1 + abs(t64[0]))
    assert g[idx["zero_x_outside"]] == -1 and g[idx["zero_x_on_upper_face"]] == -1


def test_short_t_far_is_a_miss(case):
    label, t, g = run(case, case["o"], case["d"], KEEP)
    hit = (g >= 0) & (t > 1e-3)
    assert hit.sum() > 100
    o, d = case["o"][hit], case["d"][hit]
    # t_far at the hit itself: the crossing into the accepted cell is not in front of t_exit
    for n in range(0, o.shape[0], 7):
        l2, t2, g2 = run(case, o[n:n + 1], d[n:n + 1], KEEP, far=float(t[hit][n]))
        assert (l2[0], g2[0]) == (255, -1) and t2[0] == np.inf
        l3, t3, g3 = run(case, o[n:n + 1], d[n:n + 1], KEEP, far=float(np.nextafter(t[hit][n], f32(np.inf))))
        assert g3[0] == g[hit][n] and t3[0] == t[hit][n]


def test_mask_passes_other_labels_through(case):
    dims = case["dims"]
    o, d = T.column_rays(case["lo"], case["cell"], dims)
    vol = np.full(dims, 2, np.uint8)
    vol[:, :, dims[2] - 1] = 5
    label, t, g = run(case, o, d, (5,), far=1e9, labels=vol)
    assert (label == 5).all() and (g % dims[2] == dims[2] - 1).all()
    label, t, g = run(case, o, d, (2, 5), far=1e9, labels=vol)
    assert (label == 2).all() and (g % dims[2] == 0).all()


def test_labels_from_C_on_are_never_hit(case):
    dims = case["dims"]
    o, d = T.column_rays(case["lo"], case["cell"], dims)
    vol = np.full(dims, 255, np.uint8)
    vol[:, :, 0], vol[:, :, 1] = C, 127
    every_bit = [0xffffffff] * 4                                    # a mask with all 128 bits set: still nothing >= C
    label, t, g = T.trace(vol, case["lo"], case["cell"], case["inv_cell"], C, o, d, every_bit, 0.0, 1e9)
    assert (label == 255).all() and (g == -1).all()
    vol[:, :, 3] = C - 1
    label, t, g = T.trace(vol, case["lo"], case["cell"], case["inv_cell"], C, o, d, every_bit, 0.0, 1e9)
    assert (label == C - 1).all() and (g % dims[2] == 3).all()


# ---- the merge over ray sets
def test_set_merge(case):
    dims, lo, cell, inv_cell = case["dims"], case["lo"], case["cell"], case["inv_cell"]
    o, d = case["o"], case["d"]
    N = o.shape[0]
    masks = [T.mask_words((3,), C), T.mask_words(KEEP, C), T.mask_words((0, 7), C)]
    shifted = o + np.asarray([0.3, 0.0, 0.0], f32)
    rays = np.stack([np.stack([o, d]), np.stack([shifted, d]), np.stack([o, d])])
    label, t, g, src = T.trace_sets(case["labels"], lo, cell, inv_cell, C, rays, masks, NEAR, FAR)
    singles = [T.trace(case["labels"], lo, cell, inv_cell, C, rays[r, 0], rays[r, 1], masks[r], NEAR, FAR) for r in range(3)]
    ts = np.stack([s[1] for s in singles])
    want_src = np.where(np.isinf(ts).all(0), 255, ts.argmin(0))     # argmin: the first of equal minima
    assert np.array_equal(src, want_src.astype(np.uint8))
    for r in range(3):
        m = src == r
        assert m.any()
        assert np.array_equal(label[m], singles[r][0][m]) and np.array_equal(g[m], singles[r][2][m]) and np.array_equal(t[m], ts[r][m])
    m = src == 255
    assert m.any() and (label[m] == 255).all() and (g[m] == -1).all() and np.isinf(t[m]).all()


def test_set_merge_equal_t_goes_to_the_lowest_set(case):
    lo, cell, inv_cell = case["lo"], case["cell"], case["inv_cell"]
    o, d = case["o"], case["d"]
    both = np.stack([np.stack([o, d]), np.stack([o, d])])
    everything = T.mask_words(range(C), C)
    label, t, g, src = T.trace_sets(case["labels"], lo, cell, inv_cell, C, both, [everything, everything], NEAR, FAR)
    assert ((src == 0) | (src == 255)).all() and (src == 0).any()
    # ... and to the higher one only where it is strictly nearer
    label, t, g, src = T.trace_sets(case["labels"], lo, cell, inv_cell, C, both, [T.mask_words((3,), C), everything], NEAR, FAR)
    one = T.trace(case["labels"], lo, cell, inv_cell, C, o, d, T.mask_words((3,), C), NEAR, FAR)
    full = T.trace(case["labels"], lo, cell, inv_cell, C, o, d, everything, NEAR, FAR)
    assert np.array_equal(src == 0, (one[2] >= 0) & (one[1] == full[1])) and (src == 1).any()
