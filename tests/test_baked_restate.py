"""The numpy restatement of csrc/baked.hip (tests/_baked_restate.py): its walk against the trace restatement, its segment order
against an independent float64 referee, its float32 compositing against the float64 one, the inputs of tests/test_gpu_baked.py against
the cap on ambiguous labels, and the argument checks of the entries and the Python layer that run before anything touches a device."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _baked_restate as B
import _label_trace_restate as T

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)


# ---- hand-written volumes: which segments, in which order
def hand_volume():
    """(5, 6, 7) cells: a slab of label 1, a block of label 2 behind it, a column of label 3 and a label >= C; the rest unlabelled."""
    vol = np.full(T.GRIDS[0], 255, np.uint8)
    vol[:, :, 1] = 1
    vol[1:4, 2:5, 3:6] = 2
    vol[2, 3, :] = 3
    vol[0, 0, 6] = 9
    return vol


def hand_rays(n=48):
    o, d = T.random_rays(n, 11)
    sets = [np.stack([o, d]), np.stack([o, d]), np.stack([o, (d * f32(1.25)).astype(f32)])]
    return np.stack(sets)


def test_segment_order_equals_the_sorted_referee():
    C = 4
    consts = T.grid_consts(T.LO, T.HI, T.GRIDS[0])
    lo, cell, inv_cell, dims = consts
    vol, rays = hand_volume(), hand_rays()
    wanted = [[1, 2, 3], [2, 3], [1, 3]]                                          # sets 0 and 1 share rays and labels 2, 3: equal t_in
    masks = [T.mask_words(s, C) for s in wanted]
    seg = B.merge(vol, lo, cell, inv_cell, C, rays, masks, 0.0, 20.0)
    flat = vol.reshape(-1)
    total = 0
    for n in range(rays.shape[2]):
        every = []
        for r in range(3):
            walk = T.referee_walk(dims, lo, cell, rays[r, 0, n], rays[r, 1, n], 0.0, 20.0)
            every += [(s, r, g) for s, g in walk if int(flat[g]) < C and int(flat[g]) in wanted[r]]
        every.sort(key=lambda e: (e[0], e[1]))
        k = int(seg["count"][n])
        assert k == len(every), n
        assert [(int(seg["set"][n, j]), int(seg["g"][n, j])) for j in range(k)] == [(r, g) for _, r, g in every], n
        assert np.allclose(seg["t_in"][n, :k], [s for s, _, _ in every], rtol=0, atol=1e-5)
        assert (seg["t_out"][n, :k] >= seg["t_in"][n, :k]).all()
        total += k
    assert total > 200
    out = B.render(vol, np.ones(vol.shape + (4,), f32), lo, cell, inv_cell, C, rays, masks, 0.0, 20.0, seg=seg)
    assert np.array_equal(out["nseg"], seg["count"])
    # equal t_in goes to the lowest set: sets 0 and 1 walk the same ray, so the shared cells come as (0, g), (1, g)
    pairs = sum(int(seg["set"][n, j]) == 0 and int(seg["set"][n, j + 1]) == 1 and seg["g"][n, j] == seg["g"][n, j + 1]
                for n in range(rays.shape[2]) for j in range(int(seg["count"][n]) - 1))
    assert pairs > 20


def test_first_segment_is_the_trace_restatement_s_hit():
    C = 5
    consts = T.grid_consts(B.LO, B.HI, B.DIMS)
    lo, cell, inv_cell, _ = consts
    labels, _ = B.volume(C)
    o, d = B.view_rays(consts)
    for accepted in (range(C), (1, 3)):
        words = T.mask_words(accepted, C)
        count, t_in, _, g, l = B.segments(labels, lo, cell, inv_cell, C, o, d, words, f32(B.NEAR), f32(B.FAR))
        hit, wl, wt, wc = T.trace_one(labels, lo, cell, inv_cell, C, o, d, words, f32(B.NEAR), f32(B.FAR))
        assert np.array_equal(count > 0, hit) and hit.any() and not hit.all()
        assert np.array_equal(l[hit, 0], wl[hit]) and np.array_equal(g[hit, 0], wc[hit])
        assert np.array_equal(t_in[hit, 0].view(np.int32), wt[hit].view(np.int32))


def test_opaque_first_cell_and_empty_inputs():
    consts = T.grid_consts(T.LO, T.HI, T.GRIDS[0])
    lo, cell, inv_cell, dims = consts
    vol = hand_volume()
    cells = np.zeros(vol.shape + (4,), f32)
    cells[..., 3] = 1e6
    cells[..., 0] = 2.0
    rays = hand_rays()[:1]
    every = [T.mask_words(range(4), 4)]
    out = B.render(vol, cells, lo, cell, inv_cell, 4, rays, every, 0.0, 20.0)
    wl, wt, _, _ = T.trace_sets(vol, lo, cell, inv_cell, 4, rays, every, 0.0, 20.0)
    hit = wl != 255
    assert hit.any() and np.array_equal(out["label"], wl)
    assert np.array_equal(out["depth"][hit].view(np.int32), wt[hit].view(np.int32)) and (out["acc"][hit] == 1).all()
    assert np.allclose(out["rgb"][hit], [1 / (1 + np.exp(-2.0)), 0.5, 0.5], rtol=0, atol=1e-6)
    for o in (out, B.render(vol, cells, lo, cell, inv_cell, 4, rays, [[0, 0, 0, 0]], 0.0, 20.0)):
        miss = ~hit if o is out else np.ones_like(hit)
        assert (o["nseg"][miss] == 0).all() and (o["label"][miss] == 255).all() and (o["source"][miss] == 255).all()
        assert (o["rgb"][miss] == 0).all() and (o["depth"][miss] == 0).all() and (o["acc"][miss] == 0).all()
    # a NaN density and a density of zero contribute nothing
    cells[..., 3] = np.where(vol == 1, np.nan, 0.0)
    out = B.render(vol, cells, lo, cell, inv_cell, 4, rays, every, 0.0, 20.0)
    assert (out["nseg"][hit] > 0).all() and (out["acc"] == 0).all() and (out["label"] == 255).all()


# ---- float32 against float64, and the inputs of the GPU test
def float_bound(seg, far):
    """What float32 may lose against float64 on one pixel.  A segment makes about ten f32 roundings on values of at most 1 (alpha, w, T,
    the sigmoid; expf's argument is rounded with relative error eps, which moves exp(-x) by at most x eps exp(-x) <= eps / e), and adds
    w * value into a sum of at most 1 (rgb, acc) or |t| <= far (depth): at most 16 eps per segment and unit of scale, errors of earlier
    segments carried through T included."""
    n = float(seg["count"].max())
    return {"rgb": 16 * EPS * n, "acc": 16 * EPS * n, "depth": 16 * EPS * n * far}


@pytest.mark.parametrize("C,R,overlapping,stop", B.CASES)
def test_float32_statement_against_the_float64_one(C, R, overlapping, stop):
    consts = T.grid_consts(B.LO, B.HI, B.DIMS)
    lo, cell, inv_cell, _ = consts
    labels, cells = B.volume(C)
    rays = B.ray_sets(consts, R)
    masks = [T.mask_words(s, C) for s in B.label_sets(C, R, overlapping)]
    seg = B.merge(labels, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR)
    got = B.render(labels, cells, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR, stop, seg=seg)
    want = B.referee(labels, cells, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR, stop, seg=seg)
    limit = float_bound(seg, B.FAR)
    for k in ("rgb", "depth", "acc"):
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all()
        assert float(np.abs(got[k] - want[k]).max()) <= limit[k], k
    assert np.array_equal(got["nseg"], want["nseg"])
    # the inputs exercise what they are meant to: hits and misses, several segments, every set, an early stop
    assert (got["nseg"] == 0).any() and int(got["nseg"].max()) >= 8
    assert set(np.unique(got["source"])) >= set(range(R)) | {255}
    if stop:
        assert (got["nseg"] < seg["count"]).any()
    else:
        assert np.array_equal(got["nseg"], seg["count"])
    if C == 128:
        assert int(got["label"][got["label"] != 255].max()) >= 96                # the fourth mask word
    # the GPU test may leave out pixels whose label the weights do not settle: the referee alone keeps them under 1 %
    bound = B.bounds(got, want)
    unsure = B.ambiguous(want, bound["acc"])
    assert unsure.mean() <= 0.01
    assert np.array_equal(got["label"][~unsure], want["label"][~unsure]) and np.array_equal(got["source"][~unsure], want["source"][~unsure])


# ---- argument checks that run before anything touches a device
def test_entries_validate_arguments():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)                                                   # never dereferenced: every call below is refused
    for C in (0, 129):
        assert lib.dmnerf_bake_cells(p, 4, C, 0.0, p, p, None) == -1 and "C=" in _lib.last_error()
    assert lib.dmnerf_bake_cells(p, -1, 14, 0.0, p, p, None) == -1
    for thr in (-1.0, B.NAN):
        assert lib.dmnerf_bake_cells(p, 4, 14, thr, p, p, None) == -1 and "sigma_threshold" in _lib.last_error()
    assert lib.dmnerf_bake_cells(None, 4, 14, 0.0, p, p, None) == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_bake_cells(p, 4, 14, 0.0, p, None, None) == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_bake_cells(p, 4, 14, 0.0, p, ctypes.c_void_p(68), None) == -1 and "aligned" in _lib.last_error()
    assert lib.dmnerf_bake_cells(None, 0, 14, 0.0, None, None, None) == 0      # nothing to do
    f3, i3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    w = (ctypes.c_uint32 * 16)()
    call = lambda dims=i3, Cn=4, R=1, N=1, vol=p, cells=p, masks=w, stop=0.0: lib.dmnerf_baked_render(
        vol, cells, f3, f3, f3, dims, Cn, p, R, N, masks, 0.0, 1.0, stop, p, p, p, p, p, p, None)
    for kw, text in ((dict(N=-1), "bad N"), (dict(R=0), "R=0"), (dict(R=5), "R=5"), (dict(Cn=0), "C=0"), (dict(Cn=129), "C=129"),
                     (dict(dims=(ctypes.c_int * 3)(4, 0, 4)), "bad dims"), (dict(dims=(ctypes.c_int * 3)(2048, 1024, 1024)), "int32"),
                     (dict(vol=None), "null"), (dict(cells=None), "null"), (dict(masks=None), "null"), (dict(stop=-0.5), "stop"),
                     (dict(stop=B.NAN), "stop"), (dict(cells=ctypes.c_void_p(72)), "aligned")):
        assert call(**kw) == -1 and text in _lib.last_error(), kw
    assert call(N=0, vol=None, cells=None) == 0                                # no launch, nothing read


def test_python_layer_validates_arguments():
    from dm_nerf_amd import editing as Ed, field as F
    for thr in (-0.5, B.NAN):
        with pytest.raises(ValueError, match="sigma_threshold"):
            F.bake_grid(None, None, sigma_threshold=thr)
    with pytest.raises(TypeError, match="SkipGrid"):
        F.bake_grid(None, "grid")
    assert issubclass(F.BakedGrid, F.LabelGrid) and F.MAX_RENDER_SETS == 4
    labels, cells = torch.zeros(2, 3, 4, dtype=torch.uint8), torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.BakedGrid.from_arrays(labels, cells, (0, 0, 0), (1, 1, 1), 5)
    stand_in = types.SimpleNamespace(C=8)                                      # the checks below come before the grid is looked at
    rays = torch.zeros(5, 2, 7, 3)
    with pytest.raises(ValueError, match="at most 4"):
        F.BakedGrid.render_sets(stand_in, rays, [0] * 5, 0.0, 1.0)
    for stop in (-1.0, B.NAN):
        with pytest.raises(ValueError, match="stop"):
            F.BakedGrid.render_sets(stand_in, rays[:1], [0], 0.0, 1.0, stop=stop)
        with pytest.raises(ValueError, match="stop"):
            Ed.render_preview(stand_in, 4, 4, np.eye(3), np.eye(4), stop=stop)
    with pytest.raises(ValueError, match="target labels"):
        Ed.render_preview(stand_in, 4, 4, np.eye(3), np.eye(4), [np.eye(4)], [])
    with pytest.raises(ValueError, match="outside"):
        Ed.render_preview(stand_in, 4, 4, np.eye(3), np.eye(4), [np.eye(4)], [8])
    four = [np.eye(4), Ed.Copy(np.eye(4)), Ed.Deform("sin", 1), np.eye(4)]
    with pytest.raises(ValueError, match="at most 3"):
        Ed.render_preview(stand_in, 4, 4, np.eye(3), np.eye(4), four, [1, 2, 3, 4])
    with pytest.raises(ValueError, match="at most 3"):
        Ed.render_preview(stand_in, 4, 4, np.eye(3), np.eye(4), four + [Ed.Remove()], [1, 2, 3, 4, 5])
