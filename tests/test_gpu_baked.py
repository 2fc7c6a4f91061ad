"""GPU tests of the baked field volume: ``dmnerf_bake_cells`` (csrc/label_grid.hip), ``dmnerf_baked_render`` (csrc/baked.hip),
``field.bake_grid`` / ``BakedGrid`` and ``editing.render_preview``.

The render's walk and merge are integers and f32 values that tests/_baked_restate.py restates bit for bit, so ``nseg`` is compared
exactly; ``rgb``, ``depth`` and ``acc`` go through ``expf`` / ``sqrtf``, which differ in the last bit between the device and numpy, so
they are held against the float64 referee within 4 x the float32 restatement's own largest deviation from it on the same inputs.
``label`` / ``source`` are compared exactly except where the referee's two largest weights lie closer than that bound (at most 1 % of
the pixels; tests/test_baked_restate.py holds the inputs to that cap).  Shapes: a 16 x 12 x 20 volume, 3000 rays (a ragged last wave)
that start with the crafted rays of the trace tests, C = 5 and 128, R = 1, 2 and 4, stop = 0 and 0.05."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import _baked_restate as B
import _label_grid_restate as LR
import _label_trace_restate as T
import _skip_restate as RS
import _gpu
from _gpu import A, model_from  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN = float("nan")
CONSTS = T.grid_consts(B.LO, B.HI, B.DIMS)


# ---- dmnerf_bake_cells
def bake_kernel(A, raw, C, thr):
    """The raw entry with one guard element behind each output."""
    raw = torch.from_numpy(np.ascontiguousarray(raw, dtype=f32)).cuda()
    M = raw.shape[0]
    labels = torch.full((M + 1,), 77, dtype=torch.uint8, device="cuda")
    cells = torch.full((M + 1, 4), -7.0, dtype=torch.float32, device="cuda")
    A.L.check(A.lib.dmnerf_bake_cells(A.L.ptr(raw), M, C, thr, A.L.ptr(labels), A.L.ptr(cells), A.L.stream()), "dmnerf_bake_cells")
    assert int(labels[M]) == 77 and bool((cells[M] == -7.0).all())
    return raw, labels[:M], cells[:M]


def crafted_rows(M, C, seed):
    """Random rows with, cyclically: a tie of two channels, sigma exactly at the threshold (0.5), a NaN sigma, a NaN colour logit in a
    labelled row, the empty row, sigma below the threshold, plain rows."""
    rng = np.random.RandomState(seed)
    raw = rng.randn(M, 4 + C).astype(f32)
    raw[:, 3] = np.abs(raw[:, 3]) + 1.0
    for m in range(M):
        kind = m % 8
        if kind == 0 and C > 1:
            a, b = sorted(rng.choice(C, 2, replace=False))
            raw[m, 4 + a] = raw[m, 4 + b] = 9.0
        elif kind == 1:
            raw[m, 3] = 0.5
        elif kind == 2:
            raw[m, 3] = NAN
        elif kind == 3:
            raw[m, 1] = NAN
        elif kind == 4:
            raw[m] = 0.0
            raw[m, -1] = 1.0
        elif kind == 5:
            raw[m, 3] = 0.25
    return raw


@pytest.mark.parametrize("C", [1, 5, 128])
@pytest.mark.parametrize("M", [1, 255, 257, 1000])
def test_bake_cells_equals_label_cells_and_the_masked_rows(A, C, M):
    raw, labels, cells = bake_kernel(A, crafted_rows(M, C, 10 * C + M), C, 0.5)
    plain = torch.empty(M, dtype=torch.uint8, device="cuda")
    A.L.check(A.lib.dmnerf_label_cells(A.L.ptr(raw), M, C, 0.5, A.L.ptr(plain), A.L.stream()), "dmnerf_label_cells")
    assert torch.equal(labels, plain)
    assert torch.equal(labels.cpu(), torch.from_numpy(LR.label_cells(raw.cpu().numpy(), C, 0.5)))
    want = torch.where((labels != 255)[:, None], raw[:, :4].view(torch.int32), torch.zeros(M, 4, dtype=torch.int32, device="cuda"))
    assert torch.equal(cells.view(torch.int32), want)                           # bit for bit: a NaN keeps its payload, a zero its sign
    if M >= 255:
        lab = labels.cpu()
        assert lab[1] == 255 and lab[2] == 255 and lab[4] == 255 and lab[5] == 255 and lab[3] != 255 and lab[6] != 255
        assert bool(torch.isnan(cells[3, 1])) and bool((cells[2] == 0).all())


_models = {}


def model(A, ins_num):
    if ins_num not in _models:
        _models[ins_num] = model_from(O.make_weights(72, ins_num, gain=1.7, sigma_bias=0.0), ins_num)
    return _models[ins_num]


@pytest.mark.parametrize("split", [None, "f16x2"])
def test_bake_grid_is_label_grid_with_the_rows_kept(A, split):
    dims, ins_num = (5, 6, 7), 13
    mf, C = model(A, ins_num), ins_num + 1
    occ = A.F.SkipGrid.from_bits(RS.pack_bits(np.random.RandomState(5).rand(*dims) < 0.6), B.LO, B.HI, dims)
    with torch.no_grad():
        baked = A.F.bake_grid(mf, occ, split=split, slab=2 * dims[1] * dims[2])            # more than one slab, a ragged last one
        plain = A.F.label_grid(mf, occ, split=split)
        o, d, z = [torch.from_numpy(t).cuda() for t in LR.label_rays(B.LO, B.HI, dims)]
        raw = A.R.run_network_skip(mf, o, d, z, occ, split=split).reshape(dims + (4 + C,))
    assert isinstance(baked, A.F.BakedGrid) and isinstance(baked, A.F.LabelGrid) and baked.dims == dims and baked.C == C
    assert torch.equal(baked.labels, plain.labels)
    labelled = baked.labels != 255
    assert 0.1 < float(labelled.float().mean()) < 0.9
    want = torch.where(labelled[..., None], raw[..., :4].view(torch.int32), torch.zeros_like(raw[..., :4]).view(torch.int32))
    assert baked.cells.dtype == torch.float32 and torch.equal(baked.cells.view(torch.int32), want)
    # everything a LabelGrid does still works
    assert torch.equal(baked.stats()["count"], plain.stats()["count"])
    assert torch.equal(baked.skip_grid([0, 1, 2]).bits, plain.skip_grid([0, 1, 2]).bits)
    ro, rd = [torch.from_numpy(t).cuda() for t in T.random_rays(100, 3)]
    for k, v in plain.trace(ro, rd, 0.0, 20.0).items():
        assert torch.equal(baked.trace(ro, rd, 0.0, 20.0)[k].view(torch.uint8), v.view(torch.uint8)), k


# ---- dmnerf_baked_render against the restatement and the referee
def render_kernel(A, labels, cells, rays, masks, near, far, stop, Cn):
    """The raw entry with one guard element behind every output."""
    lo, cell, inv_cell, dims = CONSTS
    L = A.L
    vol, cel = torch.from_numpy(labels).cuda(), torch.from_numpy(cells).cuda()
    r = torch.from_numpy(np.ascontiguousarray(rays, dtype=f32)).cuda()
    R, _, N, _ = r.shape
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    out = {"rgb": full((N + 1, 3), -7.0, torch.float32), "depth": full((N + 1,), -7.0, torch.float32), "acc": full((N + 1,), -7.0, torch.float32),
           "label": full((N + 1,), 77, torch.uint8), "source": full((N + 1,), 77, torch.uint8), "nseg": full((N + 1,), -7, torch.int32)}
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    words = (ctypes.c_uint32 * (4 * R))(*[w for m in masks for w in m])
    L.check(L.load().dmnerf_baked_render(L.ptr(vol), L.ptr(cel), f3(lo), f3(cell), f3(inv_cell), (ctypes.c_int * 3)(*dims), Cn, L.ptr(r), R, N,
                                         words, float(near), float(far), float(stop), L.ptr(out["rgb"]), L.ptr(out["depth"]),
                                         L.ptr(out["acc"]), L.ptr(out["label"]), L.ptr(out["source"]), L.ptr(out["nseg"]), L.stream()),
            "dmnerf_baked_render")
    for k, guard in (("rgb", -7.0), ("depth", -7.0), ("acc", -7.0), ("label", 77), ("source", 77), ("nseg", -7)):
        assert bool((out[k][N] == guard).all()), k
    return {k: v[:N].cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case_inputs(C, R, overlapping):
    """Volume, rays, masks and the segment list: computed once, shared by the stop values, never written to."""
    lo, cell, inv_cell, _ = CONSTS
    labels, cells = B.volume(C)
    rays = B.ray_sets(CONSTS, R)
    sets = B.label_sets(C, R, overlapping)
    masks = [T.mask_words(s, C) for s in sets]
    seg = B.merge(labels, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR)
    return labels, cells, rays, sets, masks, seg


def assert_render(got, labels, cells, C, rays, masks, seg, stop, what):
    lo, cell, inv_cell, _ = CONSTS
    r32 = B.render(labels, cells, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR, stop, seg=seg)
    r64 = B.referee(labels, cells, lo, cell, inv_cell, C, rays, masks, B.NEAR, B.FAR, stop, seg=seg)
    bound = B.bounds(r32, r64)
    worst = {k: float(np.abs(got[k].astype(np.float64) - r64[k]).max()) for k in bound}
    print(what, "bound", bound, "device", worst)
    assert got["nseg"].dtype == np.int32 and np.array_equal(got["nseg"], r32["nseg"]), what
    for k in bound:
        assert got[k].dtype == np.float32 and worst[k] <= bound[k], (what, k, worst[k], bound[k])
    unsure = B.ambiguous(r64, bound["acc"])
    assert unsure.mean() <= 0.01, what
    for k in ("label", "source"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k][~unsure], r32[k][~unsure]), (what, k)
    return r32


@pytest.mark.parametrize("C,R,overlapping,stop", B.CASES)
def test_render_kernel(A, C, R, overlapping, stop):
    labels, cells, rays, _, masks, seg = case_inputs(C, R, overlapping)
    assert rays.shape == (R, 2, 3000, 3) and labels.shape == (16, 12, 20)
    got = render_kernel(A, labels, cells, rays, masks, B.NEAR, B.FAR, stop, C)
    r32 = assert_render(got, labels, cells, C, rays, masks, seg, stop, (C, R, overlapping, stop))
    assert (r32["nseg"] == 0).any() and int(r32["nseg"].max()) >= 8 and set(np.unique(r32["source"])) >= set(range(R)) | {255}
    # the guarded rays (NaN / inf / zero direction outside the box) have no segment
    names, _, _ = T.crafted_rays(*CONSTS[:2], CONSTS[3])
    if R == 1:
        for name in ("nan_origin", "zero_direction_outside", "inf_direction", "nan_direction", "inf_origin", "misses_box", "points_away"):
            i = names.index(name)
            assert got["nseg"][i] == 0 and got["label"][i] == 255 and got["source"][i] == 255, name
            assert (got["rgb"][i] == 0).all() and got["depth"][i] == 0 and got["acc"][i] == 0, name
        assert got["nseg"][names.index("start_inside")] > 0 and got["nseg"][names.index("along_cell_edge")] > 0


def test_render_kernel_small_batches_and_other_bounds(A):
    labels, cells, rays, _, masks, _ = case_inputs(5, 2, True)
    lo, cell, inv_cell, _ = CONSTS
    for N, near, far in ((1, 0.0, 20.0), (63, 0.0, 20.0), (65, 2.5, 5.0), (65, -np.inf, 1e30)):
        sub = np.ascontiguousarray(rays[:, :, 19:19 + N])                        # behind the crafted rays: rays that hit
        seg = B.merge(labels, lo, cell, inv_cell, 5, sub, masks, near, far)
        got = render_kernel(A, labels, cells, sub, masks, near, far, 0.0, 5)
        r32 = B.render(labels, cells, lo, cell, inv_cell, 5, sub, masks, near, far, 0.0, seg=seg)
        assert np.array_equal(got["nseg"], r32["nseg"]), (N, near, far)
        assert np.allclose(got["acc"], r32["acc"], rtol=0, atol=1e-5) and np.allclose(got["depth"], r32["depth"], rtol=0, atol=1e-4)


def test_render_opaque_first_cell_is_the_trace(A):
    labels, cells, rays, _, _, _ = case_inputs(5, 1, False)
    opaque = cells.copy()
    opaque[..., 3] = 1e6
    every = [T.mask_words(range(5), 5)]
    grid = A.F.BakedGrid.from_arrays(torch.from_numpy(labels).cuda(), torch.from_numpy(opaque).cuda(), B.LO, B.HI, 5)
    dev = torch.from_numpy(rays).cuda()
    out = grid.render(dev[0, 0], dev[0, 1], B.NEAR, B.FAR, stop=0.5)           # the pixel ends behind the first cell that takes the weight
    tr = grid.trace(dev[0, 0], dev[0, 1], B.NEAR, B.FAR)
    assert sorted(out) == ["acc", "depth", "label", "nseg", "rgb", "source"]
    hit = tr["label"] != 255
    # (a ray can graze its first counted cell -- a corner, a sliver: no length, no full weight; those pixels are not the statement's)
    full = (out["nseg"] == 1) & (out["acc"] == 1)
    assert int(hit.sum()) > 1000 and int(full.sum()) >= 0.9 * int(hit.sum()) and bool(hit[full].all())
    assert torch.equal(out["label"][full], tr["label"][full]) and bool((out["source"][full] == 0).all())
    assert torch.equal(out["depth"][full].view(torch.int32), tr["t"][full].view(torch.int32))
    assert bool((out["depth"][~hit] == 0).all()) and bool((out["nseg"][~hit] == 0).all()) and bool((out["label"][~hit] == 255).all())
    first = torch.from_numpy(opaque).cuda().reshape(-1, 4)[tr["cell"][full].long()]
    assert torch.allclose(out["rgb"][full], torch.sigmoid(first[:, :3]), rtol=0, atol=1e-6)
    got = render_kernel(A, labels, opaque, rays, every, B.NEAR, B.FAR, 0.5, 5)
    assert np.array_equal(got["nseg"], out["nseg"].cpu().numpy())
    # an empty mask, and a volume without density
    none = grid.render(dev[0, 0], dev[0, 1], B.NEAR, B.FAR, labels=())
    for k in ("rgb", "depth", "acc", "nseg"):
        assert bool((none[k] == 0).all()), k
    assert bool((none["label"] == 255).all()) and bool((none["source"] == 255).all())
    thin = A.F.BakedGrid.from_arrays(grid.labels, torch.zeros_like(grid.cells), B.LO, B.HI, 5).render(dev[0, 0], dev[0, 1], B.NEAR, B.FAR)
    assert bool((thin["nseg"][hit] > 0).all()) and bool((thin["acc"] == 0).all()) and bool((thin["label"] == 255).all())


def test_render_sets_and_its_checks(A):
    labels, cells, rays, sets, masks, seg = case_inputs(128, 4, True)
    grid = A.F.BakedGrid.from_arrays(torch.from_numpy(labels).cuda(), torch.from_numpy(cells).cuda(), B.LO, B.HI, 128)
    dev = torch.from_numpy(rays).cuda()
    out = grid.render_sets(dev, sets, B.NEAR, B.FAR, stop=0.05)
    assert_render({k: v.cpu().numpy() for k, v in out.items()}, labels, cells, 128, rays, masks, seg, 0.05, "render_sets")
    empty = grid.render_sets(dev[:, :, :0].contiguous(), sets, B.NEAR, B.FAR)
    assert tuple(empty["rgb"].shape) == (0, 3) and tuple(empty["nseg"].shape) == (0,) and empty["nseg"].dtype == torch.int32
    with pytest.raises(ValueError, match="at most 4"):
        grid.render_sets(torch.cat([dev, dev[:1]]), sets + [[0]], B.NEAR, B.FAR)
    with pytest.raises(ValueError):
        grid.render_sets(dev, sets[:3], B.NEAR, B.FAR)
    with pytest.raises(ValueError):
        grid.render_sets(dev[:1], [[128]], B.NEAR, B.FAR)
    with pytest.raises(ValueError, match="stop"):
        grid.render_sets(dev, sets, B.NEAR, B.FAR, stop=-0.1)
    with pytest.raises(ValueError):
        grid.render(dev[0, 0], dev[0, 1, :5], B.NEAR, B.FAR)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        grid.render_sets(dev.cpu(), sets, B.NEAR, B.FAR)
    with pytest.raises(ValueError, match="cells"):
        A.F.BakedGrid.from_arrays(grid.labels, grid.cells[..., :3].contiguous(), B.LO, B.HI, 128)
    with pytest.raises(ValueError, match="cells"):
        A.F.BakedGrid.from_arrays(grid.labels, grid.cells.double(), B.LO, B.HI, 128)


# ---- render_preview: the scene of the trace tests (a front box, label 3, before a wider back box, label 5) with colours and densities
H, W = 24, 32
K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1.0]])
POSE = np.array([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 4.0], [0, 0, 0, 1]], dtype=np.float32)
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
FRONT, BACK, CS = 3, 5, 8
NEAR, FAR = 0.0, 10.0


def scene_volumes(second=False):
    vol = np.full((16, 16, 16), 255, np.uint8)
    if second:
        vol[2:14, 5:9, 8:11] = 6
        vol[6:10, 6:10, 12:14] = FRONT
    else:
        vol[4:12, 4:12, 3:6] = BACK
        vol[6:10, 6:10, 10:13] = FRONT
    rng = np.random.RandomState(9 + second)
    cells = np.zeros(vol.shape + (4,), f32)
    cells[..., :3] = rng.randn(*vol.shape, 3)
    cells[..., 3] = rng.uniform(1.0, 12.0, size=vol.shape)                       # soft: several cells share a pixel
    cells[vol == 255] = 0.0
    return vol, cells


@pytest.fixture(scope="module")
def scene(A):
    vol, cells = scene_volumes()
    baked = A.F.BakedGrid.from_arrays(torch.from_numpy(vol).cuda(), torch.from_numpy(cells).cuda(), *BOX, CS)
    return types.SimpleNamespace(vol=vol, cells=cells, baked=baked)


def shift_x(dx):
    m = np.eye(4)
    m[0, 3] = dx
    return m


renderer_rays = functools.partial(_gpu.renderer_rays, camera=(H, W, K, POSE), ins_num=CS - 1)


def assert_preview(A, scene, out, trans_list, target_labels, sets, keep=None, stop=0.0):
    want = scene.baked.render_sets(renderer_rays(A, trans_list, target_labels, keep), sets, NEAR, FAR, stop)
    assert tuple(out["rgb"].shape) == (H, W, 3) and tuple(out["nseg"].shape) == (H, W)
    for k in ("rgb", "depth", "acc"):
        assert torch.equal(out[k].reshape(-1).view(torch.int32), want[k].reshape(-1).view(torch.int32)), k
    for k in ("label", "source", "nseg"):
        assert torch.equal(out[k].reshape(-1), want[k]), k


def test_render_preview_is_render_sets_on_the_preview_s_rays_and_sets(A, scene):
    Ed, others = A.Ed, sorted(set(range(CS)) - {FRONT})
    call = lambda *a, **kw: Ed.render_preview(scene.baked, H, W, K, POSE, *a, near=NEAR, far=FAR, **kw)
    plain = call()
    assert_preview(A, scene, plain, [], [], [range(CS)])
    assert plain["ins_img"] is None and set(plain["label"].unique().tolist()) == {FRONT, BACK, 255}
    assert int(plain["nseg"].max()) >= 4 and 0.5 < float(plain["acc"].max()) <= 1.0 + 1e-6
    assert bool((plain["acc"][plain["label"] == 255].abs() < 1e-6).all())
    removed = call([Ed.Remove()], [FRONT])
    assert_preview(A, scene, removed, [Ed.Remove()], [FRONT], [others])
    assert not bool((removed["label"] == FRONT).any()) and bool((removed["label"][plain["label"] == FRONT] == BACK).all())
    moved = call([shift_x(0.5)], [FRONT], stop=0.05)
    assert_preview(A, scene, moved, [shift_x(0.5)], [FRONT], [others, [FRONT]], stop=0.05)
    seen = moved["label"] == FRONT
    assert int(seen.sum()) > 20 and bool((moved["source"][seen] == 1).all()) and bool((moved["source"][moved["label"] == BACK] == 0).all())
    copied = call([Ed.Copy(shift_x(0.5))], [FRONT])
    assert_preview(A, scene, copied, [Ed.Copy(shift_x(0.5))], [FRONT], [range(CS), [FRONT]])
    assert set(copied["source"][copied["label"] == FRONT].unique().tolist()) == {0, 1}
    edit = Ed.Deform("sin", 1)
    assert_preview(A, scene, call([edit], [FRONT]), [edit], [FRONT], [others, [FRONT]])
    kept = call([shift_x(0.5)], [FRONT], keep_labels=[BACK])
    assert_preview(A, scene, kept, [shift_x(0.5)], [FRONT], [[BACK], []], keep=[BACK])
    assert set(kept["label"].unique().tolist()) == {BACK, 255}
    three = [shift_x(0.5), Ed.Copy(shift_x(-0.5)), Ed.Remove(), shift_x(0.25)]
    assert_preview(A, scene, call(three, [FRONT, BACK, 6, 1]), three, [FRONT, BACK, 6, 1], [sorted(set(range(CS)) - {FRONT, 6, 1}), [FRONT], [BACK], [1]])
    with pytest.raises(ValueError, match="at most 3"):
        call(three + [shift_x(0.1)], [FRONT, BACK, 6, 1, 2])
    lut = torch.from_numpy(np.random.RandomState(3).randint(1, 256, size=(CS, 3)).astype(np.uint8)).cuda()
    coloured = call(lut=lut)
    hit = coloured["label"] != 255
    want = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
    want[hit] = lut[coloured["label"][hit].long()]
    assert torch.equal(coloured["ins_img"], want)
    with pytest.raises(ValueError):
        call(lut=lut[:CS - 1])


def test_preview_frame_is_unchanged_on_a_baked_grid(A, scene):
    plain = A.F.LabelGrid.from_labels(scene.baked.labels, *BOX, CS)
    lut = torch.from_numpy(np.random.RandomState(3).randint(1, 256, size=(CS, 3)).astype(np.uint8)).cuda()
    for edits, targets, kw in (([], [], {}), ([shift_x(0.5)], [FRONT], {}), ([A.Ed.Remove(), A.Ed.Copy(shift_x(0.5))], [BACK, FRONT], {}),
                               ([A.Ed.Deform("sin", 1)], [FRONT], dict(keep_labels=[FRONT, BACK]))):
        a = A.Ed.preview_frame(scene.baked, H, W, K, POSE, edits, targets, near=NEAR, far=FAR, lut=lut, **kw)
        b = A.Ed.preview_frame(plain, H, W, K, POSE, edits, targets, near=NEAR, far=FAR, lut=lut, **kw)
        assert sorted(a) == sorted(b) == ["depth", "ins_img", "label", "source"]
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    # a full-weight first cell: the render's label and depth are the hard preview's
    opaque = scene.baked.cells.clone()
    opaque[..., 3] = torch.where(scene.baked.labels != 255, 1e6, 0.0)
    grid = A.F.BakedGrid.from_arrays(scene.baked.labels, opaque, *BOX, CS)
    soft = A.Ed.render_preview(grid, H, W, K, POSE, [shift_x(0.5)], [FRONT], near=NEAR, far=FAR, stop=0.5)
    hard = A.Ed.preview_frame(grid, H, W, K, POSE, [shift_x(0.5)], [FRONT], near=NEAR, far=FAR)
    hit = hard["label"] != 255
    full = (soft["nseg"] == 1) & (soft["acc"] == 1)                             # (not the pixels that graze their first cell)
    assert int(full.sum()) >= 0.9 * int(hit.sum()) and bool(hit[full].all()) and bool((soft["label"][~hit] == 255).all())
    assert torch.equal(soft["label"][full], hard["label"][full]) and torch.equal(soft["source"][full], hard["source"][full])
    assert torch.equal(soft["depth"][full].view(torch.int32), hard["depth"][full].view(torch.int32))


def test_render_preview_captured_in_a_graph_follows_labels_and_cells(A):
    first, second = scene_volumes(), scene_volumes(second=True)
    make = lambda v: A.F.BakedGrid.from_arrays(torch.from_numpy(v[0]).cuda(), torch.from_numpy(v[1]).cuda(), *BOX, CS)
    lut = torch.from_numpy(np.random.RandomState(4).randint(1, 256, size=(CS, 3)).astype(np.uint8)).cuda()
    call = lambda grid: A.Ed.render_preview(grid, H, W, K, POSE, [shift_x(0.5)], [FRONT], near=NEAR, far=FAR, stop=0.01, lut=lut)
    eager = [call(make(v)) for v in (first, second)]                            # (also the warm-up)
    live = make(first)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(live)
    assert not torch.equal(eager[0]["label"], eager[1]["label"]) and not torch.equal(eager[0]["rgb"], eager[1]["rgb"])
    for v, e in ((second, eager[1]), (first, eager[0])):
        live.labels.copy_(torch.from_numpy(v[0]).cuda())                       # in place: the capture holds the pointers
        live.cells.copy_(torch.from_numpy(v[1]).cuda())
        out["label"].fill_(77)
        out["rgb"].fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        for key in ("label", "source", "nseg", "ins_img"):
            assert torch.equal(out[key], e[key]), key
        for key in ("rgb", "depth", "acc"):
            assert torch.equal(out[key].view(torch.int32), e[key].view(torch.int32)), key
