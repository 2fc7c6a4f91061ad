"""GPU tests of the label trace: ``dmnerf_label_trace`` (csrc/label_trace.hip) on crafted and random inputs, ``LabelGrid.trace`` /
``trace_sets``, ``editing.pick`` / ``editing.preview_frame`` and a graph capture.  Labels, cells and sources are integers and the
kernel's arithmetic is restated operation for operation in tests/_label_trace_restate.py: every comparison is ``torch.equal``, ``t``
by its bits.  (tests/test_label_trace_restate.py holds that restatement against a float64 referee.)

The picking / preview scene: a 16^3 volume over [-1, 1]^3, a front box (label 3, 4 x 4 x 3 cells round the z axis at z 0.25 .. 0.625) and
a wider back box (label 5, 8 x 8 x 3 cells at z -0.625 .. -0.25), seen from (0, 0, 4) down -z by a 32 x 24 camera of focal length 40."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _label_trace_restate as T
from _gpu import A  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32
C = T.C_TEST
KEEP = (1, 4, 9, 13)


def bits(t):
    return t.view(torch.int32)


def assert_same(got, want, what=""):
    """(label, t, cell[, source]) device tensors against the restatement's numpy arrays, bit for bit."""
    for name, g, w in zip(("label", "t", "cell", "source"), got, want):
        w = torch.from_numpy(np.ascontiguousarray(w))
        g = g.cpu()
        assert g.dtype == w.dtype, (what, name)
        assert torch.equal(bits(g), bits(w)) if name == "t" else torch.equal(g, w), (what, name)


def kernel(A, labels, consts, rays, masks, near, far, Cn=C):
    """The raw entry with one guard element behind every output."""
    lo, cell, inv_cell, dims = consts
    L = A.L
    vol = torch.from_numpy(labels).cuda()
    r = torch.from_numpy(np.ascontiguousarray(rays, dtype=f32)).cuda()
    R, _, N, _ = r.shape
    label = torch.full((N + 1,), 77, dtype=torch.uint8, device="cuda")
    t = torch.full((N + 1,), -7.0, dtype=torch.float32, device="cuda")
    cells = torch.full((N + 1,), -7, dtype=torch.int32, device="cuda")
    source = torch.full((N + 1,), 77, dtype=torch.uint8, device="cuda")
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    words = (ctypes.c_uint32 * (4 * R))(*[w for m in masks for w in m])
    L.check(L.load().dmnerf_label_trace(L.ptr(vol), f3(lo), f3(cell), f3(inv_cell), (ctypes.c_int * 3)(*dims), Cn, L.ptr(r), R, N, words,
                                        float(near), float(far), L.ptr(label), L.ptr(t), L.ptr(cells), L.ptr(source), L.stream()),
            "dmnerf_label_trace")
    assert int(label[N]) == 77 and float(t[N]) == -7.0 and int(cells[N]) == -7 and int(source[N]) == 77
    return label[:N], t[:N], cells[:N], source[:N]


def inputs(g, N, R):
    """N rays per set: the crafted rays first (as many as fit), random ones behind them; set r > 0 is set 0 shifted and re-aimed."""
    consts = T.grid_consts(T.LO, T.HI, T.GRIDS[g])
    lo, cell, inv_cell, dims = consts
    _, co, cd = T.crafted_rays(lo, cell, dims)
    ro, rd = T.random_rays(max(N, 2), 100 * g + N)
    o, d = np.concatenate([co, ro])[:N], np.concatenate([cd, rd])[:N]
    sets = [np.stack([o, d])]
    for r in range(1, R):
        sets.append(np.stack([o + np.asarray([0.2 * r, -0.1 * r, 0.0], f32), (d * f32(1.0 + 0.25 * r)).astype(f32)]))
    masks = [T.mask_words(m, C) for m in (range(C), (3,), KEEP)][:R]
    return consts, T.random_volume(dims, 40 + g), np.stack(sets), masks


# ---- the kernel against the restatement
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 257, 1000])
@pytest.mark.parametrize("g", [0, 1])
def test_kernel_equals_the_restatement(A, g, N, R):
    consts, labels, rays, masks = inputs(g, N, R)
    for near, far in ((0.0, 20.0), (0.5, 4.0)):
        want = T.trace_sets(labels, *consts[:3], C, rays, masks, near, far)
        assert_same(kernel(A, labels, consts, rays, masks, near, far), want, (g, N, R, near, far))
    if N >= 63:
        assert (want[0] != 255).any() and (want[0] == 255).any()
        if R == 3 and N >= 257:
            assert set(np.unique(want[3])) >= {0, 1, 255}


@pytest.mark.parametrize("g", [0, 1])
def test_kernel_on_crafted_rays_and_columns(A, g):
    consts = T.grid_consts(T.LO, T.HI, T.GRIDS[g])
    lo, cell, inv_cell, dims = consts
    names, o, d = T.crafted_rays(lo, cell, dims)
    labels = T.random_volume(dims, 40 + g)
    every = T.mask_words(range(C), C)
    for vol in (labels, np.zeros(dims, np.uint8), np.full(dims, 255, np.uint8), np.full(dims, C, np.uint8)):
        for near, far in ((0.0, 1e30), (T.NAN, 20.0), (0.0, T.NAN), (-np.inf, np.inf)):
            rays = np.stack([o, d])[None]
            want = T.trace_sets(vol, lo, cell, inv_cell, C, rays, [every], near, far)
            assert_same(kernel(A, vol, consts, rays, [every], near, far), want, (names, near, far))
    # the guarded rays miss even where every cell is accepted
    got = kernel(A, np.zeros(dims, np.uint8), consts, np.stack([o, d])[None], [every], 0.0, 1e30)
    for name in ("nan_origin", "zero_direction_outside", "inf_direction", "nan_direction", "inf_origin"):
        i = names.index(name)
        assert (int(got[0][i]), float(got[1][i]), int(got[2][i]), int(got[3][i])) == (255, float("inf"), -1, 255), name
    co, cd = T.column_rays(lo, cell, dims)
    for accepted in (range(C), KEEP, (3,)):
        rays, m = np.stack([co, cd])[None], [T.mask_words(accepted, C)]
        assert_same(kernel(A, labels, consts, rays, m, 0.0, 1e9), T.trace_sets(labels, lo, cell, inv_cell, C, rays, m, 0.0, 1e9), "columns")


def test_kernel_equal_t_goes_to_the_lowest_set_and_C_bounds_the_labels(A):
    consts, labels, rays, _ = inputs(1, 257, 1)
    every = [0xffffffff] * 4
    both = np.concatenate([rays, rays])
    got = kernel(A, labels, consts, both, [every, every], 0.0, 20.0)
    assert_same(got, T.trace_sets(labels, *consts[:3], C, both, [every, every], 0.0, 20.0))
    assert set(np.unique(got[3].cpu().numpy())) == {0, 255}
    assert int(got[0][got[0] != 255].max()) == C - 1                          # labels C and C + 1 are in the volume, and in the mask
    for Cn in (1, 5, 128):
        assert_same(kernel(A, labels, consts, rays, [every], 0.0, 20.0, Cn=Cn), T.trace_sets(labels, *consts[:3], Cn, rays, [every], 0.0, 20.0), Cn)


def test_entry_validates_its_arguments(A):
    L, lib = A.L, A.lib
    f3, i3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    w = (ctypes.c_uint32 * 64)()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = L.ptr(x)
    call = lambda dims=i3, Cn=4, R=1, N=1, vol=p, masks=w: lib.dmnerf_label_trace(vol, f3, f3, f3, dims, Cn, p, R, N, masks, 0.0, 1.0, p, p, p, p,
                                                                                 L.stream())
    for kw, text in ((dict(N=-1), "bad N"), (dict(R=0), "R=0"), (dict(R=17), "R=17"), (dict(Cn=0), "C=0"), (dict(Cn=129), "C=129"),
                     (dict(dims=(ctypes.c_int * 3)(4, 0, 4)), "bad dims"), (dict(dims=(ctypes.c_int * 3)(2048, 1024, 1024)), "int32"),
                     (dict(vol=None), "null"), (dict(masks=None), "null")):
        assert call(**kw) == -1 and text in L.last_error(), kw
    assert call(N=0, vol=None) == 0                                            # no launch, nothing read


# ---- LabelGrid.trace / trace_sets
def grid_of(A, labels, Cn=C):
    return A.F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), T.LO, T.HI, Cn)


@pytest.mark.parametrize("g", [0, 1])
def test_label_grid_trace(A, g):
    consts, labels, rays, masks = inputs(g, 1000, 3)
    lg = grid_of(A, labels)
    assert np.array_equal(lg.inv_cell, consts[2]) and np.array_equal(lg.cell, consts[1])
    dev = torch.from_numpy(rays).cuda()
    out = lg.trace_sets(dev, [range(C), 3, KEEP], 0.0, 20.0)
    assert_same([out[k] for k in ("label", "t", "cell", "source")], T.trace_sets(labels, *consts[:3], C, rays, masks, 0.0, 20.0))
    for accepted in (None, 3, KEEP, ()):
        out = lg.trace(dev[0, 0], dev[0, 1], 0.25, 20.0, labels=accepted)
        assert sorted(out) == ["cell", "label", "t"]
        words = T.mask_words(range(C) if accepted is None else [accepted] if isinstance(accepted, int) else accepted, C)
        assert_same([out[k] for k in ("label", "t", "cell")], T.trace(labels, *consts[:3], C, rays[0, 0], rays[0, 1], words, 0.25, 20.0))
    empty = lg.trace(dev[0, 0, :0], dev[0, 1, :0], 0.0, 20.0)
    assert all(tuple(empty[k].shape) == (0,) for k in ("label", "t", "cell"))
    assert empty["label"].dtype == torch.uint8 and empty["t"].dtype == torch.float32 and empty["cell"].dtype == torch.int32


def test_label_grid_trace_refuses_bad_arguments(A):
    consts, labels, rays, _ = inputs(0, 63, 1)
    lg = grid_of(A, labels)
    dev = torch.from_numpy(rays).cuda()
    o, d = dev[0, 0], dev[0, 1]
    for bad in (C, -1, [0, C], 2.5, [1.0], "3"):
        with pytest.raises(ValueError):
            lg.trace(o, d, 0.0, 20.0, labels=bad)
    with pytest.raises(ValueError):
        lg.trace_sets(dev, [range(C), 3], 0.0, 20.0)                           # two label sets for one ray set
    with pytest.raises(ValueError):
        lg.trace(o, d[:5], 0.0, 20.0)
    with pytest.raises(ValueError):
        lg.trace(o.double(), d.double(), 0.0, 20.0)
    with pytest.raises(ValueError):
        lg.trace_sets(dev.expand(17, -1, -1, -1).contiguous(), [0] * 17, 0.0, 20.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lg.trace(o.cpu(), d.cpu(), 0.0, 20.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lg.trace_sets(dev.cpu(), [0], 0.0, 20.0)


# ---- picking and previews
H, W = 24, 32
K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1.0]])
POSE = np.array([[1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 4.0], [0, 0, 0, 1]], dtype=np.float32)     # get_rays_k looks along camera +z
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
FRONT, BACK, CS = 3, 5, 8
NEAR, FAR = 0.0, 10.0


def scene_labels():
    vol = np.full((16, 16, 16), 255, np.uint8)
    vol[4:12, 4:12, 3:6] = BACK
    vol[6:10, 6:10, 10:13] = FRONT
    return vol


@pytest.fixture(scope="module")
def scene(A):
    vol = scene_labels()
    lg = A.F.LabelGrid.from_labels(torch.from_numpy(vol).cuda(), *BOX, CS)
    consts = T.grid_consts(*BOX, vol.shape)
    return types.SimpleNamespace(vol=vol, lg=lg, consts=consts)


def restate_frame(A, scene, trans_list, target_labels, sets, vol=None, keep=None):
    """The restatement on the rays ``ManipulationFrameRenderer`` itself generates for the edit."""
    args = types.SimpleNamespace(N_importance=0, target_labels=list(target_labels))
    fr = A.D.ManipulationFrameRenderer(H, W, K, torch.from_numpy(POSE), trans_list, None, args, ins_num=CS - 1, rank=0, world=1,
                                       keep_labels=keep if (keep is not None or trans_list) else ())
    rays = np.concatenate([fr.ori[None].cpu().numpy(), fr.tar.cpu().numpy()]) if fr.T else fr.ori[None].cpu().numpy()
    assert rays.shape[0] == len(sets)
    return T.trace_sets(scene.vol if vol is None else vol, *scene.consts[:3], CS, rays, [T.mask_words(s, CS) for s in sets], NEAR, FAR)


def assert_frame(out, want):
    assert tuple(out["label"].shape) == (H, W) and tuple(out["depth"].shape) == (H, W) and tuple(out["source"].shape) == (H, W)
    assert_same([out["label"].reshape(-1), out["depth"].reshape(-1), None, out["source"].reshape(-1)][:2], want[:2])
    assert torch.equal(out["source"].reshape(-1).cpu(), torch.from_numpy(want[3]))


def test_pick(A, scene):
    from dm_nerf_amd.networks import helpers
    pixels = [(16, 12), (15, 11), (17, 12), (12, 12), (1, 1), (31, 23)]
    label, t, point, cell = A.Ed.pick(scene.lg, H, W, K, POSE, pixels, NEAR, FAR)
    assert label.tolist() == [FRONT, FRONT, FRONT, BACK, 255, 255]
    assert cell[0].tolist() == [8, 8, 12] and cell[3, 2] == 5 and cell[4].tolist() == [-1, -1, -1]
    assert np.isinf(t[4:]).all() and not np.isfinite(point[4:]).any()
    ro, rd = helpers.get_rays_k(H, W, K, torch.from_numpy(POSE))                # the project's rays of those pixels
    idx = [r * W + c for c, r in pixels]
    o, d = ro.reshape(-1, 3)[idx].cpu().numpy(), rd.reshape(-1, 3)[idx].cpu().numpy()
    wl, wt, wc = T.trace(scene.vol, *scene.consts[:3], CS, o, d, T.mask_words(range(CS), CS), NEAR, FAR)
    assert np.array_equal(label, wl) and np.array_equal(t.view(np.int32), wt.view(np.int32))
    assert np.array_equal(cell[:4], np.stack(np.unravel_index(wc[:4], scene.vol.shape), 1))
    assert np.array_equal(point[:4], o[:4].astype(np.float64) + d[:4].astype(np.float64) * wt[:4].astype(np.float64)[:, None])
    assert abs(point[0, 2] - 0.625) < 1e-6 and abs(point[3, 2] + 0.25) < 1e-6   # the faces of the two boxes that look at the camera
    # restricted to the back box, the centre pixel looks through the front one
    label, t, point, cell = A.Ed.pick(scene.lg, H, W, K, POSE, pixels[:1], NEAR, FAR, labels=BACK)
    assert label.tolist() == [BACK] and cell[0].tolist() == [8, 8, 5]
    with pytest.raises(ValueError):
        A.Ed.pick(scene.lg, H, W, K, POSE, [(W, 0)], NEAR, FAR)


def test_preview_without_an_edit_is_the_trace_of_the_frame(A, scene):
    from dm_nerf_amd.networks import helpers
    out = A.Ed.preview_frame(scene.lg, H, W, K, POSE, near=NEAR, far=FAR)
    ro, rd = helpers.get_rays_k(H, W, K, torch.from_numpy(POSE))
    tr = scene.lg.trace(ro.reshape(-1, 3), rd.reshape(-1, 3), NEAR, FAR)
    assert torch.equal(out["label"].reshape(-1), tr["label"]) and torch.equal(bits(out["depth"].reshape(-1)), bits(tr["t"]))
    assert out["ins_img"] is None
    assert set(out["source"].unique().tolist()) == {0, 255} and torch.equal(out["source"] == 255, out["label"] == 255)
    assert set(out["label"].unique().tolist()) == {FRONT, BACK, 255} and int(out["label"][12, 16]) == FRONT
    assert_frame(out, restate_frame(A, scene, [], [], [range(CS)]))


def test_preview_remove_uncovers_the_back_box(A, scene):
    plain = A.Ed.preview_frame(scene.lg, H, W, K, POSE, near=NEAR, far=FAR)
    out = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [A.Ed.Remove()], [FRONT], near=NEAR, far=FAR)
    was_front = plain["label"] == FRONT
    assert int(was_front.sum()) > 20 and bool((out["label"][was_front] == BACK).all())
    assert torch.equal(out["label"][~was_front], plain["label"][~was_front]) and not bool((out["label"] == FRONT).any())
    assert_frame(out, restate_frame(A, scene, [A.Ed.Remove()], [FRONT], [sorted(set(range(CS)) - {FRONT})]))


def shift_x(dx):
    m = np.eye(4)
    m[0, 3] = dx
    return m


def test_preview_rigid_move_and_copy(A, scene):
    plain = A.Ed.preview_frame(scene.lg, H, W, K, POSE, near=NEAR, far=FAR)
    others = sorted(set(range(CS)) - {FRONT})
    move = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [shift_x(0.5)], [FRONT], near=NEAR, far=FAR)
    assert_frame(move, restate_frame(A, scene, [shift_x(0.5)], [FRONT], [others, [FRONT]]))
    seen, before = move["label"] == FRONT, plain["label"] == FRONT
    assert int(seen.sum()) > 20 and bool((move["source"][seen] == 1).all()) and bool((move["source"][move["label"] == BACK] == 0).all())
    cols = lambda m: m.any(0).nonzero().flatten()
    assert int(cols(seen).max()) < int(cols(before).min())                     # the camera went right: the object shows to the left
    assert bool((move["label"][before & ~seen] == BACK).all())                 # where it was, the back box shows
    copy = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [A.Ed.Copy(shift_x(0.5))], [FRONT], near=NEAR, far=FAR)
    assert_frame(copy, restate_frame(A, scene, [A.Ed.Copy(shift_x(0.5))], [FRONT], [range(CS), [FRONT]]))
    twice = copy["label"] == FRONT
    assert bool(twice[before].all()) and bool(twice[seen].all()) and int(twice.sum()) == int((before | seen).sum())
    assert set(copy["source"][twice].unique().tolist()) == {0, 1}
    # two entries, one without rays: the sets are [original, target of the move]
    both = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [A.Ed.Remove(), shift_x(0.5)], [BACK, FRONT], near=NEAR, far=FAR)
    assert_frame(both, restate_frame(A, scene, [A.Ed.Remove(), shift_x(0.5)], [BACK, FRONT],
                                     [sorted(set(range(CS)) - {FRONT, BACK}), [FRONT]]))
    assert set(both["label"].unique().tolist()) == {FRONT, 255}


def test_preview_deform(A, scene):
    edit = A.Ed.Deform("sin", 1)
    out = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [edit], [FRONT], near=NEAR, far=FAR)
    assert_frame(out, restate_frame(A, scene, [edit], [FRONT], [sorted(set(range(CS)) - {FRONT}), [FRONT]]))
    assert bool((out["label"] == FRONT).any()) and bool((out["source"][out["label"] == FRONT] == 1).all())


def test_preview_keep_labels_and_lut(A, scene):
    lut = torch.from_numpy(np.random.RandomState(3).randint(1, 256, size=(CS, 3)).astype(np.uint8)).cuda()
    plain = A.Ed.preview_frame(scene.lg, H, W, K, POSE, near=NEAR, far=FAR, lut=lut)
    only = A.Ed.preview_frame(scene.lg, H, W, K, POSE, keep_labels=[BACK], near=NEAR, far=FAR, lut=lut)
    assert set(only["label"].unique().tolist()) == {BACK, 255}
    assert bool((only["label"][plain["label"] != 255] == BACK).all())          # the back box is wider than the front one
    assert_frame(only, restate_frame(A, scene, [], [], [[BACK]], keep=[BACK]))
    moved = A.Ed.preview_frame(scene.lg, H, W, K, POSE, [shift_x(0.5)], [FRONT], keep_labels=[BACK], near=NEAR, far=FAR)
    assert_frame(moved, restate_frame(A, scene, [shift_x(0.5)], [FRONT], [[BACK], []], keep=[BACK]))
    assert torch.equal(moved["label"], only["label"])
    for out in (plain, only):
        hit = out["label"] != 255
        want = torch.zeros(H, W, 3, dtype=torch.uint8, device="cuda")
        want[hit] = lut[out["label"][hit].long()]
        assert out["ins_img"].dtype == torch.uint8 and torch.equal(out["ins_img"], want)
        assert bool((out["ins_img"][~hit] == 0).all()) and bool((out["ins_img"][hit] != 0).all())
    with pytest.raises(ValueError):
        A.Ed.preview_frame(scene.lg, H, W, K, POSE, [shift_x(0.5)], [], near=NEAR, far=FAR)
    with pytest.raises(ValueError):
        A.Ed.preview_frame(scene.lg, H, W, K, POSE, [shift_x(0.5)], [CS], near=NEAR, far=FAR)
    with pytest.raises(ValueError):
        A.Ed.preview_frame(scene.lg, H, W, K, POSE, near=NEAR, far=FAR, lut=lut[:CS - 1])


def test_preview_captured_in_a_graph_follows_the_labels(A, scene):
    first = scene.vol
    second = np.full_like(first, 255)
    second[2:14, 5:9, 8:11] = 6
    second[6:10, 6:10, 12:14] = FRONT
    lg = A.F.LabelGrid.from_labels(torch.from_numpy(first).cuda(), *BOX, CS)
    lut = torch.from_numpy(np.random.RandomState(4).randint(1, 256, size=(CS, 3)).astype(np.uint8)).cuda()
    call = lambda grid: A.Ed.preview_frame(grid, H, W, K, POSE, [shift_x(0.5)], [FRONT], near=NEAR, far=FAR, lut=lut)
    eager = [call(A.F.LabelGrid.from_labels(torch.from_numpy(v).cuda(), *BOX, CS)) for v in (first, second)]      # (also the warm-up)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(lg)
    assert not torch.equal(eager[0]["label"], eager[1]["label"])
    for vol, e in ((second, eager[1]), (first, eager[0])):
        lg.labels.copy_(torch.from_numpy(vol).cuda())                          # in place: the capture holds the pointer
        out["label"].fill_(77)
        graph.replay()
        torch.cuda.synchronize()
        for key in ("label", "source", "ins_img"):
            assert torch.equal(out[key], e[key]), key
        assert torch.equal(bits(out["depth"]), bits(e["depth"]))
