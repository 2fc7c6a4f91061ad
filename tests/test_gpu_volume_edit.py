"""GPU tests of ``dmnerf_volume_edit`` (csrc/volume_edit.hip) and ``editing.edit_volume``: the kernel against its numpy statement
(tests/_volume_edit_restate.py) bit for bit, the argument checks, the direction of the map against the ray-set previews, more edits
than the baked render takes ray sets, chaining, and graph capture.  Shapes: 7 x 5 x 9 (315 cells: less than two workgroups, a ragged
last wave), 19 x 17 x 23 (30 workgroups, each flushing its LDS table) and the 16^3 scenes of the CPU tests."""
import functools

import numpy as np
import pytest
import torch

import _baked_restate as B
import _gpu
import _label_trace_restate as T
import _volume_edit_restate as V
from _gpu import A  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32
BOX = ((-1.0, -0.8, -1.2), (1.1, 0.9, 1.3))                        # nothing dyadic: the f32 roundings matter
BOX16 = ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0))                      # cell 1.0: whole-cell moves are exact
DIMS16 = (16, 16, 16)
CS = 14


def make_grid(A, labels, cells, box, C):
    lab = torch.from_numpy(labels).cuda()
    if cells is None:
        return A.F.LabelGrid.from_labels(lab, *box, C)
    return A.F.BakedGrid.from_arrays(lab, torch.from_numpy(cells).cuda(), *box, C)


def as_trans(A, entries):
    """The restatement's entries as ``edit_volume`` takes them."""
    trans = [A.Ed.Remove() if k == V.REMOVE else A.Ed.Copy(m) if k == V.COPY else m for k, _, m in entries]
    return trans, [l for _, l, _ in entries]


def guarded_out(A, dims, baked, box, C):
    """A grid to write into that sits inside larger poisoned buffers -> ``(grid, check)``; ``check()`` asserts the cells around it are
    untouched."""
    n, pad = int(np.prod(dims)), 64
    lab = torch.full((n + 2 * pad,), 77, dtype=torch.uint8, device="cuda")
    cel = torch.full(((n + 2 * pad) * 4,), -7.0, dtype=torch.float32, device="cuda")
    labels = lab[pad:pad + n].reshape(dims)
    if baked:
        grid = A.F.BakedGrid.from_arrays(labels, cel[pad * 4:(pad + n) * 4].reshape(*dims, 4), *box, C)
    else:
        grid = A.F.LabelGrid.from_labels(labels, *box, C)

    def check():
        assert bool((lab[:pad] == 77).all()) and bool((lab[pad + n:] == 77).all())
        assert bool((cel[:pad * 4] == -7.0).all()) and bool((cel[(pad + n) * 4:] == -7.0).all())
        if not baked:
            assert bool((cel == -7.0).all())
    return grid, check


def assert_equals_restatement(res, want, baked, what):
    assert res["grid"].labels.dtype == torch.uint8 and torch.equal(res["grid"].labels.cpu(), torch.from_numpy(want["labels"])), what
    assert res["source"].dtype == torch.uint8 and torch.equal(res["source"].cpu(), torch.from_numpy(want["source"])), what
    if baked:
        assert torch.equal(res["grid"].cells.cpu().view(torch.int32), torch.from_numpy(want["cells"]).view(torch.int32)), what
    for k in ("won", "claimed", "hits"):
        assert res[k].dtype == torch.int64 and tuple(res[k].shape) == want[k].shape, (what, k)
        assert torch.equal(res[k].cpu(), torch.from_numpy(want[k])), (what, k, res[k].cpu(), want[k])


# ---- 1. bit-equality with the restatement
@pytest.mark.parametrize("C", [2, 14, 128])
@pytest.mark.parametrize("E", [0, 1, 3, 32])
@pytest.mark.parametrize("dims", [(7, 5, 9), (19, 17, 23)])
def test_kernel_equals_the_restatement(A, dims, E, C):
    lo, cell, inv_cell = V.grid_consts(*BOX, dims)
    labels, cells = V.random_volume(dims, C, seed=11 + E + C, baked=True)
    assert (labels == 255).any() and ((labels >= C) & (labels != 255)).any()
    entries = V.random_entries(E, C, seed=5 + E, lo=BOX[0], hi=BOX[1])
    if E >= 3:
        assert {k for k, _, _ in entries} == {V.MOVE, V.COPY, V.REMOVE} and len({l for _, l, _ in entries}) < E
    trans, targets = as_trans(A, entries)
    keep = None if C == 14 else sorted({0, C - 1} | set(range(0, C, 3)))
    words = V.mask_words(range(C) if keep is None else keep, C)
    for baked, rule in ((False, "first"), (True, "first"), (True, "densest")):
        want = V.edit(labels, cells if baked else None, lo, cell, inv_cell, C, words, entries, V_RULE[rule])
        grid = make_grid(A, labels, cells if baked else None, BOX, C)
        res = A.Ed.edit_volume(grid, trans, targets, keep_labels=keep, rule=rule)
        assert type(res["grid"]) is type(grid) and res["grid"].C == C and res["grid"].dims == grid.dims
        assert_equals_restatement(res, want, baked, (dims, E, C, baked, rule))
        assert int(res["won"].sum()) + int((res["grid"].labels == 255).sum()) == labels.size
        # a second, identical call -- into a guarded out= -- gives the same volume and the same counts
        out, check = guarded_out(A, dims, baked, BOX, C)
        again = A.Ed.edit_volume(grid, trans, targets, keep_labels=keep, rule=rule, out=out)
        assert again["grid"] is out
        assert_equals_restatement(again, want, baked, (dims, E, C, baked, rule, "out="))
        check()
        assert torch.equal(grid.labels.cpu(), torch.from_numpy(labels))           # the source is read only
        if E == 32:
            # every variant claims cells and collides, in several workgroups at 19 x 17 x 23: each one's LDS table of hits is flushed
            assert int(want["claimed"].sum()) > 0 and int(want["hits"].sum()) > 0 and int(res["hits"].sum()) > 0, (dims, C, baked, rule)
            assert (want["hits"].sum(axis=1) > 0).sum() >= 5 and (want["won"] > 0).sum() >= 5


V_RULE = {"first": 0, "densest": 1}


def test_entries_that_collide_count_as_the_restatement(A):
    """The random entries above seldom land two candidates on one cell; these do (the CPU tests hold the restatement's counts to a
    brute-force count on the same entries)."""
    labels, cells = V.scene()
    lo, cell, inv_cell = V.grid_consts(*BOX16, DIMS16)
    for entries in V.COLLISIONS:
        entries = V.shift_entries([(k, l, s if s is not None else (0, 0, 0)) for k, l, s in entries])
        trans, targets = as_trans(A, entries)
        for rule in ("first", "densest"):
            want = V.edit(labels, cells, lo, cell, inv_cell, CS, V.mask_words(range(CS), CS), entries, V_RULE[rule])
            assert want["hits"].any()
            res = A.Ed.edit_volume(make_grid(A, labels, cells, BOX16, CS), trans, targets, rule=rule)
            assert_equals_restatement(res, want, True, rule)


# ---- 2. no edits
@pytest.mark.parametrize("baked", [False, True])
def test_no_edits_and_no_keep_labels_give_back_the_input(A, baked):
    labels, cells = V.scene()
    grid = make_grid(A, labels, cells if baked else None, BOX16, CS)
    res = A.Ed.edit_volume(grid, [], [])
    assert res["grid"] is not grid and torch.equal(res["grid"].labels, grid.labels)
    if baked:
        assert torch.equal(res["grid"].cells.view(torch.int32), grid.cells.view(torch.int32))
    assert torch.equal(res["source"], torch.where(grid.labels != 255, 0, 255).to(torch.uint8))
    assert res["won"].tolist() == [int((labels != 255).sum())] and tuple(res["claimed"].shape) == (0,) and tuple(res["hits"].shape) == (0, CS)


# ---- 3. errors
def test_every_refusal_comes_before_the_device(A, monkeypatch):
    Ed = A.Ed
    labels, cells = V.scene()
    plain, baked = make_grid(A, labels, None, BOX16, CS), make_grid(A, labels, cells, BOX16, CS)
    out_p, check_p = guarded_out(A, DIMS16, False, BOX16, CS)
    out_b, check_b = guarded_out(A, DIMS16, True, BOX16, CS)
    out_p.labels.fill_(99)
    out_b.labels.fill_(99)
    out_b.cells.fill_(-3.0)
    launches = []
    real = A.L.launch
    monkeypatch.setattr(A.L, "launch", lambda *a: (launches.append(a[0]), real(*a))[1])
    eye = np.eye(4)
    for grid, out in ((plain, out_p), (baked, out_b)):
        bad = [(dict(trans_list=[Ed.Deform("sin")], target_labels=[3]), "image row"),
               (dict(trans_list=[eye, Ed.Copy(Ed.Deform("ln"))], target_labels=[3, 5]), "image row"),
               (dict(trans_list=[eye] * 33, target_labels=[3] * 33), "at most 32"),
               (dict(trans_list=[eye], target_labels=[CS]), "outside"),
               (dict(trans_list=[eye], target_labels=[-1]), "outside"),
               (dict(trans_list=[eye], target_labels=[3], keep_labels=[1, CS]), "outside"),
               (dict(trans_list=[eye, eye], target_labels=[3]), "target labels for"),
               (dict(trans_list=[eye], target_labels=[3], rule="largest"), "rule")]
        if grid is plain:
            bad.append((dict(trans_list=[eye], target_labels=[3], rule="densest"), "densest"))
        for kw, match in bad:
            with pytest.raises(ValueError, match=match):
                Ed.edit_volume(grid, out=out, **kw)
        # an out that is the source, that shares its memory, or that is another kind of volume
        alias = A.F.LabelGrid.from_labels(grid.labels, *BOX16, CS) if grid is plain else A.F.BakedGrid.from_arrays(out.labels, grid.cells, *BOX16, CS)
        for o in (grid, alias):
            with pytest.raises(ValueError, match="shares memory"):
                Ed.edit_volume(grid, [eye], [3], out=o)
        with pytest.raises(ValueError, match="out must be"):
            Ed.edit_volume(grid, [eye], [3], out=out_b if grid is plain else out_p)
        # an out with another C, another box, or that is no volume at all
        rewrap = lambda box, C: (A.F.LabelGrid.from_labels(out.labels, *box, C) if grid is plain
                                 else A.F.BakedGrid.from_arrays(out.labels, out.cells, *box, C))
        for o in (rewrap(BOX16, CS - 1), rewrap(((-8.0, -8.0, -8.0), (8.0, 8.0, 8.5)), CS), rewrap(((-8.5, -8.0, -8.0), (8.0, 8.0, 8.0)), CS),
                  {"grid": out}, out.labels):
            with pytest.raises(ValueError, match="out must be"):
                Ed.edit_volume(grid, [eye], [3], out=o)
    torch.cuda.synchronize()
    assert launches == []
    assert bool((out_p.labels == 99).all()) and bool((out_b.labels == 99).all()) and bool((out_b.cells == -3.0).all())
    check_p()
    check_b()
    assert torch.equal(plain.labels.cpu(), torch.from_numpy(labels))
    # a CPU tensor: the error every entry of the package raises
    host = A.F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), *BOX16, CS)
    host.labels = host.labels.cpu()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Ed.edit_volume(host, [eye], [3])
    assert launches == []
    Ed.edit_volume(plain, [eye], [3], out=out_p)                                 # (the counter does count)
    assert launches == ["dmnerf_volume_edit"]


# ---- 4. the direction of the map, against the ray sets
H, W = 24, 32
K = np.array([[40.0, 0, 16.0], [0, 40.0, 12.0], [0, 0, 1.0]])
POSE = np.array([[1.0, 0, 0, 0.25], [0, -1, 0, -0.5], [0, 0, -1, 20.0], [0, 0, 0, 1]], dtype=np.float32)      # a dyadic origin above the box
NEAR, FAR = 0.0, 64.0
OBJECT, STEP = 3, (3, -2, 1)                                       # the object goes STEP cells further: the map reads destination - STEP
MOVE = V.translation([-3.0, 2.0, -1.0])


renderer_rays = functools.partial(_gpu.renderer_rays, camera=(H, W, K, POSE), ins_num=CS - 1)


def cell_ijk(g):
    g = np.asarray(g, dtype=np.int64)
    return np.stack([g // 256, (g // 16) % 16, g % 16], axis=-1)


def test_direction_label_volume_against_the_ray_sets(A):
    """One whole-cell MOVE into free space: ``preview_frame`` with the move on the ORIGINAL volume (two ray sets) and without edits on
    the EDITED volume (one ray set) see the same frame.  With ``trans`` and its inverse swapped the object would go the other way.
    Both routes are first run through tests/_label_trace_restate.py on the host: they agree on every pixel for this pose."""
    labels, _ = V.scene()
    lo, cell, inv_cell = V.grid_consts(*BOX16, DIMS16)
    grid = make_grid(A, labels, None, BOX16, CS)
    res = A.Ed.edit_volume(grid, [MOVE], [OBJECT])
    edited = res["grid"]
    assert not bool(res["hits"].any()) and int(res["claimed"][0]) == int(grid.stats()["count"][OBJECT]) == int((labels == OBJECT).sum())
    assert int(edited.stats()["count"][OBJECT]) == int((labels == OBJECT).sum())
    want = V.edit(labels, None, lo, cell, inv_cell, CS, V.mask_words(range(CS), CS), [(V.MOVE, OBJECT, MOVE)])
    assert torch.equal(edited.labels.cpu(), torch.from_numpy(want["labels"]))
    others = sorted(set(range(CS)) - {OBJECT})
    # on the host
    rays = renderer_rays(A, [MOVE], [OBJECT]).cpu().numpy()
    a = T.trace_sets(labels, lo, cell, inv_cell, CS, rays, [T.mask_words(others, CS), T.mask_words([OBJECT], CS)], f32(NEAR), f32(FAR))
    b = T.trace_sets(want["labels"], lo, cell, inv_cell, CS, rays[:1], [T.mask_words(range(CS), CS)], f32(NEAR), f32(FAR))
    shifted = lambda cells, source: np.where((source == 1)[:, None], cell_ijk(cells) + np.asarray(STEP), cell_ijk(cells))
    assert np.array_equal(a[0], b[0]) and np.array_equal(np.isfinite(a[1]), np.isfinite(b[1]))
    hit = a[0] != 255
    assert (a[0] == OBJECT).sum() > 10 and (a[3][a[0] == OBJECT] == 1).all() and len(set(a[0][hit])) >= 3
    assert np.array_equal(shifted(a[2], a[3])[hit], cell_ijk(b[2])[hit])
    # on the device
    pa = A.Ed.preview_frame(grid, H, W, K, POSE, [MOVE], [OBJECT], near=NEAR, far=FAR)
    pb = A.Ed.preview_frame(edited, H, W, K, POSE, near=NEAR, far=FAR)
    assert torch.equal(pa["label"], pb["label"]) and torch.equal(pa["label"].cpu().reshape(-1), torch.from_numpy(a[0]))
    assert torch.equal(torch.isfinite(pa["depth"]), torch.isfinite(pb["depth"])) and torch.equal(torch.isfinite(pa["depth"]), pa["label"] != 255)
    ta = grid.trace_sets(renderer_rays(A, [MOVE], [OBJECT]), [others, [OBJECT]], NEAR, FAR)
    tb = edited.trace_sets(renderer_rays(A, [], []), [range(CS)], NEAR, FAR)
    dev_hit = (ta["label"] != 255).cpu().numpy()
    assert np.array_equal(dev_hit, hit)
    assert np.array_equal(shifted(ta["cell"].cpu().numpy(), ta["source"].cpu().numpy())[hit], cell_ijk(tb["cell"].cpu().numpy())[hit])


def test_direction_baked_volume_against_the_ray_sets(A):
    """The same comparison with colour: ``render_preview`` of the move on the original volume (R = 2) and of the edited volume (R = 1).
    ``nseg`` and ``label`` are equal on every pixel; ``rgb``, ``depth``, ``acc`` within 4 x the largest deviation between the two routes
    in tests/_baked_restate.py on the host.  Measured on the host for this input: 0 for all three -- the two routes composite the same
    segments with the same ``t`` (origin and move are dyadic), so the bound is exact equality."""
    labels, cells = V.scene()
    cells[..., 3] = np.where(labels != 255, np.random.RandomState(2).uniform(0.2, 1.5, size=labels.shape), 0.0)        # soft: several cells share a pixel
    lo, cell, inv_cell = V.grid_consts(*BOX16, DIMS16)
    grid = make_grid(A, labels, cells, BOX16, CS)
    res = A.Ed.edit_volume(grid, [MOVE], [OBJECT])
    want = V.edit(labels, cells, lo, cell, inv_cell, CS, V.mask_words(range(CS), CS), [(V.MOVE, OBJECT, MOVE)])
    assert_equals_restatement(res, want, True, "move")
    assert not bool(res["hits"].any()) and int(res["claimed"][0]) == int(grid.stats()["count"][OBJECT])
    others = sorted(set(range(CS)) - {OBJECT})
    rays = renderer_rays(A, [MOVE], [OBJECT]).cpu().numpy()
    a = B.render(labels, cells, lo, cell, inv_cell, CS, rays, [T.mask_words(others, CS), T.mask_words([OBJECT], CS)], NEAR, FAR)
    b = B.render(want["labels"], want["cells"], lo, cell, inv_cell, CS, rays[:1], [T.mask_words(range(CS), CS)], NEAR, FAR)
    assert np.array_equal(a["nseg"], b["nseg"]) and np.array_equal(a["label"], b["label"]) and int(a["nseg"].max()) >= 3
    assert (a["label"] == OBJECT).sum() > 10
    bound = {k: 4.0 * float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()) for k in ("rgb", "depth", "acc")}
    pa = A.Ed.render_preview(grid, H, W, K, POSE, [MOVE], [OBJECT], near=NEAR, far=FAR)
    pb = A.Ed.render_preview(res["grid"], H, W, K, POSE, near=NEAR, far=FAR)
    assert torch.equal(pa["nseg"], pb["nseg"]) and torch.equal(pa["label"], pb["label"])
    assert torch.equal(pa["nseg"].cpu().reshape(-1), torch.from_numpy(a["nseg"]))
    worst = {k: float((pa[k].double() - pb[k].double()).abs().max()) for k in bound}
    print("host deviation x 4:", bound, "device:", worst)
    for k in bound:
        assert worst[k] <= bound[k], (k, worst[k], bound[k])


# ---- 5. more edits than the baked render takes ray sets
def test_four_moves_at_once_render_as_one_ray_set(A):
    labels, cells = V.scene()
    cells[..., 3] = np.where(labels != 255, np.random.RandomState(3).uniform(0.2, 1.5, size=labels.shape), 0.0)
    lo, cell, inv_cell = V.grid_consts(*BOX16, DIMS16)
    moves = [V.translation([-2.0, 0.0, 0.0]), V.translation([0.0, 2.0, 1.0]), V.translation([1.0, 1.0, -2.0]),
             A.Ed.about(V.rotation([0.0, 0.0, 1.0], 0.4), [-5.0, 3.5, 3.0])]
    targets = [1, 3, 5, 7]
    grid = make_grid(A, labels, cells, BOX16, CS)
    with pytest.raises(ValueError, match="at most 3"):
        A.Ed.render_preview(grid, H, W, K, POSE, moves, targets, near=NEAR, far=FAR)
    res = A.Ed.edit_volume(grid, moves, targets)
    entries = [(V.MOVE, l, m) for l, m in zip(targets, moves)]
    want = V.edit(labels, cells, lo, cell, inv_cell, CS, V.mask_words(range(CS), CS), entries)
    assert_equals_restatement(res, want, True, "four moves")
    assert (want["claimed"] > 0).all() and not np.array_equal(want["labels"], labels)
    got = A.Ed.render_preview(res["grid"], H, W, K, POSE, near=NEAR, far=FAR)
    rays = renderer_rays(A, [], []).cpu().numpy()
    masks = [T.mask_words(range(CS), CS)]
    seg = B.merge(want["labels"], lo, cell, inv_cell, CS, rays, masks, NEAR, FAR)
    r32 = B.render(want["labels"], want["cells"], lo, cell, inv_cell, CS, rays, masks, NEAR, FAR, seg=seg)
    r64 = B.referee(want["labels"], want["cells"], lo, cell, inv_cell, CS, rays, masks, NEAR, FAR, seg=seg)
    bound = B.bounds(r32, r64)
    assert np.array_equal(got["nseg"].cpu().numpy().reshape(-1), r32["nseg"]) and set(np.unique(r32["label"])) >= {1, 3, 5, 7}
    for k in bound:
        worst = float(np.abs(got[k].cpu().numpy().reshape(r64[k].shape).astype(np.float64) - r64[k]).max())
        assert worst <= bound[k], (k, worst, bound[k])
    unsure = B.ambiguous(r64, bound["acc"])
    assert unsure.mean() <= 0.01
    assert np.array_equal(got["label"].cpu().numpy().reshape(-1)[~unsure], r32["label"][~unsure])


# ---- 6. chaining
@pytest.mark.parametrize("baked", [False, True])
def test_a_move_and_its_inverse_give_back_the_volume(A, baked):
    labels, cells = V.scene()
    grid = make_grid(A, labels, cells if baked else None, BOX16, CS)
    there = A.Ed.edit_volume(grid, [MOVE, A.Ed.Copy(V.translation([0.0, 0.0, 4.0]))], [OBJECT, 1])
    assert not torch.equal(there["grid"].labels, grid.labels)
    back = A.Ed.edit_volume(there["grid"], [V.translation([3.0, -2.0, 1.0])], [OBJECT])
    copy = torch.from_numpy(np.roll(labels == 1, -4, axis=2)).cuda()              # the copy of object 1 stays where the first edit put it
    assert int(copy.sum()) == int((labels == 1).sum())
    assert torch.equal(back["grid"].labels[~copy], grid.labels[~copy]) and bool((back["grid"].labels[copy] == 1).all())
    assert int(back["claimed"][0]) == int((labels == OBJECT).sum()) and not bool(back["hits"].any())
    if baked:
        assert torch.equal(back["grid"].cells[~copy].view(torch.int32), grid.cells[~copy].view(torch.int32))
    stats, first = back["grid"].stats(), grid.stats()
    assert torch.equal(stats["count"][OBJECT], first["count"][OBJECT]) and torch.equal(stats["lo_idx"][OBJECT], first["lo_idx"][OBJECT])
    assert int(back["grid"].skip_grid([OBJECT]).unpack().sum()) == int((labels == OBJECT).sum())


# ---- 7. graph capture
def test_captured_edit_follows_the_source_volume(A):
    labels, cells = V.scene()
    second, cells2 = np.roll(labels, 2, axis=1).copy(), np.roll(cells, 2, axis=1).copy()
    trans, targets = [MOVE, A.Ed.Copy(V.translation([0.0, 0.0, 4.0])), A.Ed.Remove()], [OBJECT, 1, 7]
    call = lambda g, **kw: A.Ed.edit_volume(g, trans, targets, rule="densest", **kw)
    eager = [call(make_grid(A, l, c, BOX16, CS)) for l, c in ((labels, cells), (second, cells2))]         # (also the warm-up)
    assert not torch.equal(eager[0]["grid"].labels, eager[1]["grid"].labels)
    live = make_grid(A, labels, cells, BOX16, CS)
    res = call(live)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(live, out=res["grid"])
    assert out["grid"] is res["grid"]
    for (l, c), e in (((second, cells2), eager[1]), ((labels, cells), eager[0])):
        live.labels.copy_(torch.from_numpy(l).cuda())                           # in place: the capture holds the pointers
        live.cells.copy_(torch.from_numpy(c).cuda())
        out["grid"].labels.fill_(77)
        out["source"].fill_(77)
        out["won"].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["grid"].labels, e["grid"].labels) and torch.equal(out["source"], e["source"])
        assert torch.equal(out["grid"].cells.view(torch.int32), e["grid"].cells.view(torch.int32))
        for k in ("won", "claimed", "hits"):
            assert torch.equal(out[k], e[k]), k
