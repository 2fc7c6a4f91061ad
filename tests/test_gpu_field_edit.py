"""GPU tests of the field-edit route: ``dmnerf_field_edit_select`` / ``dmnerf_field_edit_filter`` (csrc/field_edit.hip) against their numpy
statement (tests/_field_edit_restate.py) bit for bit, ``render.run_network_edited`` against the dense and the skip route where it
reduces to them, ``manipulator.edited_field`` against the chain written out, the ``field_edit=`` frame for two world sizes, and graph
capture.  Every comparison is ``torch.equal``; there is no tolerance anywhere.

Shapes: (N, S) = (37, 7) is 259 samples -- two 256-row blocks with a ragged tail -- and (1031, 64) is 65 984 samples, 258 blocks."""
import ctypes
import types

import numpy as np
import pytest
import torch

import _field_edit_restate as R
import _gpu
import _volume_edit_restate as V
from _gpu import A  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

f32 = np.float32
INS = 13
C14 = INS + 1


_models = {}


def models():
    return _gpu.models(INS, cache=_models)


def as_trans(A, entries):
    trans = [A.Ed.Remove() if k == V.REMOVE else A.Ed.Copy(m) if k == V.COPY else m for k, _, m in entries]
    return trans, [l for _, l, _ in entries]


def bits(t):
    return t.contiguous().view(torch.int32)


def c_entries(A, entries):
    E = len(entries)
    arr = (A.L.VolumeEditEntry * E)() if E else None
    for e, (k, l, m) in enumerate(entries):
        arr[e].kind, arr[e].label = k, l
        if k != V.REMOVE:
            arr[e].m[:] = [float(v) for v in V.matrix_f32(m).reshape(-1)]
    return arr


def run_select(A, src, lo, inv_cell, entries, o, d, z, C, outside, unowned, totals=None):
    """The entry itself on poisoned buffers -> a dict of device tensors."""
    N, S = z.shape
    M = N * S
    dev = "cuda"
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    t = {"owner": torch.full((M,), 77, dtype=torch.uint8, device=dev), "o_w": torch.full((M, 3), -7.0, device=dev),
         "d_w": torch.full((M, 3), -7.0, device=dev), "sel": torch.full((M,), -1, dtype=torch.int32, device=dev),
         "count": torch.full((1,), -1, dtype=torch.int32, device=dev), "rows": torch.full((M, 4 + C), 7.0, device=dev)}
    work = torch.empty(int(A.lib.dmnerf_skip_select_work_ints(M)), dtype=torch.int32, device=dev)
    fill = torch.from_numpy(R.empty_row(C)).cuda()
    A.L.launch("dmnerf_field_edit_select", torch.from_numpy(src).cuda(), f3(lo), f3(inv_cell), (ctypes.c_int * 3)(*src.shape), outside, unowned,
                 c_entries(A, entries), len(entries), C, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(z).cuda(), N, S,
                 t["owner"], t["o_w"], t["d_w"], t["sel"], t["count"], work, t["rows"], fill, totals)
    torch.cuda.synchronize()
    return t


# ---- 1. select against the restatement
@pytest.mark.parametrize("E", [0, 1, 3, 32])
@pytest.mark.parametrize("dims", [(7, 5, 9), (19, 17, 23)])
@pytest.mark.parametrize("NS", [(37, 7), (1031, 64)])
def test_select_equals_the_restatement(A, NS, dims, E):
    lo, cell, inv_cell = V.grid_consts(*R.BOX, dims)
    entries = V.random_entries(E, C14, seed=5 + E, lo=R.BOX[0], hi=R.BOX[1])
    if E >= 3:
        assert {k for k, _, _ in entries} == {V.MOVE, V.COPY, V.REMOVE}
    src = R.random_source(dims, E, seed=3 + E)
    o, d, z = R.random_rays(*NS, seed=9)
    totals = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
    for outside, unowned in ((R.EVALUATE, R.EMPTY), (R.EMPTY, R.EVALUATE)):
        rows = np.full((NS[0] * NS[1], 4 + C14), 7.0, dtype=f32)
        want = R.select(src, lo, inv_cell, entries, o, d, z, outside=outside, unowned=unowned, rows=rows, fill_row=R.empty_row(C14))
        assert 0 < want["count"] < rows.shape[0]
        got = run_select(A, src, lo, inv_cell, entries, o, d, z, C14, outside, unowned, totals=totals)
        assert torch.equal(got["owner"].cpu(), torch.from_numpy(want["owner"]))
        n = int(got["count"].item())
        assert n == want["count"] and torch.equal(got["sel"][:n].cpu(), torch.from_numpy(want["sel"]))
        assert bool((got["sel"][n:] == -1).all())                   # nothing past the count
        ev = torch.from_numpy(want["owner"] != 255)
        for k in ("o_w", "d_w"):
            assert torch.equal(bits(got[k].cpu()[ev]), bits(torch.from_numpy(want[k])[ev])), k
            assert bool((got[k].cpu()[~ev] == -7.0).all()), k        # written for evaluated samples only
        assert torch.equal(got["rows"].cpu(), torch.from_numpy(want["rows"]))
    assert totals.tolist()[1] == 7 + 2 * NS[0] * NS[1] and totals.tolist()[0] > 5


# ---- 2. filter against the restatement applied to the device's own raw
@pytest.mark.parametrize("C", [2, 14, 128])
def test_filter_equals_the_restatement(A, C):
    E, M = 3, 259 + 256 * 3
    rng = np.random.RandomState(C)
    entries = [(V.MOVE, C - 1, None), (V.COPY, 0, None), (V.REMOVE, 1 % C, None)]
    masks = R.accept_masks(C, entries, keep=None if C != 14 else [0, 1, 5, 7, 13])
    raw = rng.randn(M, 4 + C).astype(f32)
    raw[::7, 4:] = 1.5                                              # ties
    raw[3::11, 4] = np.nan
    raw[5::13, 4 + C - 1] = np.nan
    owner = rng.choice(np.array([0, 1, 2, 3, 255], dtype=np.uint8), size=M)
    d_raw = torch.from_numpy(raw).cuda()
    kept = torch.full((1 + E,), -9, dtype=torch.int64, device="cuda")
    words = (ctypes.c_uint32 * (4 * (1 + E)))(*[int(w) for w in masks.reshape(-1)])
    fill = torch.from_numpy(R.empty_row(C)).cuda()
    pad = torch.full((M + 2, 4 + C), 3.0, device="cuda")            # the rows sit inside a poisoned buffer
    pad[1:M + 1] = d_raw
    A.L.launch("dmnerf_field_edit_filter", pad[1:M + 1], torch.from_numpy(owner).cuda(), M, C, words, E, fill, kept)
    want, want_kept = R.filter_rows(raw, owner, masks, R.empty_row(C))
    assert torch.equal(bits(pad[1:M + 1].cpu()), bits(torch.from_numpy(want)))
    assert bool((pad[0] == 3.0).all()) and bool((pad[M + 1] == 3.0).all())
    assert kept.tolist() == want_kept.tolist() and 0 < want_kept[0] and want_kept[3] == 0
    A.L.launch("dmnerf_field_edit_filter", pad[1:M + 1], torch.from_numpy(owner).cuda(), M, C, words, E, fill, None)     # no kept: legal


def test_entries_refuse_bad_arguments(A):
    lib = A.lib
    f3, i3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int * 3)(4, 4, 4)
    one, ow, dw, rows, fill = (torch.zeros(64, device="cuda") for _ in range(5))
    b = torch.zeros(64, dtype=torch.uint8, device="cuda")
    i, sel, work = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(3))
    owner = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    ent = c_entries(A, [(V.MOVE, 3, V.translation([0, 0, 0]))])

    def select(dims=i3, outside=0, unowned=0, entries=ent, E=1, C=14, N=1, S=4, source=b, count=i):
        return lib.dmnerf_field_edit_select(p(source) if source is not None else None, f3, f3, dims, outside, unowned, entries, E, C, p(one), p(one),
                                            p(one), N, S, p(owner), p(ow), p(dw), p(sel), p(count) if count is not None else None, p(work), None, None,
                                            None, None)
    assert select() == 0
    assert select(N=0, source=None) == 0                            # no sample: no launch, the pointers are not looked at
    for kw in (dict(dims=(ctypes.c_int * 3)(4, 0, 4)), dict(dims=(ctypes.c_int * 3)(2048, 2048, 512)), dict(outside=2), dict(unowned=-1),
               dict(E=33), dict(E=-1), dict(entries=None), dict(C=0), dict(C=129), dict(C=3), dict(N=-1), dict(S=0), dict(N=2 ** 29, S=4),
               dict(source=None), dict(count=None), dict(entries=c_entries(A, [(3, 3, V.translation([0, 0, 0]))]))):
        assert select(**kw) == -1, kw
    w = (ctypes.c_uint32 * 8)()
    flt = lambda raw=rows, M=4, C=4, masks=w, E=1: lib.dmnerf_field_edit_filter(p(raw) if raw is not None else None, p(b), M, C, masks, E, p(fill), None, None)
    assert flt() == 0 and flt(M=0, raw=None) == 0
    for kw in (dict(raw=None), dict(M=-1), dict(M=2 ** 31), dict(C=0), dict(C=129), dict(masks=None), dict(E=33), dict(E=-1)):
        assert flt(**kw) == -1, kw
    torch.cuda.synchronize()


# ---- 3. run_network_edited where it reduces to the routes that exist
def field_case(N=37, S=7, seed=9):
    o, d, z = R.random_rays(N, S, seed=seed, nan_rays=False)
    return torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), torch.from_numpy(z).cuda()


@pytest.mark.parametrize("split", [None, "f16x2"])
def test_identity_edit_equals_run_network(A, split):
    mc, _ = models()
    o, d, z = field_case()
    src = torch.zeros(7, 5, 9, dtype=torch.uint8, device="cuda")
    edit = A.Ed.FieldEdit.from_source(src, *R.BOX, [], [], C=C14)
    with torch.no_grad():
        got = A.R.run_network_edited(mc, o, d, z, edit, split=split)
        want = A.R.run_network(mc, o, d, z, split=split)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("split", [None, "f16x2"])
def test_no_edit_with_empty_policies_equals_the_skip_route(A, split):
    mc, _ = models()
    o, d, z = field_case()
    labels, _ = V.random_volume((7, 5, 9), C14, seed=4)
    grid = A.F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), *R.BOX, C14)
    edit = A.Ed.FieldEdit.from_volume(grid, [], [], outside="empty", unowned="empty")
    assert torch.equal(edit.source, edit.volume["source"]) and edit.E == 0
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        got = A.R.run_network_edited(mc, o, d, z, edit, split=split, counts=counts)
        want = A.R.run_network_skip(mc, o, d, z, grid.skip_grid(range(C14), outside="empty"), split=split)
    assert torch.equal(bits(got), bits(want))
    n_eval, n_all = counts.tolist()
    assert n_all == 37 * 7 and 0 < n_eval < n_all


@pytest.mark.parametrize("S", [7, 64])
def test_one_rigid_move_evaluates_each_sample_once_on_the_carried_ray(A, S):
    mc, _ = models()
    o, d, z = field_case(S=S)
    dims = (7, 5, 9)
    move = V.translation([0.3, 0.0, 0.0]) @ V.rotation([0.2, 1.0, 0.1], 0.4)
    src = R.random_source(dims, 1, seed=12)
    edit = A.Ed.FieldEdit.from_source(torch.from_numpy(src).cuda(), *R.BOX, [move], [2], C=C14, unowned="empty")
    st = {}
    with torch.no_grad():
        out = A.R.run_network_edited(mc, o, d, z, edit, _stages=st)
        owner = st["owner"]
        ev = owner != 255
        assert {0, 1, 255} <= set(owner.cpu().tolist())
        # dense, on the select's own rays (rows nobody evaluates get a finite stand-in ray: they are not compared)
        o_w = torch.where(ev[:, None], st["o_w"], o[:1].expand(owner.shape[0], 3)).contiguous()
        d_w = torch.where(ev[:, None], st["d_w"], d[:1].expand(owner.shape[0], 3)).contiguous()
        dense = A.R.run_network(mc, o_w, d_w, z.reshape(-1, 1).contiguous()).reshape(-1, 4 + C14)
    raw_net = st["raw_net"].reshape(-1, 4 + C14)
    assert torch.equal(bits(raw_net[ev]), bits(dense[ev]))
    empty = torch.from_numpy(R.empty_row(C14)).cuda()
    assert bool((raw_net[~ev] == empty).all()) and bool((out.reshape(-1, 4 + C14)[~ev] == empty).all())
    # the restatement agrees on who owns what and where it is asked, and the filter on the device's own rows
    lo, cell, inv_cell = V.grid_consts(*R.BOX, dims)
    want = R.select(src, lo, inv_cell, [(V.MOVE, 2, move)], o.cpu().numpy(), d.cpu().numpy(), z.cpu().numpy(), unowned=R.EMPTY)
    assert torch.equal(owner.cpu(), torch.from_numpy(want["owner"]))
    evc = ev.cpu()
    assert torch.equal(bits(st["o_w"].cpu()[evc]), bits(torch.from_numpy(want["o_w"])[evc]))
    assert torch.equal(bits(st["d_w"].cpu()[evc]), bits(torch.from_numpy(want["d_w"])[evc]))
    filt, kept = R.filter_rows(raw_net.cpu().numpy(), want["owner"], np.asarray(list(edit.masks), dtype=np.uint32), R.empty_row(C14))
    assert torch.equal(bits(out.reshape(-1, 4 + C14).cpu()), bits(torch.from_numpy(filt)))
    assert st["kept"].tolist() == kept.tolist()


def test_field_edit_hands_the_kernels_the_restated_masks_and_entries(A):
    """What ``FieldEdit`` builds on the host, held against the restatement's own packing: MOVE, COPY and REMOVE entries, with and
    without a keep set (the filter test feeds the kernel ``R.accept_masks``; this ties the product's masks to the same words)."""
    rot = V.translation([0.3, 0.1, 0.0]) @ V.rotation([0.2, 1.0, 0.1], 0.4)
    entries = [(V.MOVE, 0, rot), (V.COPY, 1, V.translation([-0.3, 0.0, 0.2])), (V.REMOVE, 6, None), (V.COPY, 0, V.translation([0.1, 0.0, 0.0])),
               (V.MOVE, 9, np.diag([1.5, 0.75, 1.25, 1.0]))]
    trans, targets = as_trans(A, entries)
    src = torch.zeros(7, 5, 9, dtype=torch.uint8, device="cuda")
    for keep in (None, [0, 1, 5, 9, 13], [1, 6]):
        edit = A.Ed.FieldEdit.from_source(src, *R.BOX, trans, targets, C=C14, keep_labels=keep)
        assert list(edit.masks) == R.accept_masks(C14, entries, keep).ravel().tolist(), keep
        want = c_entries(A, entries)
        assert edit.E == 5 and edit.kinds == [k for k, _, _ in entries]
        for e in range(5):
            assert (edit.entries[e].kind, edit.entries[e].label) == (want[e].kind, want[e].label), e
            assert list(edit.entries[e].m) == list(want[e].m), e
    labels, _ = V.random_volume((7, 5, 9), C14, seed=4)
    grid = A.F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), *R.BOX, C14)
    edit = A.Ed.FieldEdit.from_volume(grid, trans, targets, keep_labels=[0, 1, 5, 9, 13])
    assert list(edit.masks) == R.accept_masks(C14, entries, [0, 1, 5, 9, 13]).ravel().tolist()
    lo, cell, inv_cell = V.grid_consts(*R.BOX, (7, 5, 9))
    vol = V.edit(labels, None, lo, cell, inv_cell, C14, V.mask_words([0, 1, 5, 9, 13], C14), entries, 0)
    assert torch.equal(edit.source.cpu(), torch.from_numpy(vol["source"]))


def test_refusals_of_the_python_route(A):
    mc, _ = models()
    o, d, z = field_case()
    src = torch.zeros(7, 5, 9, dtype=torch.uint8, device="cuda")
    edit = A.Ed.FieldEdit.from_source(src, *R.BOX, [], [], C=C14)
    with pytest.raises(ValueError, match="bf16x3"):
        A.R.run_network_edited(mc, o, d, z, edit, split="bf16x3")
    narrow = A.M.DM_NeRF(4, 64, 63, 27, [2], INS).cuda().eval()
    with pytest.raises(ValueError, match="8 x 256"):
        A.R.run_network_edited(narrow, o, d, z, edit)
    with pytest.raises(TypeError):
        A.R.run_network_edited(mc, o, d, z, None)
    with pytest.raises(ValueError, match="C = 128"):
        A.R.run_network_edited(mc, o, d, z, A.Ed.FieldEdit.from_source(src, *R.BOX, [], []))
    with pytest.raises(ValueError, match="Deform|deformation"):
        A.Ed.FieldEdit.from_source(src, *R.BOX, [A.Ed.Deform("sin", 0)], [2], C=C14)
    with pytest.raises(ValueError, match="outside"):
        A.Ed.FieldEdit.from_source(src, *R.BOX, [], [], C=C14, outside="maybe")
    assert tuple(A.R.run_network_edited(mc, o[:0], d[:0], z[:0], edit).shape) == (0, 7, 4 + C14)


# ---- 4. the chain, the frame, capture
NEAR, FAR = 0.0, 2.5


def chain_args(split=None, chunk=64):
    a = types.SimpleNamespace(N_samples=8, N_importance=8, near=NEAR, far=FAR, N_test=chunk, target_labels=[])
    if split:
        a.mfma_split = split
    return a


def moved_edit(A, seed=12, **kw):
    dims = (7, 5, 9)
    labels, _ = V.random_volume(dims, C14, seed=seed, empty=0.3)
    grid = A.F.LabelGrid.from_labels(torch.from_numpy(labels).cuda(), *R.BOX, C14)
    trans = [V.translation([0.3, 0.1, 0.0]) @ V.rotation([0.2, 1.0, 0.1], 0.4), A.Ed.Copy(V.translation([-0.3, 0.0, 0.2])), A.Ed.Remove()]
    return A.Ed.FieldEdit.from_volume(grid, trans, [0, 1, 6], **kw), grid, trans


@pytest.mark.parametrize("split", [None, "f16x2"])
def test_edited_field_equals_the_chain_written_out(A, split):
    mc, mf = models()
    o, d, _ = field_case()
    args = chain_args(split)
    edit, _, _ = moved_edit(A)
    u = torch.rand(37, 8, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        rgb, ins, depth = A.MA.edited_field(mc, mf, torch.stack([o, d]), args, edit, u=u)
        z = A.MA.manipulator_z(37, NEAR, FAR, 8, "cuda")
        raw = A.R.run_network_edited(mc, o, d, z, edit, split=split)
        _, w, _, _ = A.MA.manipulator_render(raw, z, d)
        z_full = A.H.importance_resample(z, w, 8, u=u)
        raw = A.R.run_network_edited(mf, o, d, z_full, edit, split=split)
        w_rgb, _, w_depth, w_ins = A.MA.manipulator_render(raw, z_full, d)
    assert tuple(rgb.shape) == (37, 3) and tuple(ins.shape) == (37, C14) and tuple(depth.shape) == (37,)
    assert torch.equal(bits(rgb), bits(w_rgb)) and torch.equal(bits(ins), bits(w_ins)) and torch.equal(bits(depth), bits(w_depth))
    assert bool(torch.isfinite(rgb).all()) and float(rgb.abs().max()) > 0


def test_frame_is_the_same_for_world_1_and_the_bands_of_world_3(A):
    H, W, chunk = 12, 16, 64
    mc, mf = models()
    K = np.array([[20.0, 0, W / 2], [0, -20.0, H / 2], [0, 0, -1]])
    pose = O.pose_spherical(30.0, -65.0, 1.6).cuda()
    args = types.SimpleNamespace(N_samples=8, N_importance=8, near=0.3, far=3.0, N_test=chunk, target_labels=[])
    edit, grid, trans = moved_edit(A)
    kw = dict(field_edit=edit)
    with torch.no_grad():
        torch.manual_seed(5)
        fr = A.D.ManipulationFrameRenderer(H, W, K, pose, [], (mc, mf), args, rank=0, world=1, **kw)
        assert fr.T == 0
        for c in range(fr.n_chunks):
            fr.step(c)
        whole = [t.clone() for t in fr.gather()]
        n_eval = fr.n_eval.tolist()
        bands = []
        for r in range(3):
            torch.manual_seed(5)
            br = A.D.ManipulationFrameRenderer(H, W, K, pose, [], (mc, mf), args, rank=r, world=3, **kw)
            for c in range(br.n_chunks):
                br.step(c)
            bands.append([t.clone() for t in br.gather()])
        torch.manual_seed(5)
        again = A.D.manipulate_frame(H, W, K, pose, [], (mc, mf), args, **kw)
    for i in range(4):
        assert torch.equal(bits(whole[i]), bits(torch.cat([b[i] for b in bands], dim=0))), i
        assert torch.equal(bits(whole[i]), bits(again[i])), i
    assert tuple(whole[0].shape) == (H, W, 3) and tuple(whole[1].shape) == (H, W, C14)
    assert not whole[2].any() and not whole[3].any()                # no target side: zeros
    assert n_eval[1] == H * W * (8 + 16) and 0 < n_eval[0] <= n_eval[1]
    assert float(whole[0].abs().max()) > 0
    # the demo path: one view, the same frame and its products
    with torch.no_grad():
        torch.manual_seed(5)
        rgbs = np.random.RandomState(0).randint(0, 255, size=(C14 + 1, 3)).astype(np.uint8)
        demo = A.Ed.manipulate_demo_path([pose], (H, W, K), (mc, mf), args, [], {}, rgbs, {str(l): l for l in range(C14)},
                                         {str(l): l for l in range(C14)}, keep_maps=True, field_edit=edit)
    assert torch.equal(bits(demo["rgb"][0]), bits(whole[0])) and torch.equal(bits(demo["ins"][0]), bits(whole[1]))
    assert tuple(demo["rgb8"].shape) == (1, H, W, 3) and tuple(demo["label"].shape) == (1, H, W) and demo["label"].dtype == torch.int64
    for bad in (dict(keep_labels=[1]), dict(skip=grid.skip_grid(range(C14)))):
        with pytest.raises(ValueError, match="cannot be combined"):
            A.Ed.manipulate_demo_path([pose], (H, W, K), (mc, mf), args, [], {}, rgbs, {}, {}, field_edit=edit, **bad)
    with pytest.raises(ValueError, match="objs must be empty"):
        A.Ed.manipulate_demo_path([pose], (H, W, K), (mc, mf), args, [{"tar_id": 1}], {}, rgbs, {}, {}, field_edit=edit)
    with pytest.raises(ValueError, match="trans_list must be empty"):
        A.D.ManipulationFrameRenderer(H, W, K, pose, trans[:1], (mc, mf), args, **kw)
    for bad in (dict(skip=grid.skip_grid(range(C14))), dict(manipulate_chunk=lambda *a: None), dict(keep_labels=[1])):
        with pytest.raises(ValueError, match="cannot be combined"):
            A.D.ManipulationFrameRenderer(H, W, K, pose, [], (mc, mf), args, **kw, **bad)


def test_captured_chunk_follows_the_source_overwritten_in_place(A):
    mc, mf = models()
    o, d, _ = field_case()
    rays = torch.stack([o, d])
    args = chain_args()
    edit_a, grid, trans = moved_edit(A, seed=12, unowned="empty")
    edit_b, _, _ = moved_edit(A, seed=13, unowned="empty")
    edit = A.Ed.FieldEdit.from_source(edit_a.source.clone(), *R.BOX, trans, [0, 1, 6], C=C14, unowned="empty")
    u = torch.rand(37, 8, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        eager_a = A.MA.edited_field(mc, mf, rays, args, edit_a, u=u)      # (also the warm-up of every kernel and of the empty row)
        eager_b = A.MA.edited_field(mc, mf, rays, args, edit_b, u=u)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = A.MA.edited_field(mc, mf, rays, args, edit, u=u)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, eager_a):
            assert torch.equal(bits(g), bits(w))
        edit.source.copy_(edit_b.source)
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(out, eager_b):
            assert torch.equal(bits(g), bits(w))
    assert not torch.equal(eager_a[0], eager_b[0])
