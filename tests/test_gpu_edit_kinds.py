"""GPU tests (-m gpu) of the edit kinds: ``dmnerf_edit_exchange`` (MOVE / COPY / REMOVE plus the keep mask) against its plain-torch
restatement bit for bit, ``manipulator(..., kinds=, keep_labels=)`` against the default path and against a composition of the
package's separately pinned primitives, and the frame driver with a ``Remove()`` entry.

The restatement's label decisions are the CPU's ``torch.argmax`` (first maximum), so it is always evaluated on host copies of the
device tensors and its result uploaded."""
import types

import pytest
import torch

import _gpu
import _edit_kinds_restate as RS
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

M, C_, R = RS.MOVE, RS.COPY, RS.REMOVE

# (N, S, C, labels, kinds, keep, pass d_ori_label, label of the inf row)
CASES = {
    "C2_remove_only": (37, 13, 2, [0], [R], None, True, 0),
    "C2_move": (37, 13, 2, [0], [M], None, False, None),
    "C2_copy_keep": (37, 13, 2, [0], [C_], [0], True, None),
    "remove_first": (37, 13, 14, [5, 0, 3], [R, M, C_], None, True, 5),
    "remove_last_keep": (37, 13, 14, [0, 5, 3], [M, C_, R], [0, 1, 5, 8, 13], False, None),
    "E8_S320": (5, 320, 14, [3, 0, 5, 7, 1, 9, 2, 12], [M, R, C_, M, R, C_, M, R], None, True, None),
    "E8_all_moves": (5, 320, 14, [3, 0, 5, 7, 1, 9, 2, 12], [M] * 8, None, False, None),
    "C128": (3, 7, 128, [70, 0], [C_, R], list(range(0, 128, 3)) + [127], True, None),
    "C128_remove_move": (3, 7, 128, [0, 126], [R, M], None, False, 0),
    "keep_only_E0": (37, 13, 14, [], [], [0, 2, 5, 11], True, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_restatement_bit_for_bit(name):
    from dm_nerf_amd.networks import manipulator as MA
    N, S, C, labels, kinds, keep, want_label, inf_label = CASES[name]
    assert (N * S) % 256 != 0
    c = RS.make_case(N, S, C, labels, kinds, seed=100 + len(name), inf_label=inf_label)
    counts = {}
    want, want_lab = RS.edit_restate(c["ori"].clone(), c["tars"], c["ori_acc"], c["tar_accs"], labels, kinds, keep_labels=keep, counts=counts)
    dev = lambda t: None if t is None else t.cuda()
    ori = c["ori"].clone().cuda()
    tars, accs = [dev(t) for t in c["tars"]], [dev(t) for t in c["tar_accs"]]
    got, got_lab = MA.edit_exchanger(ori, tars, c["ori_acc"].cuda(), accs, labels, kinds, keep_labels=keep, want_label=want_label)
    torch.cuda.synchronize()
    assert got.data_ptr() == ori.data_ptr()                                      # in place, like the reference
    assert torch.equal(RS.bits(got.cpu()), RS.bits(want))
    if want_label:
        assert torch.equal(got_lab.cpu(), want_lab)
    else:
        assert got_lab is None
    for t, src in zip(tars + accs, c["tars"] + c["tar_accs"]):                   # the targets are only read
        assert t is None or torch.equal(RS.bits(t.cpu()), RS.bits(src))
    assert not torch.equal(RS.bits(want), RS.bits(c["ori"])) and sum(counts.values()) >= 1
    if inf_label is not None:                                                    # inf * 0: NaN in both
        assert bool(torch.isnan(want[N - 1, S - 1, 1])) and bool(torch.isnan(got[N - 1, S - 1, 1]))
    if name == "E8_S320":
        assert all(counts[k] >= 1 for k in RS.BRANCHES if k != "keep_zero"), counts


def test_all_moves_equal_the_exchanger_entry():
    """The MOVE kind is the existing exchanger: same bytes, same labels."""
    from dm_nerf_amd.networks import manipulator as MA
    labels = [3, 0, 5]
    c = RS.make_case(37, 13, 14, labels, [M] * 3, seed=77)
    tars, accs = [t.cuda() for t in c["tars"]], [t.cuda() for t in c["tar_accs"]]
    a, _, a_lab, _ = MA.exchanger(c["ori"].clone().cuda(), tars, c["ori_acc"].cuda(), accs, labels)
    b, b_lab = MA.edit_exchanger(c["ori"].clone().cuda(), tars, c["ori_acc"].cuda(), accs, labels, [M] * 3)
    assert torch.equal(RS.bits(a), RS.bits(b)) and torch.equal(a_lab, b_lab)


# ---- manipulator(): 67 rays, 8 coarse + 16 fine samples, ins_num 3 (C = 4) ------------------------------------------------
NR, NS, NI, INS = 67, 8, 16, 3


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"

    def mk(seed):
        return _gpu.model_from(O.make_weights(seed, INS, **O.PEAKY), INS)
    K = O.dmsr_intrinsics(24, 32)
    ro, rd = O.get_rays_k(24, 32, K, O.pose_spherical(75.0, -65.0, 7.0))
    sel = torch.arange(NR) * 11 % (24 * 32)
    ori = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]]).cuda().contiguous()
    tars = []
    for shift in ([0.3, -0.2, 0.1], [-0.4, 0.25, 0.0]):
        t = ori.clone()
        t[0] += torch.tensor(shift, device="cuda")
        tars.append(t)
    gen = torch.Generator().manual_seed(9)
    us = [torch.rand(NR, NI, generator=gen).cuda() for _ in range(4)]
    return types.SimpleNamespace(mc=mk(731), mf=mk(732), ori=ori, tars=tars, us=us)


def _args(labels):
    return types.SimpleNamespace(N_samples=NS, N_importance=NI, near=4.0, far=15.0, target_labels=labels)


@pytest.mark.parametrize("T", [1, 2])
def test_moves_given_as_kinds_are_the_default_path(scene, T):
    from dm_nerf_amd.networks import manipulator as MA
    a = _args([1, 2][:T])
    with torch.no_grad():
        base = MA.manipulator(None, None, scene.mc, scene.mf, scene.ori, scene.tars[:T], a, us=scene.us[:2 + T])
        kind = MA.manipulator(None, None, scene.mc, scene.mf, scene.ori, scene.tars[:T], a, us=scene.us[:2 + T], kinds=[MA.MOVE] * T)
    for b, k in zip(base, kind):
        assert b.shape == k.shape and torch.equal(RS.bits(b), RS.bits(k))
    assert bool(torch.isfinite(base[0]).all())


def _restate_on_device(ori_raw, tar_raws, ori_acc, tar_accs, labels, kinds, keep, counts):
    host = lambda t: None if t is None else t.cpu()
    out, _ = RS.edit_restate(ori_raw.cpu(), [host(t) for t in tar_raws], ori_acc.cpu(), [host(t) for t in tar_accs], labels, kinds,
                             keep_labels=keep, counts=counts)
    return out.cuda()


def _referee(scene, labels, kinds, keep, us, counts):
    """``manipulator`` with kinds, composed here of ``manipulator_nerf``, ``manipulator_render``, ``helpers.importance_resample`` and
    ``sort_rows`` (each pinned by its own tests), with the RESTATEMENT as the exchange: it shares no code with the new kernel."""
    from dm_nerf_amd.networks import helpers as Hh, manipulator as MA
    mc, mf, ori = scene.mc, scene.mf, scene.ori
    tar_rays = iter(scene.tars)
    rays = [None if k == R else next(tar_rays) for k in kinds]                     # per edit
    us = list(us)
    raw, z = MA.manipulator_nerf(ori, None, None, mc, NS, 4.0, 15.0)
    _, w, _, _ = MA.manipulator_render(raw, z, ori[1])
    z_full = Hh.importance_resample(z, w, NI, u=us.pop(0))
    raw_full, _ = MA.manipulator_nerf(ori, None, None, mf, z_vals=z_full)
    _, _, _, ori_acc = MA.manipulator_render(raw_full, z_full, ori[1])
    t_raw, t_z, t_zs, t_acc = [None] * len(kinds), {}, [], [None] * len(kinds)
    tar_rgb = tar_ins = None
    for e, tr in enumerate(rays):
        if tr is None:
            continue
        t_raw[e], t_z[e] = MA.manipulator_nerf(tr, None, None, mc, NS, 4.0, 15.0)
        tar_rgb, tw, _, _ = MA.manipulator_render(t_raw[e], t_z[e], tr[1])
        tz_full, tzs = Hh.importance_resample(t_z[e], tw, NI, u=us.pop(0), return_samples=True)
        tfull, _ = MA.manipulator_nerf(tr, None, None, mf, z_vals=tz_full)
        _, _, _, t_acc[e] = MA.manipulator_render(tfull, tz_full, tr[1])
        tar_ins = t_acc[e]
        t_zs.append(tzs)
    raw = _restate_on_device(raw, t_raw, ori_acc, t_acc, labels, kinds, keep, counts)
    _, w, _, _ = MA.manipulator_render(raw, z, ori[1])
    _, zs = Hh.importance_resample(z, w, NI, u=us.pop(0), return_samples=True)
    assert not us
    merged = MA.sort_rows(torch.cat([z, zs] + t_zs, -1))
    assert merged.shape[1] == NS + NI + NI * len(t_zs)
    raw, _ = MA.manipulator_nerf(ori, None, None, mf, z_vals=merged)
    for e, tr in enumerate(rays):
        if tr is not None:
            t_raw[e], _ = MA.manipulator_nerf(tr, None, None, mf, z_vals=MA.sort_rows(torch.cat([t_z[e], zs] + t_zs, -1)))
    raw = _restate_on_device(raw, t_raw, ori_acc, t_acc, labels, kinds, keep, counts)
    rgb, _, _, ins = MA.manipulator_render(raw, merged, ori[1])
    if tar_rgb is None:
        tar_rgb, tar_ins = torch.zeros_like(rgb), torch.zeros_like(ins)
    return (rgb, ins, tar_rgb, tar_ins), ori_acc


def _ray_label(scene):
    """The most frequent accumulated label of the scene's rays: the object the tests edit, so that the edit has rows to act on."""
    from dm_nerf_amd.networks import helpers as Hh, manipulator as MA
    raw, z = MA.manipulator_nerf(scene.ori, None, None, scene.mc, NS, 4.0, 15.0)
    _, w, _, _ = MA.manipulator_render(raw, z, scene.ori[1])
    z_full = Hh.importance_resample(z, w, NI, u=scene.us[0])
    raw_full, _ = MA.manipulator_nerf(scene.ori, None, None, scene.mf, z_vals=z_full)
    acc = MA.manipulator_render(raw_full, z_full, scene.ori[1])[3].cpu()
    return int(torch.bincount(torch.argmax(torch.sigmoid(acc[:, :-1]), -1), minlength=INS).argmax())


@pytest.mark.parametrize("which", ["remove", "mixed", "remove_keep"])
def test_chunk_with_kinds_equals_the_composition_of_pinned_primitives(scene, which):
    from dm_nerf_amd.networks import manipulator as MA
    L = _ray_label(scene)
    labels, kinds, keep = {"remove": ([L], [R], None),
                           "mixed": ([(L + 1) % INS, L, (L + 2) % INS], [M, R, C_], None),
                           "remove_keep": ([L], [R], [L, (L + 1) % INS, INS])}[which]
    n_rays = sum(k != R for k in kinds)
    us = scene.us[:2 + n_rays]
    counts = {}
    with torch.no_grad():
        want, _ = _referee(scene, labels, kinds, keep, us, counts)
        got = MA.manipulator(None, None, scene.mc, scene.mf, scene.ori, scene.tars[:n_rays], _args(labels), us=us, kinds=kinds, keep_labels=keep)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(RS.bits(g), RS.bits(w))
    assert counts["remove"] >= 1, counts                                          # the edit acted on rows of both rounds' inputs
    if n_rays == 0:
        assert not got[2].any() and not got[3].any() and got[2].shape == (NR, 3) and got[3].shape == (NR, INS + 1)
    # ... and it shows: the frame differs from the same call with the removal left out
    if which == "remove":
        with torch.no_grad():
            moved = MA.manipulator(None, None, scene.mc, scene.mf, scene.ori, [], _args([]), us=us, kinds=[], keep_labels=list(range(INS + 1)))
        assert not torch.equal(moved[0], got[0])


# ---- the frame driver -----------------------------------------------------------------------------------------------------
FH, FW, FCHUNK = 8, 12, 40                      # 96 rays: chunks of 40, 40 and a ragged 16


def test_removal_frame_equals_chunkwise_manipulator_and_its_bands_at_every_world_size(scene):
    from dm_nerf_amd import distributed as D, editing as E
    from dm_nerf_amd.networks import helpers as Hh, manipulator as MA
    K = O.dmsr_intrinsics(FH, FW)
    pose = O.pose_spherical(75.0, -65.0, 7.0)
    L = _ray_label(scene)
    a = types.SimpleNamespace(N_samples=NS, N_importance=NI, near=4.0, far=15.0, N_test=FCHUNK, target_labels=[L])
    n_chunks = -(-FH * FW // FCHUNK)
    gen = torch.Generator().manual_seed(5)
    us = [[torch.rand(min(FCHUNK, FH * FW - c * FCHUNK), NI, generator=gen).cuda() for _ in range(2)] for c in range(n_chunks)]

    def frame(**kw):
        calls = []

        def draws(n, n_imp, count, dev):
            calls.append((n, n_imp, count))
            return us[len(calls) - 1]
        out = D.manipulate_frame(FH, FW, K, pose.cuda(), [E.Remove()], (scene.mc, scene.mf), a, draws=draws, ins_num=INS, **kw)
        assert calls == [(min(FCHUNK, FH * FW - c * FCHUNK), NI, 2) for c in range(n_chunks)]      # 2 + T_r draws, T_r = 0
        return out
    with torch.no_grad():
        whole = frame()
        ro, rd = Hh.get_rays_k(FH, FW, K, pose.cuda())
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        cols = [[], [], [], []]
        for c, s in enumerate(range(0, FH * FW, FCHUNK)):
            e = min(s + FCHUNK, FH * FW)
            out = MA.manipulator(None, None, scene.mc, scene.mf, torch.stack([ro[s:e], rd[s:e]]), [], a, us=us[c], kinds=[MA.REMOVE])
            for col, t in zip(cols, out):
                col.append(t)
        C = INS + 1
        for got, col, width in zip(whole, cols, (3, C, 3, C)):
            assert torch.equal(RS.bits(got), RS.bits(torch.cat(col, 0).reshape(FH, FW, width)))
        assert not whole[2].any() and not whole[3].any() and bool(torch.isfinite(whole[0]).all())
        for world in (1, 2, 3):
            bands = [frame(rank=r, world=world) for r in range(world)]
            for k in range(4):
                assert torch.equal(RS.bits(torch.cat([b[k] for b in bands], 0)), RS.bits(whole[k])), (world, k)
