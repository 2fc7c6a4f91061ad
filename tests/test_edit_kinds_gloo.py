"""Host tests (gloo, no GPU) of the frame driver with the edit kinds: ``Remove()`` / ``Copy()`` entries of ``trans_list`` and
``keep_labels`` through ``distributed.ManipulationFrameRenderer`` -- the draws per chunk, what reaches ``manipulate_chunk``, and
the frame at world sizes 1, 2 and 3.  The ray generator, the chunk renderer and the draws are injected, as in
tests/test_distributed_gloo.py; the HIP kernels are not involved."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dm_nerf_amd import distributed as D
from dm_nerf_amd import editing as E
from oracle import ref_cpu as O

MH, MW, MCHUNK, MINS, MIMP = 10, 12, 32, 5, 8          # 120 rays: chunks of 32, 32, 32 and a ragged 24 that straddle the bands
KEEP = [0, 2, 4]


def _raygen(H_, W_, K, c2w, row0, nrows):
    o, d = O.get_rays_k(H_, W_, K, c2w)
    return o[row0:row0 + nrows].contiguous(), d[row0:row0 + nrows].contiguous()


def _chunk_exact(ori, tars, models, args, us):
    """Single IEEE operations only (bitwise independent of which rows share a call), touching every input the driver routes: the
    original rays, every target's rays, every draw, the kinds and the keep set."""
    C = MINS + 1
    tag = float(sum((i + 1) * k for i, k in enumerate(args.edit_kinds))) + 0.25 * len(args.keep_labels or [])
    mix = sum(u[:, :3] for u in us)
    org = sum((t[0] for t in tars), torch.zeros_like(ori[0]))
    rgb, ins = ori[0] + ori[1] * mix + org + tag, us[-1][:, :C] * ori[1][:, :1] + us[0][:, 1:C + 1] + org[:, :1]
    if len(tars) == 0:
        return rgb, ins, torch.zeros_like(rgb), torch.zeros_like(ins)
    return rgb, ins, tars[-1][0] * mix + tars[-1][1], us[len(tars)][:, :C] - tars[0][1][:, 2:3]


def _scene():
    K = O.dmsr_intrinsics(MH, MW)
    pose = O.pose_spherical(75.0, -65.0, 7.0)
    m0 = torch.tensor([[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])
    m1 = torch.tensor([[0., -1., 0., 0.], [1., 0., 0., 0.5], [0., 0., 1., 0.], [0., 0., 0., 1.]])
    return K, pose, m0, m1


def _frame(edits, labels, keep=None, log=None, seen=None, **kw):
    K, pose, m0, m1 = _scene()
    trans = {"mixed": [m0, E.Remove(), E.Copy(m1)], "remove": [E.Remove()], "none": []}[edits]
    gen = torch.Generator().manual_seed(77)                 # every rank owns an identically seeded generator, as on the device

    def draws(n, n_imp, count, dev):
        if log is not None:
            log.append((n, count))
        return [torch.rand(n, n_imp, generator=gen) for _ in range(count)]

    def chunk(ori, tars, models, args, us):
        if seen is not None:
            seen.append((list(args.edit_kinds), args.keep_labels, list(args.target_labels), tuple(tars.shape), len(us)))
        return _chunk_exact(ori, tars, models, args, us)
    args = types.SimpleNamespace(N_samples=8, N_importance=MIMP, near=4.0, far=15.0, N_test=MCHUNK, target_labels=labels)
    return D.manipulate_frame(MH, MW, K, pose, trans, None, args, raygen=_raygen, manipulate_chunk=chunk, draws=draws, ins_num=MINS,
                              keep_labels=keep, **kw)


CASES = (("mixed", [2, 4, 1], KEEP), ("mixed", [2, 4, 1], None), ("remove", [3], None), ("none", [], KEEP))


def test_draws_kinds_and_keep_set_reach_the_chunk_renderer():
    log, seen = [], []
    frame = _frame("mixed", [2, 4, 1], KEEP, log, seen)
    assert log == [(32, 4), (32, 4), (32, 4), (24, 4)]                                # 2 + T_r draws: the removal makes none
    assert seen == [([0, 2, 1], KEEP, [2, 4, 1], (2, 2, n, 3), 4) for n in (32, 32, 32, 24)]
    assert frame[0].shape == (MH, MW, 3) and frame[3].shape == (MH, MW, MINS + 1)
    log, seen = [], []
    frame = _frame("remove", [3], None, log, seen)
    assert log == [(32, 2), (32, 2), (32, 2), (24, 2)]
    assert seen == [([2], None, [3], (0, 2, n, 3), 2) for n in (32, 32, 32, 24)]
    assert not frame[2].any() and not frame[3].any() and bool(frame[0].any())          # no target rays: zero target columns
    log, seen = [], []
    _frame("none", [], KEEP, log, seen)
    assert log == [(32, 2)] * 3 + [(24, 2)] and seen[0][:3] == ([], KEEP, [])
    with pytest.raises(ValueError):
        _frame("none", [], None)                                                       # nothing to do still raises
    with pytest.raises(ValueError):
        _frame("mixed", [2, 4], None)                                                  # one label per entry


def test_the_target_rays_are_those_of_the_entries_with_rays():
    K, pose, m0, m1 = _scene()
    args = types.SimpleNamespace(N_samples=8, N_importance=MIMP, near=4.0, far=15.0, N_test=MCHUNK, target_labels=[2, 4, 1])
    plain = D.ManipulationFrameRenderer(MH, MW, K, pose, [m0, m1], None, types.SimpleNamespace(**dict(vars(args), target_labels=[2, 1])),
                                        raygen=_raygen, ins_num=MINS, rank=1, world=3)
    assert not hasattr(plain.args, "edit_kinds") and not hasattr(plain.args, "keep_labels")   # matrices only: today's path
    fr = D.ManipulationFrameRenderer(MH, MW, K, pose, [m0, E.Remove(), E.Copy(m1)], None, args, raygen=_raygen, ins_num=MINS, rank=1, world=3)
    assert fr.T == 2 and torch.equal(fr.tar, plain.tar) and fr.args.edit_kinds == [0, 2, 1] and fr.args.keep_labels is None
    deformed = D.ManipulationFrameRenderer(MH, MW, K, pose, [E.Deform("ex", 0)], None, types.SimpleNamespace(**dict(vars(args), target_labels=[2])),
                                           raygen=_raygen, ins_num=MINS, rank=1, world=3)
    copied = D.ManipulationFrameRenderer(MH, MW, K, pose, [E.Remove(), E.Copy(E.Deform("ex", 0))], None,
                                         types.SimpleNamespace(**dict(vars(args), target_labels=[4, 2])), raygen=_raygen, ins_num=MINS, rank=1, world=3)
    assert torch.equal(copied.tar, deformed.tar) and copied.args.edit_kinds == [2, 1]


def test_bands_of_every_world_size_concatenate_to_the_frame():
    for edits, labels, keep in CASES:
        whole = _frame(edits, labels, keep)
        for world in (1, 2, 3):
            bands = [_frame(edits, labels, keep, rank=r, world=world) for r in range(world)]
            for k in range(4):
                assert torch.equal(torch.cat([b[k] for b in bands], 0), whole[k]), (edits, world, k)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = []
        for edits, labels, keep in CASES:
            log = []
            out.append(([t.numpy() for t in _frame(edits, labels, keep, log)], log))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_frame_over_a_process_group_equals_single_process(world):
    torch.set_num_threads(1)
    want = [_frame(edits, labels, keep) for edits, labels, keep in CASES]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, out in res:
        for (frame, log), w, (edits, _, _) in zip(out, want, CASES):
            assert log == [(n, 4 if edits == "mixed" else 2) for n in (32, 32, 32, 24)]      # every rank: all chunks, 2 + T_r draws
            for got, ref in zip(frame, w):
                assert np.array_equal(got, ref.numpy())


def test_demo_path_takes_the_new_entries_and_a_keep_set():
    K, pose, m0, m1 = _scene()
    objs = [dict(obj_name="a", tar_id=2, mani_mode="translation"), dict(obj_name="b", tar_id=4, mani_mode="translation"),
            dict(obj_name="c", tar_id=1, mani_mode="deform", deform_func="ex")]
    objs_trans = {"a": [dict(transformation=E.Remove())], "b": [dict(transformation=E.Copy(m1))]}
    seen = []

    def chunk(ori, tars, models, args, us):
        seen.append((list(args.edit_kinds), args.keep_labels, list(args.target_labels), tars.shape[0], len(us)))
        return _chunk_exact(ori, tars, models, args, us)
    gen = torch.Generator().manual_seed(3)
    args = types.SimpleNamespace(N_samples=8, N_importance=MIMP, near=4.0, far=15.0, N_test=MCHUNK)
    rgbs = np.arange(39).reshape(13, 3) * 6
    products = lambda rgb, ins, lut: ((255 * rgb.clamp(0, 1)).to(torch.uint8), ins.argmax(-1), ins.argmax(-1).to(torch.uint8), lut[ins.argmax(-1)])
    out = E.manipulate_demo_path([pose], (MH, MW, K), None, args, objs, objs_trans, rgbs, {str(k): k for k in range(13)}, {"0": 1, "2": 7},
                                 products=products, keep_labels=KEEP, raygen=_raygen, manipulate_chunk=chunk, ins_num=MINS,
                                 draws=lambda n, n_imp, count, dev: [torch.rand(n, n_imp, generator=gen) for _ in range(count)])
    assert seen and all(s == ([2, 1, 0], KEEP, [2, 4, 1], 2, 4) for s in seen)
    assert out["rgb8"].shape == (1, MH, MW, 3) and out["label"].shape == (1, MH, MW)
