"""GPU tests (-m gpu) of dm_nerf_amd.editing -- the drivers around ``manipulator()`` (networks/manipulator.py:208-491) and the
two kernels of csrc/edit_frame.hip:

* target rays of rigid and deformed objects against the reference's own ``manipulator_demo`` runs (tests/golden/edit_path.npz:
  run a = two rigid objects, run b = ``sin`` + ``ex`` deformations; two views of 10 x 16 rays, chunks 64, 64, 32), and
  ``dmnerf_edit_rays`` alone on a band that is no wave multiple, with offsets where f64-sum-then-round and an f32 add differ;
* ``frame_products`` against the three images the reference wrote, and at the shapes where the kernel can go wrong;
* the demo driver == chunk-by-chunk ``manipulator()`` calls on the same rays and draws, bit for bit; the plain target render
  within 1e-4 of the reference's; the frame bit-identical for every world size with a deformation and the device's own draws;
* the evaluation path's scores == the device metrics on the returned frames, its images == the reference's dict loops.

The fixture stores no draws: its generator asserts that they are the successive ``torch.rand([n, 128])`` calls after
``torch.manual_seed(741)``, and ``_draws`` remakes them."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import _gpu
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

FUNCS = ("sin", "ex")
SIZES = (64, 64, 32)


def _mk(seed, ins_num):
    return _gpu.model_from(O.make_weights(int(seed), ins_num, **O.PEAKY), ins_num)


@functools.lru_cache(maxsize=None)
def _models(ins_num=7):
    return _mk(721, ins_num), _mk(722, ins_num)


def _setup(g, tag):
    """objs / objs_trans of a fixture run in the form ``manipulator_demo`` takes them, and the per-view edits of the renderer."""
    from dm_nerf_amd import editing as E
    tar_id = [int(v) for v in g[f"{tag}_tar_id"]]
    if tag == "a":
        objs = [dict(obj_name=f"o{t}", tar_id=tar_id[t], mani_mode="rigid") for t in range(len(tar_id))]
        objs_trans = {f"o{t}": [dict(transformation=g["a_trans"][t, i].tolist()) for i in range(g["a_trans"].shape[1])]
                      for t in range(len(tar_id))}
        edits = [[g["a_trans"][t, i] for t in range(len(tar_id))] for i in range(g["a_trans"].shape[1])]
    else:
        funcs = [FUNCS[int(v)] for v in g["b_func"]]
        objs = [dict(obj_name=f"o{t}", tar_id=tar_id[t], mani_mode="deform", deform_func=funcs[t]) for t in range(len(tar_id))]
        objs_trans = {}
        edits = [[E.Deform(f, i) for f in funcs] for i in range(g["b_poses"].shape[0])]
    return objs, objs_trans, edits, tar_id


def _args(g, **kw):
    return types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=int(g["HWN"][2]), **kw)


def _tables(g):
    return (g["ins_rgbs"].numpy(), {str(int(k)): int(v) for k, v in g["color_dict"]}, {str(int(k)): int(v) for k, v in g["ins_map"]})


def _draws(g, views, T):
    gen = torch.Generator().manual_seed(int(g["rng_seed"]))
    return [[[torch.rand(n, 128, generator=gen).cuda() for _ in range(2 + T)] for n in SIZES] for _ in range(views)]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_target_rays_against_the_reference_demo_run(golden, tag):
    from dm_nerf_amd import distributed as D, editing as E
    g = golden("edit_path")
    H, W, _ = [int(v) for v in g["HWN"]]
    objs, objs_trans, edits, tar_id = _setup(g, tag)
    for i, pose in enumerate(g[f"{tag}_poses"]):
        fr = D.ManipulationFrameRenderer(H, W, g["K"].numpy(), pose.cuda(), edits[i], _models(), _args(g, target_labels=tar_id))
        ori, tar = g[f"{tag}_ori_rays{i}"], g[f"{tag}_tar_rays{i}"]
        assert tuple(fr.tar.shape) == tuple(tar.shape) == (len(tar_id), 2, H * W, 3)
        assert torch.equal(fr.ori[0].cpu(), ori[0])
        assert torch.allclose(fr.ori[1].cpu(), ori[1], rtol=3e-7, atol=1e-7)
        for t in range(len(tar_id)):
            if tag == "a":                                   # a host 4 x 4 product behind it: test_gpu_manipulator_frame.py:204-207
                assert torch.allclose(fr.tar[t, 0].cpu(), tar[t, 0], rtol=3e-7, atol=1e-7)
                assert torch.allclose(fr.tar[t, 1].cpu(), tar[t, 1], rtol=3e-7, atol=1e-7)
                continue
            off = torch.from_numpy(E.deform_offsets(H, FUNCS[int(g["b_func"][t])], i)).repeat_interleave(W)
            # the reference's own arithmetic, on its recorded base: f32 column + f64 tensor, rounded once
            assert torch.equal(tar[t, 0, :, 0], (ori[0, :, 0].double() + off).float())
            assert torch.equal(tar[t, 0, :, 1:], ori[0, :, 1:]) and torch.equal(tar[t, 1], ori[1])
            # the kernel on the driver's own original rays: exactly that arithmetic ...
            assert torch.equal(fr.tar[t, 0, :, 0], (fr.ori[0, :, 0].double() + off.cuda()).float())
            assert torch.equal(fr.tar[t, 0, :, 1:], fr.ori[0, :, 1:]) and torch.equal(fr.tar[t, 1], fr.ori[1])
            # ... so the origins (an exact base) equal the recorded ones, the directions as the original rays' do
            assert torch.equal(fr.tar[t, 0].cpu(), tar[t, 0])
            assert torch.allclose(fr.tar[t, 1].cpu(), tar[t, 1], rtol=3e-7, atol=1e-7)
        if tag == "b" and i == 1:
            assert float((fr.tar[0, 0, :, 0] - fr.ori[0, :, 0]).abs().max()) > 1e-3      # sin, view 1: the object does move


def test_edit_rays_alone_on_a_band_that_is_no_wave_multiple():
    from dm_nerf_amd import editing as E
    from dm_nerf_amd.networks import helpers as Hh
    H, W, row0, nrows = 5, 7, 1, 3                           # 21 rays
    K = O.dmsr_intrinsics(H, W)
    poses = [O.pose_spherical(75.0, -65.0, 7.0), O.pose_spherical(40.0, -50.0, 6.5), O.pose_spherical(10.0, -30.0, 8.0)]
    x = poses[1][0, 3]                                       # the deformed object's origin x (f32)
    cand = torch.rand(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 2 - 1
    differ = (x.double() + cand).float() != x + cand.float()
    assert bool(differ.any()) and not bool(differ.all())     # offsets exist where rounding the f64 offset first changes the sum
    off = torch.rand(3, H, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    off[1, 2], off[1, 3] = cand[differ][0], cand[~differ][0]
    rays = E.edit_rays(H, W, K, poses, [0, 1, 0], off.numpy(), row0=row0, nrows=nrows)
    assert tuple(rays.shape) == (3, 2, nrows * W, 3)
    for t in (0, 2):
        ro, rd = Hh.get_rays_k(H, W, K, poses[t].cuda(), row0, nrows)
        assert torch.equal(rays[t, 0], ro.reshape(-1, 3)) and torch.equal(rays[t, 1], rd.reshape(-1, 3))
    ro, rd = Hh.get_rays_k(H, W, K, poses[1].cuda(), row0, nrows)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    rows = (torch.arange(nrows * W, device="cuda") // W) + row0               # ABSOLUTE image rows
    want = (ro[:, 0].double() + off.cuda()[1][rows]).float()
    assert torch.equal(rays[1, 0, :, 0], want)
    assert torch.equal(rays[1, 0, :, 1:], ro[:, 1:]) and torch.equal(rays[1, 1], rd)
    f32_add = ro[:, 0] + off.cuda()[1][rows].float()
    assert not torch.equal(want, f32_add) and torch.equal(want[rows == 3], f32_add[rows == 3])
    # the whole frame in one call, and an empty band
    full = E.edit_rays(H, W, K, poses, [0, 1, 0], off.numpy())
    assert torch.equal(full[:, :, row0 * W:(row0 + nrows) * W], rays)
    assert tuple(E.edit_rays(H, W, K, poses, [0, 1, 0], off.numpy(), row0=5, nrows=0).shape) == (3, 2, 0, 3)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_products_equal_the_images_the_reference_wrote(golden, tag):
    from dm_nerf_amd import editing as E
    g = golden("edit_path")
    H, W, _ = [int(v) for v in g["HWN"]]
    C = int(g["ins_num"]) + 1
    lut = E.label_lut(C, *_tables(g))
    assert lut.is_cuda and not bool(lut[5].any())            # label 5 has no entry in the fixture's ins_map: black
    seen = set()
    for i in range(g[f"{tag}_poses"].shape[0]):
        rgb = g[f"{tag}_full_rgb{i}"].cuda().reshape(H, W, 3)
        ins = g[f"{tag}_full_ins{i}"].cuda().reshape(H, W, C)
        rgb8, label, mask, ins_img = E.frame_products(rgb, ins, lut)
        assert torch.equal(rgb8.cpu(), g[f"{tag}_rgb8{i}"])
        assert torch.equal(ins_img.cpu(), g[f"{tag}_ins_img{i}"])
        assert torch.equal(mask.cpu(), g[f"{tag}_mask{i}"]) and torch.equal(label.cpu(), g[f"{tag}_mask{i}"].long())
        seen |= set(label.unique().tolist())
    assert 5 in seen and C - 1 in seen                       # the unmapped label and the last channel both occur


def _product_inputs(n, C, seed):
    gen = torch.Generator().manual_seed(seed)
    buf = torch.randn(n, 2 * (3 + C), generator=gen)
    rgb = torch.rand(n, 3, generator=gen) * 2 - 0.5                                  # values below 0 and above 1
    special = torch.tensor([0.0, 1.0, 254.5 / 255, float(np.nextafter(np.float32(1), np.float32(0))), -0.0, 1.0 / 255,
                            float(np.nextafter(np.float32(1.0 / 255), np.float32(0))), 128.0 / 255, -3.0, 7.5])
    flat = rgb.reshape(-1)
    k = min(flat.numel(), special.numel())
    flat[:k] = special[:k]
    ins = torch.randn(n, C, generator=gen)
    for r in range(n):
        if r % 4 == 1:                                                              # tied maxima: the first one wins
            top = ins[r].max() + 1
            ins[r, torch.randperm(C, generator=gen)[:2]] = top
        elif r % 4 == 2:                                                            # an all-equal row
            ins[r] = float(r % 3) - 1
    buf[:, 0:3], buf[:, 3:3 + C] = rgb, ins
    return buf.cuda()


@pytest.mark.parametrize("strided", [True, False])
@pytest.mark.parametrize("C", [2, 8, 14, 65, 95, 129])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_products_at_the_shapes_where_the_kernel_can_go_wrong(n, C, strided):
    from dm_nerf_amd import editing as E
    from dm_nerf_amd.networks import evaluator as Ev
    buf = _product_inputs(n, C, 1000 * n + C)
    rgb, ins = buf[:, 0:3], buf[:, 3:3 + C]
    if not strided:
        rgb, ins = torch.empty(n, 3, device="cuda").copy_(rgb), torch.empty(n, C, device="cuda").copy_(ins)   # (fresh rows of 3 / C floats)
    # (the row stride says it: torch calls a one-row slice contiguous whatever its stride)
    assert rgb.stride(0) == (2 * (3 + C) if strided else 3) and ins.stride(0) == (2 * (3 + C) if strided else C)
    lut = torch.randint(0, 256, (C, 3), generator=torch.Generator().manual_seed(C), dtype=torch.uint8).cuda()
    before = buf.clone()
    rgb8, label, mask, ins_img = E.frame_products(rgb, ins, lut)
    want_label, _ = Ev.ins_label_conf(ins.contiguous())
    assert label.dtype == torch.int64 and torch.equal(label, want_label)
    assert np.array_equal(label.cpu().numpy(), np.argmax(ins.cpu().numpy(), -1))     # numpy: the first maximum
    assert torch.equal(rgb8, (255 * rgb.clamp(0, 1)).to(torch.uint8))
    assert torch.equal(mask, label.to(torch.uint8)) and torch.equal(ins_img, lut[label])
    assert torch.equal(buf, before)                                                  # inputs untouched
    if n * 3 >= 4:
        assert rgb8.reshape(-1)[:4].tolist() == [0, 255, 254, 254]


def test_products_leave_the_outputs_without_input_untouched():
    from dm_nerf_amd import _lib
    n, C = 65, 14
    buf = _product_inputs(n, C, 5)
    rgb, ins = buf[:, 0:3], buf[:, 3:3 + C]
    stride = buf.stride(0)
    lut = torch.randint(0, 256, (C, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    lib = _lib.load()

    def fresh():
        return (torch.full((n, 3), 77, dtype=torch.uint8, device="cuda"), torch.full((n,), -5, dtype=torch.int64, device="cuda"),
                torch.full((n,), 77, dtype=torch.uint8, device="cuda"), torch.full((n, 3), 77, dtype=torch.uint8, device="cuda"))
    want8 = (255 * rgb.clamp(0, 1)).to(torch.uint8)
    want_label = torch.from_numpy(np.argmax(ins.cpu().numpy(), -1)).cuda()
    # no object channels: only the 8-bit frame is written (the table alone colours nothing)
    rgb8, label, mask, img = fresh()
    _lib.check(lib.dmnerf_edit_products(_lib.ptr(rgb), stride, None, 0, 0, _lib.ptr(lut), n, _lib.ptr(rgb8), _lib.ptr(label), _lib.ptr(mask),
                                        _lib.ptr(img), _lib.stream()), "dmnerf_edit_products")
    assert torch.equal(rgb8, want8) and bool((label == -5).all()) and bool((mask == 77).all()) and bool((img == 77).all())
    # no table: label and mask, no object image
    rgb8, label, mask, img = fresh()
    _lib.check(lib.dmnerf_edit_products(_lib.ptr(rgb), stride, _lib.ptr(ins), stride, C, None, n, _lib.ptr(rgb8), _lib.ptr(label), _lib.ptr(mask),
                                        _lib.ptr(img), _lib.stream()), "dmnerf_edit_products")
    assert torch.equal(rgb8, want8) and torch.equal(label, want_label) and torch.equal(mask, want_label.to(torch.uint8))
    assert bool((img == 77).all())
    # every output is optional
    rgb8, label, mask, img = fresh()
    _lib.check(lib.dmnerf_edit_products(_lib.ptr(rgb), stride, _lib.ptr(ins), stride, C, _lib.ptr(lut), n, None, None, None, _lib.ptr(img),
                                        _lib.stream()), "dmnerf_edit_products")
    assert torch.equal(img, lut[want_label]) and bool((rgb8 == 77).all()) and bool((label == -5).all()) and bool((mask == 77).all())


@functools.lru_cache(maxsize=None)
def _demo_run(tag):
    """``manipulate_demo_path`` of a fixture run on the reference's RECORDED rays (a 1-ulp change of a direction is amplified by the
    chain like any other rounding, tests/test_gpu_manipulator_frame.py:208-212) and remade draws, next to the chunk-by-chunk
    ``manipulator()`` calls on the same rays and draws."""
    from dm_nerf_amd import editing as E
    from dm_nerf_amd.distributed import _default_manipulate_chunk
    from dm_nerf_amd.networks import manipulator as MA
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edit_path.npz")) as z:   # (as the golden fixture loads it)
        g = {k: (torch.from_numpy(z[k]) if z[k].ndim > 0 else z[k].item()) for k in z.files}
    H, W, _ = [int(v) for v in g["HWN"]]
    objs, objs_trans, _, tar_id = _setup(g, tag)
    poses = g[f"{tag}_poses"]
    T, P = len(tar_id), poses.shape[0]
    us = _draws(g, P, T)
    view, calls, labels = [-1], [], []

    def raygen(H_, W_, K, c2w, row0, nrows):
        view[0] += 1
        ori = g[f"{tag}_ori_rays{view[0]}"].cuda()
        return ori[0].reshape(H_, W_, 3)[row0:row0 + nrows].contiguous(), ori[1].reshape(H_, W_, 3)[row0:row0 + nrows].contiguous()

    def target_rays(H_, W_, K, poses_, kinds, offsets, row0, nrows):
        assert kinds == ([0] * T if tag == "a" else [1] * T) and offsets.shape == (T, H_)
        return g[f"{tag}_tar_rays{view[0]}"].cuda()[:, :, row0 * W_:(row0 + nrows) * W_].contiguous()

    def draws(n, n_imp, count, dev):
        calls.append((n, n_imp, count))
        return us[view[0]][(len(calls) - 1) % len(SIZES)]

    def chunk(ori, tars, models, args, us_):
        labels.append(list(args.target_labels))
        return _default_manipulate_chunk(ori, tars, models, args, us_)
    models = _models()
    with torch.no_grad():
        out = E.manipulate_demo_path(poses, (H, W, g["K"].numpy()), models, _args(g), objs, objs_trans, *_tables(g), keep_maps=True,
                                     raygen=raygen, target_rays=target_rays, draws=draws, manipulate_chunk=chunk)
        a = _args(g, target_labels=tar_id)
        want = []
        for i in range(P):
            ori, tar = g[f"{tag}_ori_rays{i}"].cuda(), g[f"{tag}_tar_rays{i}"].cuda()
            cols = [[], [], [], []]
            for c, s in enumerate(range(0, H * W, a.N_test)):
                e = min(s + a.N_test, H * W)
                res = MA.manipulator(None, None, models[0], models[1], ori[:, s:e].contiguous(), tar[:, :, s:e].contiguous(), a, us=us[i][c])
                for col, t in zip(cols, res):
                    col.append(t)
            want.append([torch.cat(col, 0).reshape(H, W, -1) for col in cols])
    torch.cuda.synchronize()
    return g, out, want, calls, labels, tar_id


@pytest.mark.parametrize("tag", ["a", "b"])
def test_demo_driver_equals_chunk_by_chunk_manipulator_calls(tag):
    g, out, want, calls, labels, tar_id = _demo_run(tag)
    H, W, _ = [int(v) for v in g["HWN"]]
    P, T, C = len(want), len(tar_id), int(g["ins_num"]) + 1
    assert calls == [(n, 128, 2 + T) for _ in range(P) for n in SIZES]
    assert len(labels) == P * len(SIZES) and all(l == tar_id for l in labels)
    for k, (name, width) in enumerate(zip(("rgb", "ins", "tar_rgb", "tar_ins"), (3, C, 3, C))):
        assert tuple(out[name].shape) == (P, H, W, width)
        for i in range(P):
            assert torch.equal(out[name][i], want[i][k]), (name, i)
    assert bool(torch.isfinite(out["ins"]).all()) and len(torch.unique(out["label"])) >= 3
    # the products are those of the float frames
    assert out["rgb8"].dtype == torch.uint8 and torch.equal(out["rgb8"], (255 * out["rgb"].clamp(0, 1)).to(torch.uint8))
    assert np.array_equal(out["label"].cpu().numpy(), np.argmax(out["ins"].cpu().numpy(), -1))
    assert out["mask"].dtype == torch.uint8 and torch.equal(out["mask"], out["label"].to(torch.uint8))
    from dm_nerf_amd import editing as E
    assert torch.equal(out["ins_img"], E.label_lut(C, *_tables(g))[out["label"]])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_plain_target_render_against_the_reference_run(tag):
    """With the recorded rays and draws the coarse render of the (last) target's rays has no resampling behind it: within 1e-4 of
    the reference's on every pixel, the bound tests/test_gpu_manipulator_frame.py holds it to for the same weights.  The edited
    outputs are ill-conditioned on a minority of pixels; their rule (oracle/manip_margins.py) belongs to the T = 1 fixture."""
    g, out, _, _, _, _ = _demo_run(tag)
    H, W, _ = [int(v) for v in g["HWN"]]
    for i in range(out["tar_rgb"].shape[0]):
        err = float((out["tar_rgb"][i].cpu() - g[f"{tag}_full_tar_rgb{i}"].reshape(H, W, 3)).abs().max())
        print(f"[edit path run {tag} view {i}] max |tar_rgb - reference| = {err:.2e}")
        assert err <= 1e-4, (tag, i, err)


def test_frame_with_a_deform_is_bit_identical_for_every_world_size_including_the_device_draws(golden):
    from dm_nerf_amd import distributed as D
    g = golden("edit_path")
    H, W, _ = [int(v) for v in g["HWN"]]
    _, _, edits, tar_id = _setup(g, "b")
    K, pose, models = g["K"].numpy(), g["b_poses"][1].cuda(), _models()
    a = _args(g, target_labels=tar_id)
    seed = 11
    with torch.no_grad():
        torch.manual_seed(seed); torch.cuda.manual_seed(seed)
        whole = D.manipulate_frame(H, W, K, pose, edits[1], models, a)
        state_after = torch.cuda.get_rng_state()
        for world in (2, 7):                                                         # 7: bands of 2 2 2 1 1 1 1 rows
            bands = []
            for rank in range(world):
                torch.manual_seed(seed); torch.cuda.manual_seed(seed)
                bands.append(D.manipulate_frame(H, W, K, pose, edits[1], models, a, rank=rank, world=world))
                assert torch.equal(torch.cuda.get_rng_state(), state_after)
            for k in range(4):
                assert torch.equal(torch.cat([b[k] for b in bands], 0), whole[k]), (world, k)
    assert bool(torch.isfinite(torch.cat([f.reshape(-1) for f in whole])).all())


def test_evaluation_path_scores_and_images():
    from dm_nerf_amd import distributed as D, editing as E
    from dm_nerf_amd.networks import evaluator as Ev
    H, W, INS = 12, 16, 7
    K = O.dmsr_intrinsics(H, W)
    poses = [O.pose_spherical(75.0, -65.0, 7.0), O.pose_spherical(60.0, -60.0, 7.0)]
    trans = torch.tensor([[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])
    gen = torch.Generator().manual_seed(4)
    gt_rgbs = torch.rand(2, H, W, 3, generator=gen)
    gt_labels = torch.tensor([0, 2, 5])[torch.randint(0, 3, (2, H, W), generator=gen)]      # three labels
    rgbs = np.random.RandomState(6).randint(1, 256, size=(13, 3))
    color_dict = {str(k): (k + 3) % 13 for k in range(13) if k != 5}                          # gt label 5 has no colour: black
    a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=64, target_label=2, ins_num=INS)
    torch.manual_seed(3); torch.cuda.manual_seed(3)
    with torch.no_grad():
        out = E.manipulate_eval_path(poses, (H, W, K), _models(INS), a, trans, gt_rgbs=gt_rgbs, gt_labels=gt_labels, ins_rgbs=rgbs,
                                     color_dict=color_dict, keep_maps=True)
    assert not hasattr(a, "target_labels")
    assert tuple(out["rgb"].shape) == (2, H, W, 3) and tuple(out["ins"].shape) == (2, H, W, INS + 1)
    for name in ("rgb", "tar_rgb"):
        assert out[name + "8"].dtype == torch.uint8 and torch.equal(out[name + "8"], (255 * out[name].clamp(0, 1)).to(torch.uint8))
    ssim, psnr = Ev.img_metrics_device(out["rgb"], gt_rgbs.cuda())
    assert torch.equal(out["ssim"], ssim) and torch.equal(out["psnr_f64"], psnr) and out["psnr"].dtype == torch.float32
    # (the f32 mean of 576 squares is within 576 x 2^-24 = 3.4e-5 of the f64 one: 1.5e-4 dB)
    assert torch.allclose(out["psnr"].double(), psnr, rtol=0, atol=2e-4)
    for i in range(2):
        gl = gt_labels[i].cuda()
        rows = torch.unique(gl)
        label, conf = Ev.ins_label_conf(out["ins"][i][..., :-1])
        _, ap, matched = Ev.ins_eval_device(label, conf, gl, rows, INS)
        assert torch.equal(out["ap"][i], ap) and torch.equal(out["matched"][i], matched) and int(out["gt_num"][i]) == 3
        # the object image through this pose's own matching: the dict loop of manipulator.py:299-323 / visualizer.py:73-86
        assert np.array_equal(out["label"][i].cpu().numpy(), np.argmax(out["ins"][i].cpu().numpy(), -1))
        ins_map = {}
        for idx, m in enumerate(matched[:3].cpu().tolist()):
            if m != -1:
                ins_map[str(m)] = int(rows[idx])
        lab = out["label"][i].cpu()
        want = np.zeros((H, W, 3))
        for l in torch.unique(lab):
            if str(int(l)) in ins_map and str(ins_map[str(int(l))]) in color_dict:
                want[(lab == l).numpy()] = rgbs[color_dict[str(ins_map[str(int(l))])]]
        assert np.array_equal(out["ins_img"][i].cpu().numpy(), want.astype(np.uint8))
        want_gt = np.zeros((H, W, 3))
        for l in torch.unique(gt_labels[i]):                                                  # visualizer.py:57-69
            if str(int(l)) in color_dict:
                want_gt[(gt_labels[i] == l).numpy()] = rgbs[color_dict[str(int(l))]]
        assert np.array_equal(out["gt_ins_img"][i].cpu().numpy(), want_gt.astype(np.uint8))
        assert want_gt.any()
    table = D.results_table(out)
    assert table.shape == (3, 9) and np.isnan(table[:, 2]).all() and np.isfinite(np.delete(table, 2, 1)).all()
    assert np.array_equal(table[:2, 0], out["psnr_f64"].cpu().numpy()) and np.array_equal(table[:2, 3:], out["ap"].double().cpu().numpy())
    # without ground truth: the two 8-bit frames only
    with torch.no_grad():
        bare = E.manipulate_eval_path(poses[:1], (H, W, K), _models(INS), a, trans)
    assert sorted(bare) == ["rgb8", "tar_rgb8"] and tuple(bare["rgb8"].shape) == (1, H, W, 3)
