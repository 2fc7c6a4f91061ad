"""Host-side tests (no GPU) of dm_nerf_amd.editing: the deformation tables of ``manipulator_demo`` (networks/manipulator.py:381-382,
:397-426), the colour table of ``render_label2img``, the band arithmetic of the demo path with a ``Deform`` (the CPU oracle's ray
generator and a stand-in chunk renderer injected, as tests/test_distributed_gloo.py does), and the argument checks of the two
entries of csrc/edit_frame.hip."""
import types

import numpy as np
import pytest
import torch

from dm_nerf_amd import editing as E
from oracle import ref_cpu as O


def test_deform_offsets_at_known_points():
    r = np.arange(400, dtype=np.float64)
    assert np.array_equal(E.deform_offsets(400, "linear", 0), (r + 1 - 200) / 215)
    for view in (0, 3, 4, 7):
        assert np.array_equal(E.deform_offsets(400, "sin", view), np.zeros(400))
    assert np.array_equal(E.deform_offsets(400, "sin", 1), np.sin(((8 * np.pi) / 400) * (r + 1)) * 0.18)
    assert np.array_equal(E.deform_offsets(400, "sin", 5), np.sin(((8 * np.pi) / 400) * (r + 1)) * -0.18)
    assert np.array_equal(E.deform_offsets(10, "ex", 0), np.exp(-1 * (r[:10] + 1) / 50))
    assert np.array_equal(E.deform_offsets(10, "abs_linear", 0), np.abs(r[:10] + 1 - 200) / 200)
    assert np.array_equal(E.deform_offsets(10, "ln", 9), np.log((r[:10] + 1) / 200))      # (only sin reads deform_v)
    out = E.deform_offsets(7, "ex", 2)
    assert out.dtype == np.float64 and out.shape == (7,)
    with pytest.raises(IndexError):
        E.deform_offsets(400, "sin", 8)
    with pytest.raises(ValueError):
        E.deform_offsets(400, "cos", 0)
    with pytest.raises(ValueError):
        E.Deform("cos", 0)
    assert E.Deform("sin", 1) == E.Deform("sin", 1) and np.array_equal(E.Deform("ln", 3).offsets(5), E.deform_offsets(5, "ln", 3))


def test_label_lut_against_the_dict_loop():
    C = 8
    rgbs = np.random.RandomState(3).randint(0, 256, size=(13, 3))
    color_dict = {str(k): (5 * k) % 13 for k in range(13)}
    ins_map = {"0": 4, "1": 11, "2": 2, "4": 0, "6": 9, "7": 12, "9": 3}       # 3 and 5 missing; 7 = the last channel; 9 beyond C
    lut = E.label_lut(C, rgbs, color_dict, ins_map, device="cpu")
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (C, 3)
    want = np.zeros((C, 3))
    for label in range(C):                                                     # tools/visualizer.py:79-84
        if str(label) in ins_map.keys():
            want[label] = rgbs[color_dict[str(ins_map[str(label)])]]
    assert np.array_equal(lut.numpy(), want.astype(np.uint8))
    assert not lut[3].any() and not lut[5].any() and np.array_equal(lut[7].numpy(), rgbs[color_dict["12"]].astype(np.uint8))


MH, MW, MCHUNK, MINS, MIMP = 10, 12, 32, 5, 8          # 120 rays: chunks of 32, 32, 32 and a ragged 24 that straddle the bands


def _raygen(H_, W_, K, c2w, row0, nrows):
    o, d = O.get_rays_k(H_, W_, K, c2w)
    return o[row0:row0 + nrows].contiguous(), d[row0:row0 + nrows].contiguous()


def _mani_chunk_exact(ori, tars, models, args, us):
    """Single IEEE operations only (bitwise independent of which rows share a call), touching every input the driver routes --
    the origins of EVERY target among them."""
    C = MINS + 1
    mix = sum(u[:, :3] for u in us)
    org = sum(t[0] for t in tars)
    return (ori[0] + ori[1] * us[0][:, :3] + org, us[-1][:, :C] * ori[1][:, :1] + us[1][:, 1:C + 1] + org[:, :1],
            tars[-1][0] * mix + tars[-1][1], us[len(tars)][:, :C] - tars[0][1][:, 2:3] + tars[0][0][:, :1])


def _products(rgb, ins, lut):
    label = ins.argmax(-1)
    return (255 * rgb.clamp(0, 1)).to(torch.uint8), label, label.to(torch.uint8), lut[label]


def _demo(target_rays=None, **kw):
    K = O.dmsr_intrinsics(MH, MW)
    poses = [O.pose_spherical(75.0, -65.0, 7.0), O.pose_spherical(60.0, -60.0, 7.0)]
    objs = [dict(obj_name="a", tar_id=2, mani_mode="deform", deform_func="ex"),
            dict(obj_name="b", tar_id=4, mani_mode="translation"),
            dict(obj_name="c", tar_id=1, mani_mode="deform", deform_func="sin")]
    objs_trans = {"b": [dict(transformation=[[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])] * 2}
    gen = torch.Generator().manual_seed(77)                 # every rank owns an identically seeded generator, as on the device
    seen = []

    def draws(n, n_imp, count, dev):
        return [torch.rand(n, n_imp, generator=gen) for _ in range(count)]

    def chunk(ori, tars, models, args, us):
        seen.append(list(args.target_labels))
        return _mani_chunk_exact(ori, tars, models, args, us)
    args = types.SimpleNamespace(N_samples=8, N_importance=MIMP, near=4.0, far=15.0, N_test=MCHUNK)
    rgbs = np.arange(39).reshape(13, 3) * 6
    out = E.manipulate_demo_path(poses, (MH, MW, K), None, args, objs, objs_trans, rgbs, {str(k): k for k in range(13)},
                                 {"0": 1, "2": 7, "5": 3}, keep_maps=True, products=_products, raygen=_raygen, target_rays=target_rays,
                                 manipulate_chunk=chunk, draws=draws, ins_num=MINS, **kw)
    assert seen and all(s == [2, 4, 1] for s in seen)
    return out


def _offsets_by_band_row(H, W, K, poses, kinds, offsets, row0, nrows):
    """The mistake the absolute-row rule excludes: the offset table indexed by the row INSIDE the band."""
    import dm_nerf_amd.distributed as D
    shifted = np.zeros_like(offsets)
    shifted[:, row0:row0 + nrows] = offsets[:, :nrows]
    return D._target_rays_from(_raygen)(H, W, K, poses, kinds, shifted, row0, nrows)


def test_demo_path_bands_with_a_deform_concatenate_to_the_single_process_frame():
    whole = _demo(rank=0, world=1)
    assert whole["rgb8"].shape == (2, MH, MW, 3) and whole["mask"].dtype == torch.uint8 and whole["label"].shape == (2, MH, MW)
    assert whole["ins"].shape == (2, MH, MW, MINS + 1) and whole["ins_img"].shape == (2, MH, MW, 3)
    for world in (1, 3, 7):
        bands = [_demo(rank=r, world=world) for r in range(world)]
        for key, want in whole.items():
            got = torch.cat([b[key] for b in bands], 1)
            assert got.shape == want.shape and torch.equal(got, want), (world, key)
    # ... and the check has teeth: offsets indexed by the band's own rows give another frame as soon as a band starts below row 0
    assert torch.equal(_demo(target_rays=_offsets_by_band_row, rank=0, world=1)["rgb"], whole["rgb"])
    wrong = torch.cat([_demo(target_rays=_offsets_by_band_row, rank=r, world=3)["rgb"] for r in range(3)], 1)
    assert not torch.equal(wrong, whole["rgb"])


def test_matrices_only_take_the_unchanged_path():
    """Without a ``Deform`` and without ``target_rays=`` the renderer never builds an offset table: the target rays are the
    injected ray generator's, as before."""
    import dm_nerf_amd.distributed as D
    K = O.dmsr_intrinsics(MH, MW)
    pose = O.pose_spherical(75.0, -65.0, 7.0)
    trans = torch.tensor([[1., 0., 0., 0.3], [0., 1., 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]])
    args = types.SimpleNamespace(N_samples=8, N_importance=MIMP, near=4.0, far=15.0, N_test=MCHUNK, target_label=2)
    fr = D.ManipulationFrameRenderer(MH, MW, K, pose, [trans], None, args, raygen=_raygen, ins_num=MINS, rank=1, world=3)
    to, td = _raygen(MH, MW, K, D._matmul4_f32(trans, pose), *D.row_band(MH, 1, 3))
    assert torch.equal(fr.tar[0, 0], to.reshape(-1, 3)) and torch.equal(fr.tar[0, 1], td.reshape(-1, 3))
    mixed = D.ManipulationFrameRenderer(MH, MW, K, pose, [trans, E.Deform("ex", 0)], None, args, raygen=_raygen, ins_num=MINS, rank=1, world=3)
    assert torch.equal(mixed.tar[0], fr.tar[0]) and torch.equal(mixed.tar[1, 1], fr.ori[1])
    row0, nrows = D.row_band(MH, 1, 3)
    off = torch.from_numpy(E.deform_offsets(MH, "ex", 0)[row0:row0 + nrows]).repeat_interleave(MW)
    assert torch.equal(mixed.tar[1, 0, :, 0], (fr.ori[0, :, 0].double() + off).float())
    assert torch.equal(mixed.tar[1, 0, :, 1:], fr.ori[0, :, 1:])


def test_new_entries_refuse_null_arguments_without_a_device():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    assert lib.dmnerf_edit_rays(5, 7, None, None, None, 1, None, 0, 3, None, None) == -1 and "null" in _lib.last_error()
    import ctypes
    intr_a, poses_a = np.ones(5, np.float32), np.zeros(12, np.float32)          # (kept alive: the calls below get raw addresses)
    intr, poses = intr_a.ctypes.data, poses_a.ctypes.data
    kind = (ctypes.c_int * 1)(1)
    assert lib.dmnerf_edit_rays(5, 7, intr, poses, kind, 1, None, 0, 3, None, None) == -1            # no output, no offsets
    assert lib.dmnerf_edit_rays(5, 7, intr, poses, kind, 1, None, 3, 3, None, None) == -1            # rows outside the image
    assert lib.dmnerf_edit_rays(5, 7, intr, poses, kind, 9, None, 0, 3, None, None) == -1            # T > 8
    assert lib.dmnerf_edit_rays(5, 7, intr, poses, (ctypes.c_int * 1)(2), 1, None, 0, 3, None, None) == -1   # unknown kind
    assert lib.dmnerf_edit_products(None, 3, None, 0, 0, None, 4, None, None, None, None, None) == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_edit_products(None, 2, None, 0, 0, None, 4, None, None, None, None, None) == -1   # row stride < 3
    assert lib.dmnerf_edit_products(None, 3, poses, 130, 130, None, 4, None, None, None, None, None) == -1   # C > 129
    assert lib.dmnerf_edit_products(None, 3, poses, 4, 8, None, 4, None, None, None, None, None) == -1       # ins stride < C
    assert lib.dmnerf_edit_products(None, 3, None, 0, 0, None, -1, None, None, None, None, None) == -1
    assert lib.dmnerf_edit_products(None, 3, None, 0, 0, None, 0, None, None, None, None, None) == 0        # n == 0: a no-op
