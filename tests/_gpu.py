"""What the GPU tests (tests/test_gpu_*.py) share: one namespace of project modules under one vocabulary (fixture ``A``), the model
builders, the benchmark camera's rays, the random skip grid and three comparison helpers.  A plain module next to the ``_*_restate.py``
ones (``import _gpu``), importable without a device; tests/test_gpu_helpers_host.py holds the builders to the constructions they
replaced.  Nothing here caches: a file that keeps models for its lifetime passes its own dict as ``cache=``."""
import types

import numpy as np
import pytest
import torch

import _skip_restate as RS
from oracle import ref_cpu as O

NAMES = ("M", "H", "R", "MA", "E", "P", "D", "F", "Ed", "Cfg", "G", "graphed", "L", "lib", "Gen", "Lo")


def namespace():
    """The project's modules under the letters every GPU test uses; ``L`` is the ``_lib`` module, ``lib`` the loaded library."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from dm_nerf_amd import _lib, autograd, config, distributed, editing, field, generic, graphed, losses
    from dm_nerf_amd.networks import dm_nerf, evaluator, helpers, manipulator, penalizer, render
    return types.SimpleNamespace(M=dm_nerf, H=helpers, R=render, MA=manipulator, E=evaluator, P=penalizer, D=distributed, F=field,
                                 Ed=editing, Cfg=config, G=autograd, graphed=graphed, L=_lib, lib=_lib.load(), Gen=generic, Lo=losses)


@pytest.fixture(scope="module")
def A():
    return namespace()


# ---- models
def model_from(sd, ins_num, D=8, W=256, train=False, device="cuda"):
    """A ``DM_NeRF(D, W, 63, 27, [4], ins_num)`` holding ``sd`` (None: as the constructor initialised it) on ``device``, in train or
    eval mode."""
    from dm_nerf_amd.networks import dm_nerf
    m = dm_nerf.DM_NeRF(D, W, 63, 27, [4], ins_num)
    if sd is not None:
        m.load_state_dict(sd)
    m = m.to(device)
    return m.train() if train else m.eval()


def models(ins_num=13, D=8, W=256, seeds=(61, 62), gain=1.7, sigma_bias=0.3, train=False, state_dicts=None, device="cuda", cache=None):
    """The coarse and the fine model with the oracle's synthetic weights of ``seeds`` (or with ``state_dicts``).  With ``cache=`` (a
    dict the calling file owns) the list is built once per argument set; training tests and ``state_dicts=`` callers pass none."""
    assert cache is None or (not train and state_dicts is None), "only eval models of the synthetic weights are kept"
    key = (ins_num, D, W, tuple(seeds), gain, sigma_bias, device)
    if cache is not None and key in cache:
        return cache[key]
    sds = state_dicts if state_dicts is not None else [O.make_weights(s, ins_num, W=W, D=D, gain=gain, sigma_bias=sigma_bias) for s in seeds]
    out = [model_from(sd, ins_num, D, W, train, device) for sd in sds]
    if cache is not None:
        cache[key] = out
    return out


# ---- rays and grids
def frame_rays(n, start=0, stride=97, device="cuda"):
    """``n`` rays of the benchmark camera (640 x 480, ``pose_spherical(30, -65, 7)``): every ``stride``-th from ray ``start``."""
    K = O.dmsr_intrinsics(480, 640)
    ro, rd = O.get_rays_k(480, 640, K, O.pose_spherical(30.0, -65.0, 7.0))
    ro, rd = ro.reshape(-1, 3)[start:start + n * stride:stride], rd.reshape(-1, 3)[start:start + n * stride:stride]
    return ro.contiguous().to(device), rd.contiguous().to(device)


def renderer_rays(A, trans_list, target_labels, keep=None, *, camera, ins_num):
    """The ray sets ``preview_frame`` / ``render_preview`` use -- ``ManipulationFrameRenderer``'s own -- for ``camera = (H, W, K, pose)``:
    [1 + T, 2, H * W, 3].  (``frame_rays`` above is the dense render's camera; this is the edit previews'.)"""
    H, W, K, pose = camera
    args = types.SimpleNamespace(N_importance=0, target_labels=list(target_labels))
    fr = A.D.ManipulationFrameRenderer(H, W, K, torch.from_numpy(pose), trans_list, None, args, ins_num=ins_num, rank=0, world=1,
                                       keep_labels=keep if (keep is not None or trans_list) else ())
    return torch.cat([fr.ori[None], fr.tar], dim=0) if fr.T else fr.ori[None]


def words_of(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def random_words(dims, frac, seed):
    """The packed words of a random occupancy: about ``frac`` of the cells set."""
    return RS.pack_bits(np.random.RandomState(seed).rand(*dims) < frac)


def random_grid(dims, lo, hi, frac, seed, outside="evaluate"):
    from dm_nerf_amd import field
    return field.SkipGrid.from_bits(random_words(dims, frac, seed), lo, hi, dims, outside=outside)


# ---- comparisons
def cpu(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def maxrel(a, b):
    return float(((a - b).abs() / (1 + b.abs())).max())


def ulp32(x):
    return 2.0 ** (np.floor(np.log2(x)) - 23) if x > 0 else 0.0
