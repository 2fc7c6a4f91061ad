"""CPU tests of tests/_gpu.py, the helpers the GPU tests share: each builder, on ``device="cpu"``, against the construction it
replaced, written out once here; the comparison helpers on hand cases; the namespace's vocabulary read from its source; and a scan
that no test_gpu_*.py has grown a private copy of a shared helper again."""
import ast
import glob
import inspect
import os

import numpy as np
import torch

import _gpu
import _skip_restate as RS
from oracle import ref_cpu as O

HERE = os.path.dirname(os.path.abspath(__file__))


def camera_rays():
    K = O.dmsr_intrinsics(480, 640)
    ro, rd = O.get_rays_k(480, 640, K, O.pose_spherical(30.0, -65.0, 7.0))
    return ro.reshape(-1, 3), rd.reshape(-1, 3)


def test_frame_rays_are_the_former_slices():
    ro, rd = camera_rays()
    n, start = 130, 90000
    got = _gpu.frame_rays(n, start=start, device="cpu")
    assert torch.equal(got[0], ro[start:start + n * 97:97]) and torch.equal(got[1], rd[start:start + n * 97:97])
    assert got[0].shape == (130, 3) and got[0].is_contiguous() and got[1].is_contiguous()
    n, start = 64, 4096
    got = _gpu.frame_rays(n, start, stride=1, device="cpu")
    assert torch.equal(got[0], ro[start:start + n]) and torch.equal(got[1], rd[start:start + n])
    assert torch.equal(_gpu.frame_rays(8, device="cpu")[1], rd[0:8 * 97:97])


def test_models_hold_the_oracle_weights():
    from dm_nerf_amd.networks import dm_nerf
    ms = _gpu.models(ins_num=13, device="cpu")
    assert len(ms) == 2
    for m, seed in zip(ms, (61, 62)):
        want = O.make_weights(seed, 13, gain=1.7, sigma_bias=0.3)
        got = m.state_dict()
        assert isinstance(m, dm_nerf.DM_NeRF) and not m.training and set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    assert all(m.training for m in _gpu.models(ins_num=13, train=True, device="cpu"))
    a, b = _gpu.models(ins_num=13, device="cpu"), _gpu.models(ins_num=13, device="cpu")
    assert a[0] is not b[0]                                            # nothing is kept unless the caller passes its own dict
    cache = {}
    a, b = _gpu.models(ins_num=5, device="cpu", cache=cache), _gpu.models(ins_num=5, device="cpu", cache=cache)
    assert a is b and len(cache) == 1 and _gpu.models(ins_num=5, sigma_bias=60.0, device="cpu", cache=cache) is not a
    sds = [O.make_weights(3, 13), O.make_weights(4, 13)]
    for m, sd in zip(_gpu.models(13, state_dicts=sds, device="cpu"), sds):
        assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)


def test_models_of_a_generic_shape():
    for m, seed in zip(_gpu.models(ins_num=13, D=4, W=128, device="cpu"), (61, 62)):
        want = O.make_weights(seed, 13, W=128, D=4, gain=1.7, sigma_bias=0.3)
        got = m.state_dict()
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert (m.D, m.W) == (4, 128) and not m._fused_ok()


def test_model_from_keeps_the_constructors_weights_without_a_state_dict():
    from dm_nerf_amd.networks import dm_nerf
    torch.manual_seed(3)
    want = dm_nerf.DM_NeRF(D=8, W=256, input_ch_pts=63, input_ch_views=27, skips=[4], ins_num=13).state_dict()
    torch.manual_seed(3)
    m = _gpu.model_from(None, 13, train=True, device="cpu")
    assert m.training and all(torch.equal(m.state_dict()[k], want[k]) for k in want)


def test_random_words():
    for dims, frac, seed in (((8, 8, 8), 0.4, 11), ((9, 11, 10), 0.25, 3)):
        want = RS.pack_bits(np.random.RandomState(seed).rand(*dims) < frac)
        assert np.array_equal(_gpu.random_words(dims, frac, seed), want)
    assert "random_words(dims, frac, seed)" in inspect.getsource(_gpu.random_grid)


def test_ulp32_and_maxrel():
    assert _gpu.ulp32(1.0) == 2.0 ** -23 and _gpu.ulp32(1.5) == 2.0 ** -23 and _gpu.ulp32(2.0 ** -130) == 2.0 ** -153
    assert _gpu.ulp32(0) == 0.0 and _gpu.ulp32(0.0) == 0.0 and _gpu.ulp32(-1.0) == 0.0
    assert _gpu.maxrel(torch.tensor([1.0, -3.0]), torch.tensor([1.5, 1.0])) == 2.0         # max(0.5 / 2.5, 4 / 2)


def test_namespace_vocabulary():
    """Read from the source: calling it needs a device."""
    call = next(n for n in ast.walk(ast.parse(inspect.getsource(_gpu.namespace))) if isinstance(n, ast.Call) and ast.unparse(n.func) == "types.SimpleNamespace")
    got = {k.arg: ast.unparse(k.value) for k in call.keywords}
    assert got == {"M": "dm_nerf", "H": "helpers", "R": "render", "MA": "manipulator", "E": "evaluator", "P": "penalizer", "D": "distributed",
                   "F": "field", "Ed": "editing", "Cfg": "config", "G": "autograd", "graphed": "graphed", "L": "_lib", "lib": "_lib.load()",
                   "Gen": "generic", "Lo": "losses"}
    assert tuple(got) == _gpu.NAMES
    assert '"GPU tests need a MI355X"' in inspect.getsource(_gpu.namespace)


def test_no_gpu_test_file_defines_a_shared_helper():
    shared = {"cpu", "maxrel", "ulp32", "model_from", "words_of", "random_grid"}
    files = sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py")))
    assert len(files) > 40
    for path in files:
        tree = ast.parse(open(path).read())
        found = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)} & shared
        assert not found, (os.path.basename(path), found)
