"""tests/_optim_restate.py held against torch on the CPU: ``adam_f64`` against ``torch.optim.Adam`` on float64 parameters (fresh and
from a loaded state), the measured f32 class that tests/test_gpu_optim_edges.py carries as constants, ``head_product_f64`` against a
float64 matmul of the named tensors, and the argument refusals of ``dmnerf_adam_step`` / ``dmnerf_repack_train`` that return before
any launch (no device needed)."""
import ctypes

import numpy as np
import pytest
import torch

import _optim_restate as RS

REL64 = 1e-12


def _close64(got, want, grads):
    """1e-12 relative in the three measures of ``RS.deviation`` (float64 against float64)."""
    dev = RS.deviation(got, want, grads)
    assert dev["p"] <= REL64 and dev["m"] <= REL64 and dev["v"] <= REL64, dev


def test_adam_f64_equals_torch_adam_on_float64_parameters():
    named = RS.cases()
    assert set(named) == {"spread", "edges", "all_zero_first"} and all(named[k] is RS.case(k, RS.N_EDGE) for k in named)    # one copy
    p0, grads = named["spread"]
    assert len(grads) == 12
    decades = torch.stack(grads).abs()
    assert float(decades[decades > 0].min()) < 1e-6 and float(decades.max()) > 1.0           # six decades
    assert 0.03 < float((torch.stack(grads) == 0).float().mean()) < 0.07                     # ~5 % exact zeros
    _close64(RS.adam_f64(p0, grads), RS.torch_adam_cpu(p0, grads, torch.float64), grads)


def test_adam_f64_from_a_loaded_state_at_step_999():
    p0, grads = RS.case("spread")
    g = torch.Generator().manual_seed(5)
    m0 = 1e-2 * torch.randn(p0.numel(), generator=g)
    v0 = 1e-4 * torch.rand(p0.numel(), generator=g)
    own = RS.adam_f64(p0, grads[:5], t0=999, m0=m0, v0=v0)
    _close64(own, RS.torch_adam_cpu(p0, grads[:5], torch.float64, state=(999, m0, v0)), grads[:5])
    fresh = RS.adam_f64(p0, grads[:5])
    assert float(np.abs(own[0] - fresh[0]).max()) > 1e-4                                      # the loaded state is not ignored


def test_adam_f64_on_the_value_edges():
    """Everywhere except the two kinds of overflow element (|g| > 1e19: float64 keeps them finite, f32 does not)."""
    p0, grads = RS.case("edges")
    n = p0.numel()
    assert grads[RS.EDGE_STEP - 1][:8].tolist() == grads[RS.EDGE_STEP - 1][n - 8:].tolist()
    assert torch.equal(grads[RS.EDGE_STEP - 1][:8].view(torch.int32), torch.tensor(RS.EDGE_VALUES, dtype=torch.float32).view(torch.int32))
    over = RS.overflow_mask(grads)
    assert np.nonzero(over)[0].tolist() == [2, 3, n - 6, n - 5]
    own = RS.adam_f64(p0, grads)
    assert all(np.isfinite(x).all() for x in own)
    _close64(own, RS.torch_adam_cpu(p0, grads, torch.float64), grads)
    # single-tensor f32 Adam forms (value * g) * g and stays finite there; the multi-tensor form (g * g first) is the device twin
    single = RS.torch_adam_cpu(p0, grads, torch.float32)
    assert np.isfinite(single[2]).all()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e20) * np.float32(1e20))


def test_all_zero_gradients_on_zero_moments_move_nothing():
    p0, grads = RS.case("all_zero_first")
    p, m, v = RS.adam_f64(p0, grads[:2])
    assert np.array_equal(p, p0.double().numpy()) and not m.any() and not v.any()
    tp, tm, tv = RS.torch_adam_cpu(p0, grads[:2], torch.float32)
    assert np.array_equal(tp, p0.numpy()) and not tm.any() and not tv.any()
    _close64(RS.adam_f64(p0, grads), RS.torch_adam_cpu(p0, grads, torch.float64), grads)


def test_eps_zero_with_a_zero_gradient_on_zero_moments_is_nan():
    """0 / (sqrt(0) / c + 0): NaN in float64 as in torch's f32."""
    p0 = torch.tensor([0.5, -0.25])
    grads = [torch.tensor([0.0, 1e-3])]
    p, _, _ = RS.adam_f64(p0, grads, eps=0.0)
    tp, _, _ = RS.torch_adam_cpu(p0, grads, torch.float32, eps=0.0)
    assert np.isnan(p[0]) and np.isnan(tp[0]) and np.isfinite(p[1]) and np.isfinite(tp[1])


def test_f32_class_constants_of_the_gpu_file(capsys):
    """The three constants at the top of tests/test_gpu_optim_edges.py are this measurement (worst over ``gpu_adam_cases``),
    rounded up to three digits.  Re-measured here so they cannot drift from the committed cases; another CPU's vector units
    may round torch's float32 chain differently (the same class, not the same rounding), hence a band and not equality."""
    import test_gpu_optim_edges as G
    worst = dict(p=0.0, m=0.0, v=0.0)
    for name, n in RS.gpu_adam_cases():
        dev = RS.f32_class(name, n)
        worst = {k: max(worst[k], dev[k]) for k in worst}
    with capsys.disabled():
        print(f"\n[f32 class of Adam, torch CPU float32 vs adam_f64] |dp| / (|p| + 1e-3) {worst['p']:.3e}, |dm| / max|g| {worst['m']:.3e}, "
              f"|dv| / v {worst['v']:.3e}")
    for k, const in (("p", G.F32_P), ("m", G.F32_M), ("v", G.F32_V)):
        assert 0.5 * const <= worst[k] <= 1.5 * const, (k, worst[k], const)


@pytest.mark.parametrize("ins_num", RS.REPACK_INS)
def test_head_product_f64_is_the_matmul_of_the_two_named_tensors(ins_num):
    from dm_nerf_amd.networks.dm_nerf import DM_NeRF
    from oracle import ref_cpu as O
    m = DM_NeRF(8, 256, 63, 27, [4], ins_num)
    m.load_state_dict(O.make_weights(RS.REPACK_SEED[ins_num], ins_num, gain=1.7, sigma_bias=0.3))
    named = dict(m.named_parameters())
    want = named["rgb_feature_linears.0.weight"].detach().double()[:, :256] @ named["rgb_feature_linear.weight"].detach().double()
    got = RS.head_product_f64(RS.repack_flat(ins_num), ins_num)
    assert got.shape == (128, 256) and np.array_equal(got, want.numpy())
    assert float(np.abs(got).max()) > 0.1


def test_head_product_f32_class_constant_of_the_gpu_file(capsys):
    import test_gpu_optim_edges as G
    worst = max(RS.head_product_f32_class(i) for i in RS.REPACK_INS)
    with capsys.disabled():
        print(f"\n[f32 class of the head product, CPU float32 matmul vs float64] max |error| / max |F| {worst:.3e}")
    assert 0.5 * G.F32_HEAD <= worst <= 1.5 * G.F32_HEAD, (worst, G.F32_HEAD)


ONE = ctypes.c_void_p(64)                  # a non-null address that is never dereferenced: every call below returns before a launch


def _adam(lib, p=ONE, g=ONE, m=ONE, v=ONE, n=8, lr=5e-4, d_lr=None, b1=0.9, b2=0.999, eps=1e-8, state=ONE):
    return lib.dmnerf_adam_step(p, g, m, v, n, lr, d_lr, b1, b2, eps, state, None)


def test_adam_step_refuses_bad_arguments_without_a_device():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    assert _adam(lib, n=-1) == -1 and "n = -1" in _lib.last_error()
    for which in ("p", "g", "m", "v", "state"):
        assert _adam(lib, **{which: None}) == -1 and "null" in _lib.last_error(), which
    for b1 in (1.0, -0.1, 1.5, float("nan")):
        assert _adam(lib, b1=b1) == -1 and "out of range" in _lib.last_error(), b1
    for b2 in (1.0, -0.1, 1.5, float("nan")):
        assert _adam(lib, b2=b2) == -1 and "out of range" in _lib.last_error(), b2
    for eps in (-1e-8, float("nan")):
        assert _adam(lib, eps=eps) == -1 and "out of range" in _lib.last_error(), eps
    for b1 in (0.5, 0.3, 0.0):
        assert _adam(lib, b1=b1) == -1 and "lerp" in _lib.last_error(), b1
    assert _adam(lib, n=0) == 0
    assert _adam(lib, p=None, g=None, m=None, v=None, state=None, n=0) == 0                 # n == 0: nothing is looked at


def _repack_model(ins_num=13, flat=64, copy=128, idx=192, blob=256, idx_t=320, blob_t=384, f_pos=None):
    from dm_nerf_amd import _lib
    return _lib.RepackModel(flat, ins_num, copy, idx, blob, idx_t, blob_t, f_pos)


def test_repack_train_refuses_bad_arguments_without_a_device():
    from dm_nerf_amd import _lib
    lib = _lib.load()
    arr = (_lib.RepackModel * 5)(*[_repack_model() for _ in range(5)])
    for n_models in (0, 5, -1):
        assert lib.dmnerf_repack_train(arr, n_models, None) == -1 and f"got {n_models}" in _lib.last_error(), n_models
    assert lib.dmnerf_repack_train(None, 1, None) == -1
    for ins_num in (0, 128, -3):
        arr[0] = _repack_model(ins_num=ins_num)
        assert lib.dmnerf_repack_train(arr, 1, None) == -1 and f"ins_num {ins_num}" in _lib.last_error(), ins_num
    for which in ("flat", "idx", "blob", "idx_t", "blob_t"):
        arr[0] = _repack_model(**{which: None})
        assert lib.dmnerf_repack_train(arr, 1, None) == -1 and "null" in _lib.last_error(), which
    arr[0] = _repack_model(copy=64)
    assert lib.dmnerf_repack_train(arr, 1, None) == -1 and "aliases" in _lib.last_error()
    arr[0] = _repack_model()
    arr[1] = _repack_model(blob=None)                                   # a later model of the launch is checked too
    assert lib.dmnerf_repack_train(arr, 2, None) == -1 and "null" in _lib.last_error()
