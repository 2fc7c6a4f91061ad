"""The numpy restatement of the reference's image scores (tests/_img_metrics_restate.py) that the GPU test compares against, checked
on the CPU: its two independent forms against each other, closed forms, the power of the tolerance, scikit-image itself wherever
it imports, ``distributed.results_table``, and the argument checks of the C entry on a host without a device."""
import numpy as np
import pytest

import _img_metrics_restate as RS


@pytest.fixture(scope="module")
def main_cases():
    return RS.main_cases()


@pytest.fixture(scope="module")
def shape_cases():
    return RS.shape_cases()


def test_two_forms_agree_on_every_gpu_input(main_cases, shape_cases):
    worst = 0.0
    for name, (a, b) in list(main_cases.items()) + list(shape_cases.items()):
        u, d = RS.ssim_channels_uniform(a, b), RS.ssim_channels_direct(a, b)
        worst = max(worst, float(np.abs(u - d).max()), abs(RS.ssim_uniform(a, b) - RS.ssim_direct(a, b)))
        assert np.abs(u - d).max() <= 1e-12, (name, u, d)
        assert abs(RS.ssim_uniform(a, b) - RS.ssim_direct(a, b)) <= 1e-12, name
    print(f"uniform_filter vs direct 49-term sums: max |delta SSIM| {worst:.2e}")


def test_identical_images(main_cases):
    a, b = main_cases["same"]
    assert RS.ssim_uniform(a, b) == 1.0 and RS.ssim_direct(a, b) == 1.0
    assert RS.psnr_restate(a, b) == float("inf") and RS.mse_restate(a, b) == 0.0


def test_constant_images_closed_form():
    for va, vb in ((0.3, 0.7), (0.0, 1.0), (0.25, 0.25)):
        a = np.full((20, 31, 3), va, dtype=np.float32)
        b = np.full((20, 31, 3), vb, dtype=np.float32)
        fa, fb = float(np.float32(va)), float(np.float32(vb))
        want = (2 * fa * fb + RS.C1) / (fa * fa + fb * fb + RS.C1)          # the variances vanish: the C2 factors cancel
        assert abs(RS.ssim_uniform(a, b) - want) <= 1e-12
        assert abs(RS.ssim_direct(a, b) - want) <= 1e-12
        d = np.float32(va) - np.float32(vb)
        want_mse = float(np.float32(d * d))
        assert abs(RS.mse_restate(a, b) - want_mse) <= 1e-15
        if want_mse:
            assert abs(RS.psnr_restate(a, b) - 10 * np.log10(1 / want_mse)) <= 1e-9


def test_single_window_by_hand():
    rng = np.random.default_rng(5)
    a = rng.random((7, 7, 2)).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1).astype(np.float32)
    per_channel = []
    for c in range(2):
        x, y = a[..., c].astype(np.float64).ravel(), b[..., c].astype(np.float64).ravel()
        ux, uy = x.sum() / 49, y.sum() / 49
        vx = ((x - ux) ** 2).sum() / 48                   # the sample variance: 49/48 (E[xx] - ux ux)
        vy = ((y - uy) ** 2).sum() / 48
        vxy = ((x - ux) * (y - uy)).sum() / 48
        per_channel.append(((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4)))
    want = (per_channel[0] + per_channel[1]) / 2
    assert abs(RS.ssim_uniform(a, b) - want) <= 1e-12
    assert abs(RS.ssim_direct(a, b) - want) <= 1e-12
    assert np.abs(RS.ssim_channels_direct(a, b) - np.array(per_channel)).max() <= 1e-12


def test_too_small_images_raise():
    a = np.zeros((6, 640, 3), dtype=np.float32)
    with pytest.raises(ValueError):
        RS.ssim_uniform(a, a)
    with pytest.raises(ValueError):
        RS.ssim_direct(a.transpose(1, 0, 2), a.transpose(1, 0, 2))


def test_power_of_the_tolerance(main_cases):
    """The GPU test's bound is 1e-9.  Two plausible wrong implementations are 100 times further than that from the definition on
    the main 480 x 640 input: float32 moments, and a map whose reflected border is counted."""
    a, b = main_cases["noise"]
    ref = RS.ssim_uniform(a, b)
    d_f32 = abs(RS.ssim_f32_moments(a, b) - ref)
    d_border = abs(RS.ssim_no_crop(a, b) - ref)
    print(f"f32 moments: |delta SSIM| {d_f32:.3e}; border counted: {d_border:.3e}")
    assert d_f32 > 1e-7
    assert d_border > 1e-7


def test_against_scikit_image_where_installed(main_cases, shape_cases):
    try:
        from skimage import metrics
    except ImportError as e:
        print(f"scikit-image does not import here ({e}): the comparison with the library itself is skipped; everything else in "
              f"this file ran")
        pytest.skip("scikit-image is not installed: the restatement was written without it")
    import inspect
    kw = {"channel_axis": -1} if "channel_axis" in inspect.signature(metrics.structural_similarity).parameters else {"multichannel": True}
    for name, (a, b) in list(main_cases.items()) + list(shape_cases.items()):
        want = metrics.structural_similarity(a, b, data_range=1, **kw)
        assert abs(RS.ssim_uniform(a, b) - want) <= 1e-12, (name, want)
        wp = metrics.peak_signal_noise_ratio(a, b, data_range=1)
        got = RS.psnr_restate(a, b)
        assert (got == wp) if np.isinf(wp) else abs(got - wp) <= 1e-9, (name, got, wp)


def test_results_table_layout():
    import torch
    from dm_nerf_amd import distributed as D
    P = 3
    out = {"psnr_f64": torch.tensor([30.0, 31.5, 29.25], dtype=torch.float64), "ssim": torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64),
           "ap": torch.arange(18, dtype=torch.float32).reshape(P, 6) / 32, "psnr": torch.zeros(P), "rgb": torch.zeros(P, 7, 7, 3)}
    t = D.results_table(out)
    assert isinstance(t, np.ndarray) and t.shape == (P + 1, 9) and t.dtype == np.float64
    assert np.array_equal(t[:P, 0], [30.0, 31.5, 29.25]) and np.array_equal(t[:P, 1], [0.9, 0.8, 0.7])       # PSNR, SSIM
    assert np.isnan(t[:, 2]).all()                                                                           # LPIPS
    assert np.array_equal(t[:P, 3:], out["ap"].double().numpy())                                             # AP50 .. AP95
    assert np.allclose(t[P, [0, 1]], [np.mean([30.0, 31.5, 29.25]), np.mean([0.9, 0.8, 0.7])], rtol=0, atol=1e-15)
    assert np.allclose(t[P, 3:], out["ap"].double().numpy().mean(0), rtol=0, atol=1e-15)
    t2 = D.results_table(out, lpips=[0.1, 0.2, 0.3])
    assert np.allclose(t2[:, 2], [0.1, 0.2, 0.3, 0.2], rtol=0, atol=1e-15)
    assert np.array_equal(np.delete(t2, 2, axis=1), np.delete(t, 2, axis=1))
    with pytest.raises(ValueError, match="ssim"):
        D.results_table({"psnr_f64": out["psnr_f64"], "ap": out["ap"]})
    with pytest.raises(ValueError, match="LPIPS"):
        D.results_table(out, lpips=[0.1])


def test_c_entry_validates_arguments_without_a_device():
    """As test_abi.py::test_host_only_calls_validate_arguments: argument errors come back before anything touches a device."""
    from dm_nerf_amd import _lib
    lib = _lib.load()
    assert lib.dmnerf_img_metrics_work_bytes(1, 480, 640, 3) == 30 * 20 * 4 * 8        # 16 x 32 windows per workgroup, C + 1 doubles
    assert lib.dmnerf_img_metrics_work_bytes(5, 7, 7, 1) == 5 * 2 * 8
    assert lib.dmnerf_img_metrics_work_bytes(0, 7, 7, 3) == 0
    for bad in ((1, 6, 640, 3), (1, 640, 6, 3), (1, 8, 8, 0), (1, 8, 8, 5), (-1, 8, 8, 3), (1, 40000, 8, 3)):
        assert lib.dmnerf_img_metrics_work_bytes(*bad) == -1, bad
    rc = lib.dmnerf_img_metrics(None, None, 1, 480, 640, 3, None, 0, None, None, None, None, None)
    assert rc == -1 and "null" in _lib.last_error()
    rc = lib.dmnerf_img_metrics(None, None, 1, 6, 640, 3, None, 0, None, None, None, None, None)
    assert rc == -1 and "H=6" in _lib.last_error()
    rc = lib.dmnerf_img_metrics(None, None, 1, 8, 8, 5, None, 0, None, None, None, None, None)
    assert rc == -1 and "C=5" in _lib.last_error()
    rc = lib.dmnerf_img_metrics(None, None, -1, 8, 8, 3, None, 0, None, None, None, None, None)
    assert rc == -1 and "P=-1" in _lib.last_error()
    assert lib.dmnerf_img_metrics(None, None, 0, 8, 8, 3, None, 0, None, None, None, None, None) == 0       # P == 0: nothing to do
    import ctypes
    one = ctypes.c_void_p(64)                           # a non-null address that is never dereferenced: the size check comes first
    rc = lib.dmnerf_img_metrics(one, one, 1, 480, 640, 3, one, 100, one, None, one, one, None)
    assert rc == -1 and "too small" in _lib.last_error()


def test_python_entry_refuses_what_the_device_cannot_score():
    import torch
    from dm_nerf_amd.networks import evaluator as E
    with pytest.raises(ValueError, match="device"):
        E.img_metrics_device(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match="device"):
        E.ssim(torch.zeros(8, 8, 3), torch.zeros(8, 8, 3))
