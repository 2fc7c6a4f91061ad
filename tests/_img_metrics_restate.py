"""numpy float64 restatement of the two image scores of ``render_test`` (networks/tester.py:89-90):

    skimage.metrics.peak_signal_noise_ratio(rgb, gt, data_range=1)
    skimage.metrics.structural_similarity(rgb, gt, multichannel=True, data_range=1)

written from the documented algorithm of scikit-image 0.18 (the version the reference pins) WITHOUT the library at hand;
tests/test_img_metrics_restate.py compares against the library wherever it imports.  Per channel, in float64: the 7x7 box means
``ux, uy, uxx, uyy, uxy`` of ``x, y, x x, y y, x y``; ``vx = 49/48 (uxx - ux ux)`` (sample covariance), ``vy``, ``vxy`` likewise;
``S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2))`` with ``C1 = 1e-4``, ``C2 = 9e-4``; the map is cropped by 3
on every side before the mean (only windows wholly inside the image count); the frame's SSIM is the mean over the channels.

Two independent forms of the box means:
  (a) ``ssim_uniform``: ``scipy.ndimage.uniform_filter(size=7)`` on the whole image, then the crop -- the calls skimage itself makes;
  (b) ``ssim_direct``:  the 49 terms of every window summed over ``numpy.lib.stride_tricks.sliding_window_view``.
Two deliberately WRONG variants show what the tests' tolerance can see: ``ssim_f32_moments`` (form (b) with the moments and the
map in float32) and ``ssim_no_crop`` (form (a) without the crop: the filter's reflected border counted)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view
from scipy.ndimage import uniform_filter

WIN = 7
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)


def _check(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.ndim != 3:
        raise ValueError("expected two [H, W, C] images of one shape")
    if a.shape[0] < WIN or a.shape[1] < WIN:
        raise ValueError("win_size exceeds image extent")
    return a, b


def _s_map(ux, uy, uxx, uyy, uxy, cov_norm=COV_NORM, c1=C1, c2=C2):
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))


def _box_direct(x):
    return sliding_window_view(x, (WIN, WIN)).sum(axis=(-1, -2)) / float(WIN * WIN)


def ssim_channels_uniform(a, b, crop=True):
    """Form (a) -> the per-channel means of S, float64 [C]."""
    a, b = _check(a, b)
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        S = _s_map(*(uniform_filter(t, size=WIN) for t in (x, y, x * x, y * y, x * y)))
        pad = (WIN - 1) // 2
        out.append((S[pad:S.shape[0] - pad, pad:S.shape[1] - pad] if crop else S).mean(dtype=np.float64))
    return np.array(out, dtype=np.float64)


def ssim_channels_direct(a, b):
    """Form (b) -> the per-channel means of S, float64 [C]."""
    a, b = _check(a, b)
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c].astype(np.float64), b[..., c].astype(np.float64)
        out.append(_s_map(*(_box_direct(t) for t in (x, y, x * x, y * y, x * y))).mean(dtype=np.float64))
    return np.array(out, dtype=np.float64)


def channel_mean(ch):
    """The frame's SSIM from the per-channel means: summed in channel order, divided by C (what the device computes, and what
    ``numpy.mean`` does for so few terms)."""
    s = 0.0
    for v in ch:
        s = s + float(v)
    return s / len(ch)


def ssim_uniform(a, b):
    return channel_mean(ssim_channels_uniform(a, b))


def ssim_direct(a, b):
    return channel_mean(ssim_channels_direct(a, b))


def ssim_no_crop(a, b):
    """WRONG on purpose: form (a) with the border of the filtered map (scipy's 'reflect' rule) counted in the mean."""
    return channel_mean(ssim_channels_uniform(a, b, crop=False))


def ssim_f32_moments(a, b):
    """WRONG on purpose: form (b) with float32 moments, constants and map (``uxx - ux ux`` cancels against C2 = 9e-4)."""
    a, b = _check(a, b)
    f = np.float32
    out = []
    for c in range(a.shape[-1]):
        x, y = a[..., c].astype(f), b[..., c].astype(f)
        m = [_box_direct(t).astype(f) for t in (x, y, x * x, y * y, x * y)]
        out.append(_s_map(*m, cov_norm=f(COV_NORM), c1=f(C1), c2=f(C2)).mean(dtype=np.float64))
    return channel_mean(out)


def mse_restate(a, b):
    """``np.mean((a - b) ** 2, dtype=np.float64)`` as skimage's mean_squared_error sees two float32 images: the difference and the
    square in float32, the sum in float64."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError("expected two images of one shape")
    return float(np.mean((a - b) ** 2, dtype=np.float64))


def psnr_restate(a, b):
    """``peak_signal_noise_ratio(a, b, data_range=1)``: ``10 log10(1 / mse)`` in float64, ``inf`` for identical images."""
    err = mse_restate(a, b)
    if err == 0.0:
        return float("inf")
    return float(10.0 * np.log10(1.0 / err))


# ---- the inputs of the GPU test (tests/test_gpu_img_metrics.py), generated from the analytic scene and seeded numpy ------------
SHAPES = ((7, 7, 3), (7, 9, 3), (9, 7, 3), (13, 640, 3), (123, 77, 3), (120, 160, 3), (123, 77, 1), (120, 160, 4))


def scene_view(H, W, theta=30.0):
    """One [H, W, 3] float32 view of oracle/analytic_scene.py."""
    from oracle import analytic_scene as S
    from oracle.ref_cpu import pose_spherical
    rgb, _ = S.render_view(H, W, pose_spherical(theta, -65.0, 7.0), 13)
    return np.ascontiguousarray(np.asarray(rgb, dtype=np.float32))


def with_channels(img, C, rng):
    """``img [H, W, 3]`` as a C-channel image: the first channels kept, a fourth made of a noisy mix."""
    if C <= 3:
        return np.ascontiguousarray(img[..., :C])
    extra = np.clip(img.mean(-1, keepdims=True) + rng.normal(0, 0.05, img.shape[:2] + (1,)), 0, 1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([img, extra], -1))


def main_cases(H=480, W=640):
    """The 480 x 640 x 3 pairs ``name -> (pred, gt)``: the view against itself plus (i) Gaussian noise of sd 0.02 clipped to
    [0, 1], (ii) a 1-pixel shift, (iii) a constant frame -- and against itself."""
    gt = scene_view(H, W)
    rng = np.random.default_rng(7)
    noise = np.clip(gt + rng.normal(0, 0.02, gt.shape), 0, 1).astype(np.float32)
    return {"noise": (noise, gt), "shift": (np.ascontiguousarray(np.roll(gt, 1, axis=1)), gt),
            "const": (np.full_like(gt, 0.3), gt), "same": (gt.copy(), gt)}


def shape_cases():
    """One noisy pair per entry of SHAPES: ``(H, W, C) -> (pred, gt)``."""
    out = {}
    for k, (H, W, C) in enumerate(SHAPES):
        rng = np.random.default_rng(100 + k)
        gt = with_channels(scene_view(H, W, theta=30.0 + 40.0 * k), C, rng)
        pred = np.clip(gt + rng.normal(0, 0.03, gt.shape), 0, 1).astype(np.float32)
        out[(H, W, C)] = (pred, gt)
    return out
