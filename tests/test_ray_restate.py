"""The float64 restatement of the per-ray stages (tests/_ray_restate.py) that tests/test_gpu_ray_edges.py compares the kernels
against, held on the CPU to the oracle (oracle/ref_cpu.py, evaluated in float64 and in float32) and to the committed fixtures of
the reference; then, for every edge case the GPU test runs: the float32 oracle and the restatement are finite, and the oracle's own
error against float64 -- the yardstick of the GPU test's tolerance -- is recorded and is small enough to measure with."""
import pytest
import torch

import _ray_restate as RR
from oracle import ref_cpu as O


# ------------------------------------------------------------------------------------------
# the restatement against the oracle and the fixtures
# ------------------------------------------------------------------------------------------
def test_render_train_matches_oracle_and_fixture(golden):
    g = golden("render_train")
    for k in ("S64_C14", "S192_C14", "S320_C60", "S192_C94", "S5_C3", "kat"):
        raw, z, d = g[f"{k}_raw"], g[f"{k}_z"], g[f"{k}_d"]
        got = RR.render_train(raw, z, d)
        o64 = O.render_train(raw.double(), z.double(), d.double())
        for name, a, b in zip(("rgb", "w", "depth", "ins"), got, o64):
            # (the oracle forms 1 - (1 - e) + 1e-10 where the restatement forms e + 1e-10: one float64 rounding of 1 apart)
            assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max())), (k, name)
        for name, a in zip(("rgb", "w", "depth", "ins"), got):
            want = g[f"{k}_{name}"].double()
            assert float((a - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max())), (k, name)


def test_render_train_gradients_match_oracle_f64():
    for S, C, seed in ((64, 14, 1), (70, 3, 2), (5, 94, 3)):
        gen = torch.Generator().manual_seed(seed)
        N = 5
        raw = torch.randn(N, S, 4 + C, generator=gen)
        raw[0, S // 2, 3] = 50.0
        z = torch.sort(torch.rand(N, S, generator=gen) * 11 + 4, -1)[0]
        d = torch.randn(N, 3, generator=gen)
        ct = [torch.randn(N, 3, generator=gen), torch.randn(N, S, generator=gen), torch.randn(N, generator=gen), torch.randn(N, C - 1, generator=gen)]
        got = RR.render_train_grads(raw, z, d, ct)
        for name, which in RR.cotangent_sets(ct).items():
            r = raw.double().requires_grad_(True)
            want, = torch.autograd.grad(RR.composite_loss(O.render_train(r, z.double(), d.double()), ct, which), r)
            assert float((got[name] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (S, C, name)
        assert float(got["ins"][..., :4].abs().max()) == 0.0       # the object-code path is detached from the density


def test_sampling_matches_oracle_and_fixture(golden):
    g = golden("sample_pdf")
    bins, w, cdf = g["bins"], g["w"], g["cdf"]
    assert float((RR.cdf_from_weights(w) - cdf.double()).abs().max()) <= 2.4e-7
    RR.check_cdf(cdf, w, "fixture cdf")
    for u_key, s_key, i_key in (("u_det", "s_det", "inds_det"), ("u_rnd", "s_rnd", "inds_rnd")):
        s, inds = RR.sample_tail(bins, cdf, g[u_key])
        assert torch.equal(inds, g[i_key])
        assert torch.equal(inds, O.sample_from_cdf(bins, cdf, g[u_key].expand(bins.shape[0], -1))[1])
        RR.check_samples(g[s_key], g[i_key], bins, cdf, g[u_key], "fixture " + s_key)     # the reference's float32 samples, every one
        s64, _ = O.sample_from_cdf(bins.double(), cdf.double(), g[u_key].double().expand(bins.shape[0], -1))
        assert float((s - s64).abs().max()) <= 1e-12


def test_penalizer_matches_oracle_and_fixture(golden):
    g = golden("penalizer")
    for k in ("S64_C14", "S192_C14", "S192_C60"):
        raw, z, depth, d, tol = g[f"{k}_raw"], g[f"{k}_z"], g[f"{k}_depth"], g[f"{k}_d"], float(g[f"{k}_tol"])
        loss, grad = RR.emptiness_penalizer_grad(raw, z, depth, d, tol=tol)
        r = raw.double().requires_grad_(True)
        l64 = O.emptiness_penalizer(r, z.double(), depth.double()[:, None], d.double(), tol, RR.DETA_W).sum()
        g64, = torch.autograd.grad(l64, r)
        # (the oracle divides by 1-element float32 tensors, which makes its two quotients float32 whatever the inputs are:
        # one float32 rounding each, in the loss and as a common factor of the gradient)
        assert abs(float(loss) - float(l64.detach())) <= 2.4e-7 * abs(float(loss)), k
        assert float((grad - g64).abs().max()) <= 2.4e-7 * float(g64.abs().max()), k
        assert abs(float(loss) - float(g[f"{k}_loss"])) <= 2e-6 * abs(float(loss)), k
        want = g[f"{k}_grad"].double()
        assert float((grad[..., 4:] - want).abs().max()) <= 2e-5 * float(want.abs().max()), k      # (the GPU golden test's bound)
        assert float(grad[..., :4].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------
# the edge cases of the GPU test: finite in float32 and float64, and the yardstick
# ------------------------------------------------------------------------------------------
# The GPU test allows 4 x the float32 oracle's error + 8 ulp of the ray's scale.  That only measures the kernel if the oracle's
# error is itself of float32 rounding size: a float32 evaluation of these formulas makes a handful of roundings per element and
# sums S <= 1280 of them pairwise, so 64 ulp of the (floored) scale is generous for a well-conditioned input and far below any
# structural mistake (a wrong term is of the order of the scale itself).
YARDSTICK_ULP = 64.0
# The penalizer is the exception, by the reference's own arithmetic: its Gaussian takes depth |d| - z |d|, the float32 difference
# of two float32 products of size ~10 that are 0.01 ... 1 apart, so the float32 exponent (difference^2 / 0.005) carries a relative
# error of up to ~1e-3 where the Gaussian matters.  The kernels keep these operations, so the oracle's error is the right
# yardstick; here it only has to stay far below the scale (a structural mistake is of the order of the scale).
YARDSTICK_PEN_REL = 1e-2


def _yardstick(want, o32, what, worst, limit_ulp=YARDSTICK_ULP, limit_rel=None):
    if want.numel() == 0:
        return
    assert bool(torch.isfinite(want).all()), (what, "restatement not finite")
    assert bool(torch.isfinite(o32).all()), (what, "float32 oracle not finite")
    _, err_o, scale = RR.bound(want, o32)
    ulps = float(torch.where(scale > 0, err_o / RR.ulp32(scale).clamp(min=1e-300), err_o * 0).max())
    rel = float(torch.where(scale > 0, err_o / scale.clamp(min=1e-300), err_o * 0).max())
    worst[what.split(" ")[-1]] = max(worst.get(what.split(" ")[-1], 0.0), rel)
    if limit_rel is None:
        assert ulps <= limit_ulp, (what, ulps, err_o.tolist(), scale.tolist())
    else:
        assert rel <= limit_rel, (what, rel, err_o.tolist(), scale.tolist())
    RR.zeros_kept(o32, want, what)             # where float64 is exactly 0 the float32 oracle is too: the GPU test may ask the same


@pytest.mark.parametrize("S,C,batch", RR.composite_case_ids())
def test_composite_edge_cases_finite_and_yardstick(S, C, batch):
    ref = RR.composite_reference(S, C, batch, O)
    worst = {}
    for name, want, o32 in zip(("rgb", "w", "depth", "ins"), ref["want"], ref["o32"]):
        _yardstick(want, o32, f"{ref['name']} {name}", worst)
    for cot in ref["want_g"]:
        for grp, want in RR.d_raw_groups(ref["want_g"][cot]).items():
            _yardstick(want, RR.d_raw_groups(ref["o32_g"][cot])[grp], f"{ref['name']} d_raw[{cot}].{grp}", worst)
    kinds = ref["kinds"]
    for i, kind in enumerate(kinds):
        if kind in ("empty", "zero_dir"):                                   # nothing is composited: every output and gradient is 0
            assert all(float(t[i].abs().max()) == 0 for t in ref["want"][:3])
            assert float(ref["want_g"]["all"][i][..., :4].abs().max()) == 0
    assert float(ref["want_g"]["ins"][..., :4].abs().max()) == 0
    print(f"{ref['name']} {kinds}: float32 oracle's error / scale, worst ray: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("S,C,batch", RR.pen_case_ids())
def test_penalizer_edge_cases_finite_and_yardstick(S, C, batch):
    ref = RR.pen_reference(S, C, batch, O)
    worst = {}
    _yardstick(ref["want_loss"].reshape(1, 1), ref["o32_loss"].reshape(1, 1), f"{ref['name']} loss", worst, limit_rel=YARDSTICK_PEN_REL)
    _yardstick(ref["want_grad"], ref["o32_grad"], f"{ref['name']} d_raw", worst, limit_rel=YARDSTICK_PEN_REL)
    assert float(ref["want_grad"][..., :4].abs().max()) == 0
    print(f"{ref['name']}: float32 oracle's error / scale: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("nb,batch", RR.sample_case_ids())
def test_sampling_edge_cases_finite(nb, batch):
    case = RR.sample_case(nb, batch)
    bins, w = case["bins"], case["w"]
    assert bool(torch.isfinite(bins).all() and torch.isfinite(w).all())
    _, cdf, _ = O.sample_pdf(bins, w, 1, u=torch.zeros(bins.shape[0], 1), return_aux=True)
    RR.check_cdf(cdf, w, case["name"] + " oracle", strict=False)
    cand = RR.u_candidates(cdf, nb)
    worst = 0.0
    for n in RR.SAMPLE_N:
        for u in RR.u_chunks(cand, n)[:: 1 if n == 128 else 7]:
            s, inds = O.sample_from_cdf(bins, cdf, u)
            worst = max(worst, RR.check_samples(s, inds, bins, cdf, u, f"{case['name']} n={n}"))
    print(f"{case['name']}: float32 oracle's samples within {worst:.2f} ulp of max|bins| of the float64 evaluation")


@pytest.mark.parametrize("S,n_imp", RR.RESAMPLE_SHAPES)
def test_resample_edge_cases_finite(S, n_imp):
    case = RR.resample_case(S, n_imp)
    z, w = case["z"], case["w"]
    mid = .5 * (z[:, 1:] + z[:, :-1])
    _, cdf, _ = O.sample_pdf(mid, w[:, 1:-1], 1, u=torch.zeros(z.shape[0], 1), return_aux=True)
    u = RR.resample_u(case, cdf)
    assert u.shape == (z.shape[0], n_imp)
    s, inds = O.sample_from_cdf(mid, cdf, u)
    RR.check_samples(s, inds, mid, cdf, u, case["name"])
    # the case does what it is for: samples of the all-zero-weight ray with repeated depths land exactly on coarse depths
    hits = (s[0][:, None] == z[0][None, :]).any(-1)
    assert int(hits.sum()) >= 1, case["name"]


@pytest.mark.parametrize("K", RR.SORT_K)
def test_sort_cases(K):
    x = RR.sort_case(K)
    assert x.shape == (7, K) and not bool(torch.isnan(x).any())
    assert RR.sort_case(K, 5).shape == (5, K)
