"""GPU tests (-m gpu) of the per-ray kernels of csrc/render_kernels.hip -- compositing forward / backward, the weights-only pass,
the fused compositing + penalizer passes, the stand-alone penalizer, sample_pdf / sample_from_cdf / importance_resample and
sort_rows -- against the float64 restatement of tests/_ray_restate.py, on saturated, empty and odd-shaped rays.

Inputs (generated in tests/_ray_restate.py; tests/test_ray_restate.py runs the same tensors through the float32 oracle on the CPU):
every compositing shape of S in {1, 2, 5, 63, 64, 65, 129, 1280} x C in {1, 2, 17, 28, 29, 60, 61, 94, 128} that was kept gets rays
with sigma dist > 104 (expf returns 0) at a middle sample, at two consecutive samples, at sample 0 and (S >= 65) at samples 63 and 64,
sigma dist in 20 ... 80 (alpha rounds to 1, exp is not 0), all sigma <= 0 with one exactly 0, sigma > 0 only at the last sample,
rays_d = 0, two equal neighbouring z and rgb logits of +-90; N = 5 and N = 5 | 6 rays, the hardest alone in the partial block.

Tolerance: per ray and per output (d raw also per channel group rgb | sigma | ins) the kernel's error against float64 is at most
4 x the float32 oracle's error on the same ray and group + 8 float32 ulp of the group's scale (max |want| of the ray's group,
floored at 1e-3 of the group's maximum over the case); where the restatement is exactly 0 the kernel is exactly 0.  No ray,
sample or channel is left out of any comparison.  At S = 1 the reference keeps no sample at all (its ``expand`` of the last
distance yields weights of shape [N, 0]); there the kernels' one sample of length 1e10 |d| is compared with the restatement's,
and the float32 yardstick is the float32 evaluation of the restatement's formulas.

OBSERVED on an MI355X, per case family: the largest kernel error in float32 ulp of the ray's scale [the float32 oracle's own on
the same inputs, from tests/test_ray_restate.py], and the largest multiple of the oracle's error a ray needed on top of the 8 ulp
(the rule allows 4; the module prints both figures per family when it finishes).  The worst rays are those whose error is set by
the float32 rounding of sigma dist itself, which kernel and oracle share: there the two figures coincide.
  composite forward        15.6 ulp  [15.6],  every ray within 4 x + 8 ulp
  composite backward rgb   17.6 ulp  [17.6],  every ray within 4 x + 8 ulp
  composite backward sigma 30.4 ulp  [30.4],  every ray within 4 x + 8 ulp
  composite backward ins   17.0 ulp  [17.0],  every ray within 4 x + 8 ulp
  penalizer loss           93.9 ulp  [94.4],  penalizer backward 1738 ulp [1739]: the reference's float32 Gaussian of
                           depth |d| - z |d| (tests/test_ray_restate.py), which the kernel reproduces: at most 2.0 x the oracle's error
  sampling                 cdf 8.4e-8 (bound 2.4e-7), samples 1.27 ulp of max|bins| (bound 4), indices exact
  importance_resample, sort_rows, weights_from_sigma, fused pen forward / backward: exact, as asserted
ONE FAMILY NEEDED MORE THAN 4 before csrc/render_kernels.hip was changed: the compositing weights at S = 1280 (case S1280_C17_b,
the ray with two equal depths): 47 ulp of the ray's largest weight from float64 where the oracle is 8 ulp away (5.0 x the oracle's
error + 8 ulp).  Cause: the transmittance is a product of up to 1280 factors exp(-sigma dist), and the device expf (1 ulp) errs more
than ATen's (almost always the correctly rounded float); the error of the factors adds up along the ray.  The compositing kernels
now round exp once through double (expf_rn); on the CPU the same arithmetic lands 7.7 ulp away on that ray.
Also exposed: C = 1 (an object-code map of width 0) was refused by the C entry points as a null pointer; they accept it now.
"""

import pytest
import torch

import _gpu
import _ray_restate as RR
from _gpu import cpu
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

STATS = {}


@pytest.fixture(scope="module")
def A():
    yield _gpu.namespace()
    for fam, st in STATS.items():
        print(f"\n[ray edges] {fam}: needs {st.get('ratio', 0.0):.2f} x the oracle's error + 8 ulp, largest error {st.get('ulps', 0.0):.2f} ulp of the scale"
              + (f", largest cdf error {st['cdf']:.2e}" if "cdf" in st else ""))


def stats(family):
    return STATS.setdefault(family, {})


# ------------------------------------------------------------------------------------------
# compositing
# ------------------------------------------------------------------------------------------
OUT = ("rgb", "w", "depth", "ins")


def _grad(A, ref, which, fn=None):
    raw = ref["raw"].cuda().requires_grad_(True)
    outs = (fn or A.R.render_train)(raw, ref["z"].cuda(), ref["d"].cuda())
    g, = torch.autograd.grad(RR.composite_loss(outs[:4], ref["ct"], which), raw)
    return cpu(g)


@pytest.mark.parametrize("S,C,batch", RR.composite_case_ids())
def test_composite_vs_float64(A, S, C, batch):
    ref = RR.composite_reference(S, C, batch, O)
    name = ref["name"]
    raw, z, d = ref["raw"].cuda(), ref["z"].cuda(), ref["d"].cuda()
    with torch.no_grad():
        got = [cpu(t) for t in A.R.render_train(raw, z, d)]
    for o, g, want, o32 in zip(OUT, got, ref["want"], ref["o32"]):
        RR.compare(g, want, o32, f"{name} {o}", stats("composite forward"))
    # the training forward (the autograd Function) writes the same floats
    tr = A.R.render_train(ref["raw"].cuda().requires_grad_(True), z, d)
    for o, g, t in zip(OUT, got, tr):
        assert torch.equal(cpu(t), g), (name, o, "training forward != inference forward")
    # backward: cotangents on all four outputs, on rgb + ins only, on ins only
    for cot, which in RR.cotangent_sets(ref["ct"]).items():
        g = _grad(A, ref, which)
        for grp, part in RR.d_raw_groups(g).items():
            RR.compare(part, RR.d_raw_groups(ref["want_g"][cot])[grp], RR.d_raw_groups(ref["o32_g"][cot])[grp],
                       f"{name} d_raw[{cot}].{grp}", stats(f"composite backward, {grp}"))
        if cot == "ins":                                                    # the object-code path is detached from the density
            assert float(g[..., :4].abs().max()) == 0.0, name
    # the weights-only pass on the same density: the compositing weights bit for bit
    L = A.L
    sigma = raw[..., 3].contiguous()
    w = torch.full((raw.shape[0], S), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.load().dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z), L.ptr(d), raw.shape[0], S, L.ptr(w), L.stream()), "dmnerf_weights_from_sigma")
    assert torch.equal(cpu(w), got[1]), (name, "weights_from_sigma != compositing weights")


@pytest.mark.parametrize("S,C,batch", RR.composite_case_ids())
def test_fused_pen_equals_standalone(A, S, C, batch):
    """CompositePenFunction (compositing + the penalizer's partial sums in one pass, the penalizer's gradient added inside the
    backward kernel) against the stand-alone compositing and penalizer kernels plus autograd's add: bit for bit."""
    ref = RR.composite_reference(S, C, batch, O)
    name = ref["name"]
    z, d = ref["z"].cuda(), ref["d"].cuda()
    k2w, kh = A.P._consts(RR.DETA_W)
    consts = (RR.TOL, k2w, kh)
    assert (k2w, kh) == RR.pen_consts()
    for cot, which in (("all", (0, 1, 2, 3)), ("rgb_ins", (0, 3))):
        r1 = ref["raw"].cuda().requires_grad_(True)
        f = A.G.CompositePenFunction.apply(r1, z, d, consts)
        pen_f = A.P._PenalizerFromPartials.apply(f[4], C, False)
        g1, = torch.autograd.grad(RR.composite_loss(f[:4], ref["ct"], which) + pen_f.sum() * 1.5, r1)
        r2 = ref["raw"].cuda().requires_grad_(True)
        s = A.R.render_train(r2, z, d)
        pen_s = A.P.emptiness_penalizer(r2, z, s[2].detach()[..., None], d, RR.TOL, RR.DETA_W)
        g2, = torch.autograd.grad(RR.composite_loss(s, ref["ct"], which) + pen_s.sum() * 1.5, r2)
        for o, a, b in zip(OUT, f[:4], s):
            assert torch.equal(cpu(a), cpu(b)), (name, o, "fused forward != stand-alone")
        assert bool(torch.isfinite(cpu(pen_f)).all()) and torch.equal(cpu(pen_f), cpu(pen_s)), (name, "fused penalizer loss", cpu(pen_f), cpu(pen_s))
        g1, g2 = cpu(g1), cpu(g2)
        assert bool(torch.isfinite(g1).all()), (name, cot)
        assert torch.equal(g1, g2), (name, cot, "fused backward != stand-alone + add", float((g1 - g2).abs().max()))


# ------------------------------------------------------------------------------------------
# penalizer
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,C,batch", RR.pen_case_ids())
def test_penalizer_vs_float64(A, S, C, batch):
    ref = RR.pen_reference(S, C, batch, O)
    raw = ref["raw"].cuda().requires_grad_(True)
    loss = A.P.emptiness_penalizer(raw, ref["z"].cuda(), ref["depth"].cuda()[:, None], ref["d"].cuda(), RR.TOL, RR.DETA_W)
    assert loss.shape == (1,)
    grad, = torch.autograd.grad(loss.sum(), raw)
    RR.compare(cpu(loss).reshape(1, 1), ref["want_loss"].reshape(1, 1), ref["o32_loss"].reshape(1, 1), f"{ref['name']} loss", stats("penalizer loss"))
    RR.compare(cpu(grad), ref["want_grad"], ref["o32_grad"], f"{ref['name']} d_raw", stats("penalizer backward"))
    assert float(cpu(grad)[..., :4].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------
# sampling
# ------------------------------------------------------------------------------------------
def _sample_both(A, bins, w, cdf, u, what):
    """sample_pdf and sample_from_cdf on one draw: stage (ii) for both, and the same floats from both."""
    n = u.shape[-1]
    s, cdf2, inds = A.H.sample_pdf(bins.cuda(), w.cuda(), n, u=u.cuda(), return_aux=True)
    assert torch.equal(cpu(cdf2), cdf), (what, "cdf_out changed with u")
    worst = RR.check_samples(cpu(s), cpu(inds), bins, cdf, u, what + " sample_pdf")
    s2, inds2 = A.H.sample_from_cdf(bins.cuda(), cdf.cuda(), u.cuda())
    assert torch.equal(cpu(inds2), cpu(inds)) and torch.equal(cpu(s2), cpu(s)), (what, "sample_from_cdf != sample_pdf on the same cdf")
    return worst


@pytest.mark.parametrize("nb,batch", RR.sample_case_ids())
def test_sampling_vs_float64(A, nb, batch):
    case = RR.sample_case(nb, batch)
    bins, w, name = case["bins"], case["w"], case["name"]
    N = bins.shape[0]
    # stage (i): the CDF the kernel returns
    _, cdf, _ = A.H.sample_pdf(bins.cuda(), w.cuda(), 1, u=torch.zeros(N, 1).cuda(), return_aux=True)
    cdf = cpu(cdf)
    err = RR.check_cdf(cdf, w, name)
    st = stats("sampling")
    st["cdf"] = max(st.get("cdf", 0.0), err)
    # stage (ii), given that CDF: 0, 1, every knot, both neighbours of every knot, random draws -- every one of them, per-row u
    cand = RR.u_candidates(cdf, nb)
    worst = 0.0
    for i, u in enumerate(RR.u_chunks(cand, 128)):
        worst = max(worst, _sample_both(A, bins, w, cdf, u, f"{name} n=128 chunk {i}"))
    for n in (1, 63, 65):
        chunks = RR.u_chunks(cand, n)
        for i in sorted({0, 2 % len(chunks), len(chunks) // 2, len(chunks) - 1}):      # 0 and 1; knots; knots' neighbours; random
            worst = max(worst, _sample_both(A, bins, w, cdf, chunks[i], f"{name} n={n} chunk {i}"))
    # one draw shared by all rows (u_row_stride 0): row 0's knots and neighbours
    for n in RR.SAMPLE_N:
        chunks = RR.u_chunks(cand[:1], n)
        for i in sorted({0, len(chunks) // 2}):
            worst = max(worst, _sample_both(A, bins, w, cdf, chunks[i][0].contiguous(), f"{name} shared n={n} chunk {i}"))
    st["ulps"] = max(st.get("ulps", 0.0), worst)
    print(f"{name}: samples within {worst:.2f} ulp of max|bins| of the float64 evaluation")


@pytest.mark.parametrize("S,n_imp", RR.RESAMPLE_SHAPES)
def test_importance_resample_ties(A, S, n_imp):
    case = RR.resample_case(S, n_imp)
    z, w, name = case["z"], case["w"], case["name"]
    N = z.shape[0]
    mid = (.5 * (z[:, 1:] + z[:, :-1])).contiguous()
    _, cdf, _ = A.H.sample_pdf(mid.cuda(), w[:, 1:-1].contiguous().cuda(), 1, u=torch.zeros(N, 1).cuda(), return_aux=True)
    cdf = cpu(cdf)
    RR.check_cdf(cdf, w[:, 1:-1], name)
    u = RR.resample_u(case, cdf)
    for uu in (u, u[0].contiguous()):
        zf, zs = A.H.importance_resample(z.cuda(), w.cuda(), n_imp, u=uu.cuda(), return_samples=True)
        zf, zs = cpu(zf), cpu(zs)
        assert zf.shape == (N, S + n_imp)
        assert bool(torch.isfinite(zf).all()), (name, "a slot of z_fine was left unwritten or is not finite")
        assert torch.equal(zf, torch.sort(torch.cat([z, zs], -1), -1).values), name
        s, _, _ = A.H.sample_pdf(mid.cuda(), w[:, 1:-1].contiguous().cuda(), n_imp, u=uu.cuda(), return_aux=True)
        assert torch.equal(zs, cpu(s)), (name, "importance_resample's samples != sample_pdf's")
        RR.check_samples(zs, None, mid, cdf, uu, name)
    hits = (zs[0][:, None] == z[0][None, :]).any(-1)                         # (row 0 of the shared draw is row 0's own draw)
    assert int(hits.sum()) >= 1, (name, "no sample landed on a coarse depth: the case lost its ties")


@pytest.mark.parametrize("K", RR.SORT_K)
def test_sort_rows_ties(A, K):
    for N in ((7, 5) if K == 65 else (7,)):
        x = RR.sort_case(K, N)
        got = cpu(A.MA.sort_rows(x.cuda()))
        want = torch.sort(x, -1).values
        assert got.shape == want.shape and not bool(torch.isnan(got).any()), (K, N)
        assert torch.equal(got, want), (K, N, (got != want).nonzero()[:8].tolist())
