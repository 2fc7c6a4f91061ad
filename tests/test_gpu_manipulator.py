"""GPU tests (-m gpu) of the manipulation render against vectors produced by the reference's own
networks/manipulator.py: the integer / copy stages exactly, the float stages to the composite tolerance, and the
whole ``manipulator`` loosely (it chains three ill-conditioned resamplings and discrete label decisions)."""
import types

import numpy as np
import pytest
import torch

from _gpu import A, cpu, model_from  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu


def test_exchanger_golden_exact(A, golden):
    g = golden("manipulator")
    labels = [int(v) for v in g["ex_labels"]]
    for T in (1, 2):
        ori = g["ex_ori_raw"].clone().cuda()
        tars = [g["ex_tar_raw0"].cuda(), g["ex_tar_raw1"].cuda()][:T]
        accs = [g["ex_tar_acc0"].cuda(), g["ex_tar_acc1"].cuda()][:T]
        out_raw, _, ori_label, tar_label = A.MA.exchanger(ori, tars, g["ex_ori_acc"].cuda(), accs, labels[:T])
        assert out_raw.data_ptr() == ori.data_ptr()                              # in place, like the reference
        want = O.exchanger(g["ex_ori_raw"].clone(), [g["ex_tar_raw0"].clone(), g["ex_tar_raw1"].clone()][:T], g["ex_ori_acc"],
                           [g["ex_tar_acc0"], g["ex_tar_acc1"]][:T], labels[:T])
        assert torch.equal(cpu(ori_label), want[2]) and torch.equal(cpu(tar_label), want[3])
        assert torch.equal(cpu(out_raw), want[0])
        if T == 2:                                                               # the committed reference outputs
            assert torch.equal(cpu(out_raw), g["ex_out_raw"])
            assert torch.equal(cpu(ori_label), g["ex_out_ori_label"]) and torch.equal(cpu(tar_label), g["ex_out_tar_label"])
    # every branch of the operation mask occurs in the fixture
    changed = (g["ex_out_raw"] != g["ex_ori_raw"]).any(-1)
    zeroed = (g["ex_out_raw"] == 0).all(-1)
    assert bool(changed.any()) and bool(zeroed.any()) and bool((~changed).any())


def test_manipulator_render_z_and_sort(A, golden):
    g = golden("manipulator")
    rgb, w, dep, ins = [cpu(t) for t in A.MA.manipulator_render(g["mr_raw"].cuda(), g["mr_z"].cuda(), g["mr_d"].cuda())]
    assert ins.shape == g["mr_ins"].shape                                        # all C channels kept
    for got, name in ((rgb, "rgb"), (w, "w"), (dep, "depth"), (ins, "ins")):
        want = g[f"mr_{name}"]
        assert torch.allclose(got, want, rtol=2e-6, atol=2e-6 * max(1.0, float(want.abs().max()))), name
    assert torch.equal(cpu(A.MA.manipulator_z(2, 0.0, 4.7, 64)), g["mz"])
    x = torch.randn(7, 320, generator=torch.Generator().manual_seed(3))
    x[0, 5] = x[0, 17]                                                            # duplicates
    assert torch.equal(cpu(A.MA.sort_rows(x.cuda())), torch.sort(x, -1)[0])


def _mk(A, seed, ins_num, **kw):
    return model_from(O.make_weights(int(seed), ins_num, **kw), ins_num)


def test_manipulator_stage_by_stage_on_reference_intermediates(A, golden, capsys):
    """``manipulator`` (networks/manipulator.py:137-205) chains three inverse-CDF resamplings (each divides by a cdf slope
    as small as 1e-5) and two rounds of discrete label decisions, so float noise anywhere moves a few samples and the
    swaps that depend on them: end to end only a loose bound is meaningful.  Like ``_check_levels`` for ``dm_nerf``, every
    stage is therefore pinned TIGHTLY on the inputs the reference itself fed to it -- the recorded intermediates of one
    run of the reference (T = 2 moved objects, 24 rays, 'trained-like' weights so that the swaps really happen: the second
    exchanger call rewrites 5181 of 10752 samples and zeroes 808):
      exchanger #1 -> render of the edited coarse field -> 4th resampling -> merged depths (64 + 128 + 2 x 128) ->
      fine network on the merged depths -> exchanger #2 -> final render."""
    from dm_nerf_amd.networks import helpers as H, render as R
    g = golden("manipulator_stages")
    labels = [int(v) for v in g["labels"]]
    ins_num = int(g["ins_num"])
    d = g["ori_rays"][1].cuda()
    accs = [g["ex1_tar_acc0"].cuda(), g["ex1_tar_acc1"].cuda()]
    # exchanger #1 (manipulator.py:177): integer / copy logic, exact
    ori = g["ex1_ori_raw_in"].clone().cuda()
    out_raw, _, _, _ = A.MA.exchanger(ori, [g["ex1_tar_raw0"].cuda(), g["ex1_tar_raw1"].cuda()], g["ex1_ori_acc"].cuda(), accs, labels)
    assert torch.equal(cpu(out_raw), g["ex1_out_raw"])
    # step 2 (:179-203).  weights of the edited coarse field
    _, w, _, _ = A.MA.manipulator_render(g["ex1_out_raw"].cuda(), g["s2_z"].cuda(), d)
    w = cpu(w)
    assert torch.allclose(w, g["s2_w"], rtol=2e-6, atol=2e-6)
    # the 4th resampling (manipulator.py:186-187), on the reference's weights and draw.
    # (i) identical (cdf, u) -> identical bin indices, exactly, and samples to roundoff (the contract's "inds exact")
    mid = .5 * (g["s2_z"][..., 1:] + g["s2_z"][..., :-1])
    _, cdf_o, _ = O.sample_pdf(mid, g["pdf3_w"], 128, u=g["pdf3_u"], return_aux=True)
    s_o, inds_o = O.sample_from_cdf(mid, cdf_o, g["pdf3_u"])
    s_d, inds_d = H.sample_from_cdf(mid.cuda(), cdf_o.cuda(), g["pdf3_u"].cuda())
    assert torch.equal(cpu(inds_d), inds_o)
    assert torch.allclose(cpu(s_d), s_o, rtol=1e-6, atol=1e-6)
    # (ii) from the weights: with 'trained-like' weights most bins are EMPTY, i.e. carry exactly the 1e-5 the reference adds
    # (helpers.py:125), their pdf is 1e-5 / (1 + 62e-5) = 0.9994e-5 -- 6e-9 below the `denom < 1e-5 -> 1` threshold of
    # helpers.py:150-151, closer than one f32 ulp of the cdf (6e-8): which side a bin falls on is decided by the rounding
    # of the cdf sums, in the reference as much as here.  Such threshold-critical draws (they sample empty space; the
    # render does not see them) are set aside, every other draw must agree.
    # Everywhere else the sample is bins_lo + (u - cdf_lo) / denom * width: a cdf that differs in its last bits (4 ulp =
    # 2.4e-7; the sum of the 62 weights is formed in a different order) moves it by 2.4e-7 / denom * width -- the
    # conditioning of the reference's own formula, which is what the tolerance follows (denom is as small as 1e-5).
    below, above = (inds_o - 1).clamp(min=0), inds_o.clamp(max=cdf_o.shape[-1] - 1)
    denom = torch.gather(cdf_o, 1, above) - torch.gather(cdf_o, 1, below)
    critical = (denom - 1e-5).abs() <= 2.4e-7                                      # within 4 ulp of the cdf
    width = torch.gather(mid, 1, above) - torch.gather(mid, 1, below)
    tol = 1e-5 * (1 + g["pdf3_out"].abs()) + 4.8e-7 / torch.where(denom < 1e-5, torch.ones_like(denom), denom) * width
    _, zs = H.importance_resample(g["s2_z"].cuda(), g["s2_w"].cuda(), 128, u=g["pdf3_u"].cuda(), return_samples=True)
    zs = cpu(zs)
    same = (zs - g["pdf3_out"]).abs() <= tol
    tight = (zs - g["pdf3_out"]).abs() <= 1e-5 * (1 + g["pdf3_out"].abs())
    frac_crit, agree = float(critical.float().mean()), float(same[~critical].float().mean())
    assert agree >= 0.999 and float(tight.float().mean()) >= 0.99, (agree, frac_crit, float(tight.float().mean()))
    # merged depths: a pure permutation, exact
    merged = A.MA.sort_rows(torch.cat([g["s2_z"], g["pdf3_out"], g["pdf1_out"], g["pdf2_out"]], -1).cuda())
    assert torch.equal(cpu(merged), g["s2_ori_z_merged"])
    tz0 = A.MA.sort_rows(torch.cat([O.manipulator_z(24, 4.0, 15.0, 64), g["pdf3_out"], g["pdf1_out"], g["pdf2_out"]], -1).cuda())
    assert torch.equal(cpu(tz0), g["s2_tar_z0"]) and torch.equal(g["s2_tar_z0"], g["s2_tar_z1"])
    # fine network on the merged depths (448 samples per ray), original and both target ray sets
    mf = _mk(A, g["seeds"][1], ins_num, **O.PEAKY)
    worst, f32gap = {}, {}
    for rays_key, z_key, raw_key in (("ori_rays", "s2_ori_z_merged", "s2_ori_raw"), ("tar_rays0", "s2_tar_z0", "s2_tar_raw0"),
                                     ("tar_rays1", "s2_tar_z1", "s2_tar_raw1")):
        rays = g[rays_key].cuda()
        with torch.no_grad():
            raw, _ = A.MA.manipulator_nerf(rays, None, None, mf, z_vals=g[z_key].cuda())
        raw, want = cpu(raw), g[raw_key]
        assert raw.shape == want.shape == (24, 448, 4 + ins_num + 1)
        err = (raw - want).abs() / (1 + want.abs())
        worst[raw_key] = [float(err[..., :3].max()), float(err[..., 3].max()), float(err[..., 4:].max())]
        # PEAKY scales the density head by 100 and the trunk by 2 (the contract's 1e-5 (1 + |raw|) is stated for default-init-class
        # weights).  The f32-roundoff class of THESE weights is MEASURED, not assumed: the reference's own f32 result (the golden
        # `want`) against a float64 evaluation of the same network on the same inputs -- the kernel may be as far from the reference
        # as the reference is from the real number (x 2: two independent f32 roundings), and never beyond the old fixed bounds
        sd64 = {k: v.double() for k, v in O.make_weights(int(g["seeds"][1]), ins_num, **O.PEAKY).items()}
        ref64, _ = O.manipulator_nerf(g[rays_key].double(), sd64, z_vals=g[z_key].double())
        gap = (want.double() - ref64).abs() / (1 + ref64.abs())
        own = [float(gap[..., :3].max()), float(gap[..., 3].max()), float(gap[..., 4:].max())]
        f32gap.setdefault(raw_key, own)
        for got_e, ref_e, cap in zip(worst[raw_key], own, (1e-4, 1e-3, 1e-4)):
            assert got_e <= min(cap, max(2.0 * ref_e, 1e-5)), (raw_key, worst[raw_key], own)
    # exchanger #2 (:201) on the reference's own fine raws: exact, labels included
    ori = g["s2_ori_raw"].clone().cuda()
    out_raw, _, ol, tl = A.MA.exchanger(ori, [g["s2_tar_raw0"].cuda(), g["s2_tar_raw1"].cuda()], g["ex1_ori_acc"].cuda(), accs, labels)
    assert torch.equal(cpu(out_raw), g["ex2_out_raw"])
    assert torch.equal(cpu(ol), g["ex2_out_ori_label"]) and torch.equal(cpu(tl), g["ex2_out_tar_label"])
    # final render (:203): object map keeps all C channels
    rgb, _, _, ins = A.MA.manipulator_render(g["ex2_out_raw"].cuda(), g["s2_ori_z_merged"].cuda(), d)
    assert torch.allclose(cpu(rgb), g["final_rgb"], rtol=2e-6, atol=2e-6) and torch.allclose(cpu(ins), g["final_ins"], rtol=2e-6, atol=2e-6)
    assert torch.equal(cpu(ins).argmax(-1), g["final_ins"].argmax(-1))
    with capsys.disabled():
        print(f"\n[manipulator stages] resampling: {frac_crit:.4f} of the draws threshold-critical, within the conditioning bound on the others "
              f"{agree:.5f}, within 1e-5 overall {float(tight.float().mean()):.5f}; fine network max |d raw|/(1+|raw|) [rgb, sigma, ins]: " + str(worst)
              + "; the reference's own f32 result against float64 on the same inputs: " + str(f32gap))


def test_manipulator_whole_chain_smoke(A, golden):
    """The whole chain, loosely (see the stage test above for why): finite, right shapes, the plain coarse render tight,
    most rays close; plus rays are independent -- a 96-ray call equals its two halves bit for bit."""
    g = golden("manipulator")
    ins_num = int(g["m_ins_num"])
    mc, mf = _mk(A, g["m_seed_c"], ins_num, gain=1.7, sigma_bias=0.3), _mk(A, g["m_seed_f"], ins_num, gain=1.7, sigma_bias=0.3)
    tars = [g["m_tar_rays0"].cuda(), g["m_tar_rays1"].cuda()]
    labels = [int(v) for v in g["ex_labels"]]
    for T in (1, 2):
        a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, target_labels=labels[:T])
        us = [g[f"m{T}_u{i}"].cuda() for i in range(2 + T)]
        with torch.no_grad():
            out = A.MA.manipulator(None, None, mc, mf, g["m_ori_rays"].cuda(), tars[:T], a, us=us)
        for got, n in zip(out, ("final_rgb", "final_ins", "tar_rgb", "tar_ins_accum")):
            got, want = cpu(got), g[f"m{T}_{n}"]
            assert got.shape == want.shape and bool(torch.isfinite(got).all()), (T, n)
            err = (got - want).abs().amax(-1)
            if n == "tar_rgb":
                assert float(err.max()) <= 2e-5, (T, n, float(err.max()))
            else:
                assert float((err <= 5e-3).float().mean()) >= 0.75, (T, n, err.tolist())
        assert out[1].shape[-1] == ins_num + 1                    # the object map has all C channels (manipulator.py:101-102)
    # config-5-sized call: 3072 rays (N_train of the ScanNet config), T = 1; halves reproduce the whole
    K = O.dmsr_intrinsics(480, 640)
    ro, rd = O.get_rays_k(480, 640, K, O.pose_spherical(110.0, -65.0, 7.0))
    sel = torch.from_numpy(np.random.RandomState(29).choice(480 * 640, 3072, replace=False))
    ori = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]], 0).cuda()
    tar = ori.clone(); tar[0] += torch.tensor([0.3, -0.2, 0.1], device="cuda")
    mc, mf = _mk(A, 713, ins_num, **O.PEAKY), _mk(A, 714, ins_num, **O.PEAKY)
    a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, target_labels=[2])
    us = [torch.rand(3072, 128, generator=torch.Generator().manual_seed(30 + i)).cuda() for i in range(3)]
    with torch.no_grad():
        whole = A.MA.manipulator(None, None, mc, mf, ori, [tar], a, us=us)
        half = A.MA.manipulator(None, None, mc, mf, ori[:, 1536:].contiguous(), [tar[:, 1536:].contiguous()], a, us=[x[1536:].contiguous() for x in us])
    for w_, h_ in zip(whole, half):
        assert bool(torch.isfinite(w_).all()) and torch.equal(w_[1536:], h_)
    assert len(torch.unique(whole[1].argmax(-1))) >= 3


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_manipulator_opt_in_split_modes(A, golden, mode):
    """``args.mfma_split`` reaches the manipulator's 3 + 4 T network launches (extension; the chain itself is the default one).  The
    chain thresholds on accumulated object codes and resamples on thresholded weights, so, as in the smoke test above, it is held
    loosely against the reference's recorded outputs -- the plain coarse target render tight -- and against the default mode on a
    config-5-sized call; rays stay independent (halves reproduce the whole bit for bit)."""
    g = golden("manipulator")
    ins_num = int(g["m_ins_num"])
    mc, mf = _mk(A, g["m_seed_c"], ins_num, gain=1.7, sigma_bias=0.3), _mk(A, g["m_seed_f"], ins_num, gain=1.7, sigma_bias=0.3)
    labels = [int(v) for v in g["ex_labels"]]
    a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, target_labels=labels[:1], mfma_split=mode)
    us = [g[f"m1_u{i}"].cuda() for i in range(3)]
    with torch.no_grad():
        out = A.MA.manipulator(None, None, mc, mf, g["m_ori_rays"].cuda(), [g["m_tar_rays0"].cuda()], a, us=us)
    for got, n in zip(out, ("final_rgb", "final_ins", "tar_rgb", "tar_ins_accum")):
        got, want = cpu(got), g[f"m1_{n}"]
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), n
        err = (got - want).abs().amax(-1)
        if n == "tar_rgb":
            assert float(err.max()) <= 2e-5, (n, float(err.max()))
        else:
            assert float((err <= 5e-3).float().mean()) >= 0.75, (n, err.tolist())
    K = O.dmsr_intrinsics(480, 640)
    ro, rd = O.get_rays_k(480, 640, K, O.pose_spherical(110.0, -65.0, 7.0))
    sel = torch.from_numpy(np.random.RandomState(29).choice(480 * 640, 2048, replace=False))
    ori = torch.stack([ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]], 0).cuda()
    tar = ori.clone(); tar[0] += torch.tensor([0.3, -0.2, 0.1], device="cuda")
    mc, mf = _mk(A, 713, ins_num, gain=1.7, sigma_bias=0.3), _mk(A, 714, ins_num, gain=1.7, sigma_bias=0.3)
    us = [torch.rand(2048, 128, generator=torch.Generator().manual_seed(30 + i)).cuda() for i in range(3)]
    a0 = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, target_labels=[2])
    a1 = types.SimpleNamespace(**vars(a0), mfma_split=mode)
    with torch.no_grad():
        base = A.MA.manipulator(None, None, mc, mf, ori, [tar], a0, us=us)
        whole = A.MA.manipulator(None, None, mc, mf, ori, [tar], a1, us=us)
        half = A.MA.manipulator(None, None, mc, mf, ori[:, 1024:].contiguous(), [tar[:, 1024:].contiguous()], a1, us=[x[1024:].contiguous() for x in us])
    for w_, h_, b_, n in zip(whole, half, base, ("final_rgb", "final_ins", "tar_rgb", "tar_ins_accum")):
        assert bool(torch.isfinite(w_).all()) and torch.equal(w_[1024:], h_), n
        err = (w_ - b_).abs().amax(-1)
        assert float((err <= 5e-3).float().mean()) >= 0.9, (mode, n, float((err <= 5e-3).float().mean()))
    assert float((whole[2] - base[2]).abs().max()) <= 2e-5          # the plain coarse render of the target view
