"""``dmnerf_render_rays_fwd`` and ``dmnerf_render_rays_fwd_fine`` (csrc/api.hip) against their own stages, called one by one through
the public stage entries -- ``dmnerf_stratify``, the network, ``dmnerf_composite_fwd`` / ``dmnerf_weights_from_sigma``,
``dmnerf_importance_resample`` -- on the same inputs and draws.  A chain only enqueues those launches in order, so every output is
``torch.equal``: there is no tolerance.  (The third chain, ``.._fwd_fine_skip``, has this comparison in test_gpu_skip.py and
test_gpu_f16_skip.py: ``restate_render``.)

The shapes are the smallest the entries accept, S = 3 and n_imp = 2, on 33 rays: one full group of 32 sample lanes and a tail."""
import types

import pytest
import torch

from _gpu import A, frame_rays, models  # noqa: F401

pytestmark = pytest.mark.gpu

N, S, N_IMP = 33, 3, 2


_cache = {}


def case(A, ins_num, perturb):
    """-> (coarse model, fine model, rays_o, rays_d, z, args, draws); the models and rays are made once per ins_num."""
    if ins_num not in _cache:
        _cache[ins_num] = (*models(ins_num), *frame_rays(N, start=90000), A.H.z_val_sample(N, 4.0, 15.0, S, device="cuda"))
    g = torch.Generator().manual_seed(5)
    t_rand, u = torch.rand(N, S, generator=g).cuda(), torch.rand(N, N_IMP, generator=g).cuda()
    args = types.SimpleNamespace(perturb=1.0 if perturb else False, N_importance=N_IMP, is_train=False, N_ins=None)
    return (*_cache[ins_num], args, dict(t_rand=t_rand, u=u) if perturb else dict(u=u))


def fine_stages(A, mf, ro, rd, z_f):
    raw = A.R.run_network(mf, ro, rd, z_f)
    rgb, _, depth, ins = A.R.render_train(raw, z_f, rd)
    return {"rgb_fine": rgb, "ins_fine": ins, "depth_fine": depth, "z_vals_fine": z_f, "raw_fine": raw}


def same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert bool(torch.isfinite(got["raw_fine"]).all()) and float(got["rgb_fine"].std()) > 0


# (ins_num 1, 13: one block of 32 logits; 59: two)
@pytest.mark.parametrize("perturb", [False, True], ids=["z_copy", "t_rand"])
@pytest.mark.parametrize("ins_num", [1, 13, 59])
def test_render_rays_fwd_equals_its_stages(A, ins_num, perturb):
    mc, mf, ro, rd, z, args, draws = case(A, ins_num, perturb)
    with torch.no_grad():
        z_c = A.H.stratify(z, draws["t_rand"]) if perturb else z
        raw_c = A.R.run_network(mc, ro, rd, z_c)
        rgb_c, w_c, depth_c, ins_c = A.R.render_train(raw_c, z_c, rd)
        want = fine_stages(A, mf, ro, rd, A.H.importance_resample(z_c, w_c, N_IMP, u=draws["u"]))
        want.update(raw_coarse=raw_c, rgb_coarse=rgb_c, depth_coarse=depth_c, ins_coarse=ins_c, z_vals_coarse=z_c)
        got = A.R.dm_nerf(torch.stack([ro, rd]), None, None, mc, mf, z, args, **draws)
    assert got["raw_fine"].shape == (N, S + N_IMP, 4 + ins_num + 1)
    same(got, want)


@pytest.mark.parametrize("ins_num,perturb,events", [(i, p, False) for i in (1, 13, 59) for p in (False, True)] + [(13, False, True), (13, True, True)])
def test_render_rays_fwd_fine_equals_its_stages(A, ins_num, perturb, events):
    mc, mf, ro, rd, z, args, draws = case(A, ins_num, perturb)
    L, lib = A.L, A.lib
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if events else None
    with torch.no_grad():
        z_c = A.H.stratify(z, draws["t_rand"]) if perturb else z
        sigma, w = torch.empty(N, S, device="cuda"), torch.empty(N, S, device="cuda")
        L.check(lib.dmnerf_mlp_fwd_rays_density(L.ptr(mc.blob()), ins_num, L.ptr(ro), L.ptr(rd), L.ptr(z_c), N, S, L.ptr(sigma), L.stream()), "density")
        L.check(lib.dmnerf_weights_from_sigma(L.ptr(sigma), L.ptr(z_c), L.ptr(rd), N, S, L.ptr(w), L.stream()), "weights")
        want = fine_stages(A, mf, ro, rd, A.H.importance_resample(z_c, w, N_IMP, u=draws["u"]))
        got = A.R.dm_nerf_fine(torch.stack([ro, rd]), None, None, mc, mf, z, args, _events=ev, **draws)
    same(got, want)
    if events:
        torch.cuda.synchronize()
        assert ev[0].elapsed_time(ev[1]) > 0                         # the pair brackets the fine network's launch
