"""CPU tests of tests/_fwd_save_restate.py, the float64 restatement tests/test_gpu_fwd_save.py holds the training forwards' saved
activations to: the restated network is the oracle's (and a two-sample case done by hand), ``layer_from_saved`` chained over its own
outputs is ``forward_tensors``, the restated encoding is the oracle's in Embedder.embed's column order, the rays of every case give the
chosen points exactly, the kernels' encoding ALGORITHM is measured against the referee on every argument the GPU test uses (ALG_ABS,
which the GPU module carries as a constant), and the integer and one-hot operands keep what their exactness rests on.

    pytest -s tests/test_fwd_save_restate.py -k "algorithm or integer"        prints ALG_ABS and the integer set's largest sum of |terms|
"""
import numpy as np
import pytest
import torch

import _dgrad_restate as DR
import _fwd_save_restate as FR
from _gpu import ulp32
from oracle import ref_cpu as O


def split(x):
    return x[:, :FR.POS_CH].T.contiguous(), x[:, FR.POS_CH:].T.contiguous()


@pytest.mark.parametrize("ins_num,M", [(13, 40), (93, 33), (1, 7)])
def test_float32_restatement_is_the_oracle_to_a_few_ulp(ins_num, M):
    """Both are float32 evaluations of the same formulas (the oracle row-major through F.linear, the restatement feature-major): they
    may differ by summation order only, which after eleven layers is a few ulp of the largest output -- 8 is allowed, and each is
    seen to be several ulp from float64, so the comparison could tell them apart."""
    sd = O.make_weights(21, ins_num, gain=1.7)
    x = torch.randn(M, 90, generator=torch.Generator().manual_seed(22))
    want = O.mlp_forward(sd, x)
    pe, de = split(x)
    got = FR.forward_tensors(sd, pe, de, torch.float32)["raw"].T
    f64 = FR.forward_tensors(sd, pe, de, torch.float64)["raw"].T
    u = ulp32(float(want.abs().max()))
    print(f"restatement - oracle: {float((got - want).abs().max()) / u:.2f} ulp; float32 - float64: {float((got.double() - f64).abs().max()) / u:.2f} ulp")
    assert float((got - want).abs().max()) <= 8 * u
    assert float((got.double() - f64).abs().max()) <= 64 * u
    acts = O.mlp_forward({k: v.double() for k, v in sd.items()}, x.double(), return_acts=True)[1]
    h64 = FR.forward_tensors(sd, pe, de, torch.float64)["h"]
    for l in range(8):
        assert float((acts[l][:, :256].T - h64[l]).abs().max()) <= 1e-12 * float(h64[l].abs().max()), l


def test_float64_restatement_on_a_case_done_by_hand():
    """Two samples, weights with one or two entries per row: every value below is written out from networks/dm_nerf.py:80-106."""
    ins_num = 1
    p = {}
    for name, (n_out, n_in) in FR.param_shapes(ins_num).items():
        p[name + ".weight"], p[name + ".bias"] = torch.zeros(n_out, n_in), torch.zeros(n_out)
    pe, de = torch.zeros(63, 2), torch.zeros(27, 2)
    pe[0], pe[62], de[26] = torch.tensor([1.0, -2.0]), torch.tensor([0.5, 4.0]), torch.tensor([3.0, 1.0])
    p["mlps.0.weight"][0, 0], p["mlps.0.weight"][1, 0], p["mlps.0.bias"][1] = 2.0, -1.0, 0.25      # h_0[0] = relu(2 x), h_0[1] = relu(-x + 1/4)
    for l in range(1, 8):
        p[f"mlps.{l}.weight"][0, 0], p[f"mlps.{l}.weight"][1, 1] = 1.0, 1.0                         # carried on
    p["mlps.5.weight"][2, 256 + 62], p["mlps.5.bias"][2] = 3.0, -1.0                               # the skip: h_5[2] = relu(3 pe_62 - 1)
    p["mlps.7.weight"][2, 2] = 0.0                                                                 # (h_6[2] is not carried into h_7)
    p["mlps.6.weight"][2, 2] = 1.0
    p["density_linear.weight"][0, 0], p["density_linear.weight"][0, 1], p["density_linear.bias"][0] = 1.0, 10.0, -0.5
    p["rgb_feature_linear.weight"][5, 0], p["rgb_feature_linear.bias"][5] = 1.0, 1.0               # rgb_feature[5] = h_7[0] + 1
    p["rgb_feature_linears.0.weight"][7, 5], p["rgb_feature_linears.0.weight"][7, 256 + 26] = 1.0, -1.0      # g1[7] = relu(that - de_26)
    p["rgb_linear.weight"][2, 7], p["rgb_linear.bias"][2] = 2.0, 0.125
    p["ins_feature_linear.weight"][9, 1] = 4.0                                                     # ins_feature[9] = 4 h_7[1]
    p["ins_feature_linears.0.weight"][3, 9], p["ins_feature_linears.0.bias"][3] = 1.0, -1.0       # g2[3] = relu(that - 1)
    p["ins_linear.weight"][1, 3], p["ins_linear.bias"][0] = -1.0, 7.0
    t = FR.forward_tensors(p, pe, de, torch.float64)
    h0 = {0: [2.0, 0.0], 1: [0.0, 2.25]}
    for l in range(8):
        want = torch.zeros(256, 2, dtype=torch.float64)
        want[0], want[1] = torch.tensor(h0[0]), torch.tensor(h0[1])
        if l in (5, 6):
            want[2] = torch.tensor([0.5, 11.0])
        assert torch.equal(t["h"][l], want), l
    g1 = torch.zeros(128, 2, dtype=torch.float64)
    g1[7] = torch.tensor([0.0, 0.0])                               # relu(2 + 1 - 3), relu(0 + 1 - 1)
    assert torch.equal(t["g1"], g1)
    g2 = torch.zeros(128, 2, dtype=torch.float64)
    g2[3] = torch.tensor([0.0, 8.0])                               # relu(0 - 1), relu(9 - 1)
    assert torch.equal(t["g2"], g2)
    raw = torch.tensor([[0.0, 0.0], [0.0, 0.0], [0.125, 0.125], [1.5, 22.0], [7.0, 7.0], [0.0, -8.0]], dtype=torch.float64)
    assert torch.equal(t["raw"], raw)
    p["rgb_feature_linears.0.bias"][7] = 0.5                       # ... and with g1[7] open: rgb[2] = 2 x 1/2 + 1/8
    assert torch.equal(FR.forward_tensors(p, pe, de, torch.float64)["raw"][2], torch.tensor([1.125, 1.125], dtype=torch.float64))
    ab = FR.forward_tensors(p, pe, de, torch.float64, absolute=True)
    assert ab["g1"][7].tolist() == [6.5, 2.5] and ab["raw"][5].tolist() == [0.0, 8.0] and ab["h"][0][1].tolist() == [1.25, 2.25]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layers_chained_over_their_own_outputs_are_the_forward(dtype):
    ins_num, M = 13, 37
    sd = O.make_weights(23, ins_num, gain=1.7)
    pe, de = split(torch.randn(M, 90, generator=torch.Generator().manual_seed(24)))
    for absolute in (False, True):
        full = FR.forward_tensors(sd, pe, de, dtype)
        inp = {"pe": pe, "de": de, "h": [None] * 8}
        for l in range(8):
            inp["h"][l] = FR.layer_from_saved(sd, f"h_{l}", inp, dtype)
            assert torch.equal(inp["h"][l], full["h"][l]), l
        for k in ("g1", "g2"):
            inp[k] = FR.layer_from_saved(sd, k, inp, dtype)
            assert torch.equal(inp[k], full[k]), k
        for k in ("rgb", "sigma", "logits"):
            assert torch.equal(FR.layer_from_saved(sd, k, inp, dtype), full["raw"][FR.raw_rows(k, ins_num + 1)]), k
        if absolute:                                               # the sums of |terms|: never below |value|, and on the last GEMM never above the path's
            last = FR.forward_tensors(sd, pe, de, dtype, absolute=True)
            for name in FR.TENSORS:
                path = FR.layer_from_saved(sd, name, inp, dtype, absolute=True)
                val = FR.layer_from_saved(sd, name, inp, dtype)
                assert bool((path >= val.abs()).all()), name
                l = last["h"][int(name[2:])] if name.startswith("h_") else (last[name] if name in last else last["raw"][FR.raw_rows(name, ins_num + 1)])
                assert bool((l <= path * (1 + 1e-6)).all()), name
    assert [FR.roundings(n) for n in ("h_0", "h_1", "h_5", "g1", "g2", "sigma", "rgb", "logits")] == [66, 259, 322, 286 + 259, 259 + 259, 259, 131, 131]
    assert FR.roundings("h_3") == DR.STAGE_ROUNDINGS


def test_encoding_is_the_oracles_in_embed_order():
    g = torch.Generator().manual_seed(5)
    v = torch.rand(3, 50, generator=g) * 2 - 1                     # small arguments: |2^k v| <= 512
    for L in (FR.POS_L, FR.DIR_L):
        want = O.embed(v.T.contiguous(), L).T                      # [3 + 6 L, M]
        got = FR.encode_rows(v, L, torch.float32)
        assert got.shape == (3 + 6 * L, 50) and torch.equal(got[:3], want[:3])
        assert bool(((got - want).abs().double() <= FR.ulp32_of(want.double())).all())      # the same torch calls on another memory order
        ref = FR.encode_rows(v, L, torch.float64)
        assert ref.dtype == torch.float64 and torch.equal(ref[:3], v.double())
        assert bool(((got.double() - ref).abs() <= FR.ulp32_of(ref)).all())      # float32 sin / cos of the same argument: within 1 ulp
        alg = FR.encode_algorithm(v, L)
        # csrc/layout.h::pefeat spelled out: k-pair 2 + 3 k + c holds (sin, cos)(2^k v_c) = columns 3 + 6 k + c and 3 + 6 k + 3 + c
        for k in range(L):
            for c in range(3):
                a = v[c].double() * 2.0 ** k
                for t in (ref, alg):
                    assert float((t[3 + 6 * k + c] - torch.sin(a)).abs().max()) < 1e-9 and float((t[3 + 6 * k + 3 + c] - torch.cos(a)).abs().max()) < 1e-9
    assert FR.ulp32_of(torch.tensor([0.0, 1.0, -1.5, 2.0 ** -127, 0.75], dtype=torch.float64)).tolist() == [2.0 ** -149, 2.0 ** -23, 2.0 ** -23, 2.0 ** -149, 2.0 ** -24]


def test_rays_give_the_chosen_points_exactly():
    specials = set(FR.SPECIALS.view(np.uint32).tolist())
    assert len(specials) == 26
    seen, kinds = set(), set()
    for case in FR.CASES:
        r = FR.case_rays(case)
        assert r["N"] * r["S"] == case.M and r["rays_o"].shape == (r["N"], 3) and r["z"].shape == (r["N"], r["S"])
        pts = FR.ray_points(r)
        assert pts.shape == (3, case.M) and float(pts.abs().max()) <= 16.0
        have = set(pts.numpy().view(np.uint32).reshape(-1).tolist())
        if case.M >= 128:
            assert specials <= have, FR.case_id(case)
        seen |= have & specials
        kinds |= set(r["kinds"])
        d = FR.ray_dirs(r, torch.float64)
        assert float(((d * d).sum(0) - 1).abs().max()) < 1e-12
    assert seen == specials and kinds == set(FR.KINDS)
    # the denormal products and a 1e-20 direction component are there
    pts, dirs = FR.all_arguments()
    assert int(((pts.abs() > 0) & (pts.abs() < 2.0 ** -126)).sum()) > 100 and bool((dirs.abs() == np.float32(1e-20)).any())
    assert bool((pts.view(torch.int32) == torch.tensor(-0.0).view(torch.int32)).any())            # -0 itself


def test_encoding_algorithm_against_the_referee():
    """ALG_ABS: the largest absolute error of the kernels' algorithm (before its final rounding to float32) against the referee, over
    every point and direction of every case.  It is an order of magnitude above what the header of csrc/mlp_common.h::encode expects of
    the recurrence: c' = 1 - 2 s^2, s' = 2 s c multiply the distance of (s, c) from the unit circle by 4 s^2 per octave, and the
    polynomial's truncation (6e-12 at the fold, |x| = pi / 2) is such a distance."""
    pts, dirs = FR.all_arguments()
    worst = 0.0
    for name, v, L in (("points", pts, FR.POS_L), ("directions", dirs, FR.DIR_L)):
        ref, alg = FR.encode_rows(v, L, torch.float64), FR.encode_algorithm(v, L)
        assert torch.equal(alg[:3], ref[:3])
        err = (alg - ref).abs()
        per_k = [float(err[3 + 6 * k:9 + 6 * k].max()) for k in range(L)]
        print(f"encode_algorithm - referee, {name} ({v.shape[1]} triples): per octave " + " ".join(f"{e:.2e}" for e in per_k))
        worst = max(worst, float(err.max()))
    print(f"ALG_ABS = {worst:.3e}")
    import test_gpu_fwd_save as G
    assert worst <= G.ALG_ABS <= 1.05 * worst, (worst, G.ALG_ABS)   # the GPU module's constant is this figure
    assert 4 * G.ALG_ABS < 2.4e-7 / 10                             # far inside the encoding's contract


@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_integer_set_is_exact_in_float32(case):
    """Whole numbers everywhere and every sum of |terms| -- of every element of every tensor, the two unsaved feature linears included
    -- below 2^24: every float32 partial sum, in any order, is exact.  And the operands are not vacuous."""
    params, x = FR.integer_set(case.ins_num), FR.integer_rows(case)
    for k, w in params.items():
        assert set(w.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}, k
        if k.endswith(".weight"):
            assert int((w != 0).sum(0).max()) <= FR.INT_TERMS, k
    assert set(x.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    pe, de = split(x)
    want = FR.forward_tensors(params, pe, de, torch.float64)
    ab = FR.forward_tensors(params, pe, de, torch.float64, absolute=True)
    top = max(float(t.max()) for t in ab.values())
    print(f"{FR.case_id(case)}: largest sum of |terms| {top:.0f} = 2^{np.log2(top):.2f}")
    assert top < 2.0 ** 24
    for k, t in want.items():
        assert bool((t == torch.round(t)).all()) and bool((t.abs() <= ab[k]).all()), k
    assert torch.equal(FR.forward_tensors(params, pe, de, torch.float32)["raw"].double(), want["raw"])
    if case.M >= 31:
        for name, t in [(f"h_{l}", want["h"][l]) for l in range(8)] + [("g1", want["g1"]), ("g2", want["g2"])]:
            assert 0.2 < float((t > 0).float().mean()) < 0.8, name
        assert float((want["raw"] != 0).float().mean()) > 0.5


@pytest.mark.parametrize("ins_num", [13, 93])
def test_onehot_operands_name_every_feature(ins_num):
    params = FR.onehot_params(ins_num)
    for k, w in params.items():
        if k.endswith(".weight"):
            assert set(w.unique().tolist()) <= {0.0, 1.0} and int(w.sum(1).min()) >= 1 and int(w.sum(1).max()) <= 2, k
        else:
            assert float(w.min()) > 0 and len(set(w.tolist())) == w.numel() and bool((w % 8 == 0).all()), k
    assert float(params["rgb_feature_linears.0.weight"][:, 256:].abs().max()) == 0
    x, r = FR.onehot_rows(), FR.onehot_rays()
    inputs = {"embedded": split(x), "rays": (FR.encode_rows(FR.ray_points(r), FR.POS_L, torch.float64), FR.encode_rows(FR.ray_dirs(r, torch.float32), FR.DIR_L, torch.float64))}
    assert bool((inputs["rays"][0] == torch.round(inputs["rays"][0])).all())
    for pe, de in inputs.values():
        want = FR.forward_tensors(params, pe, de, torch.float64)
        ab = FR.forward_tensors(params, pe, de, torch.float64, absolute=True)
        assert max(float(t.max()) for t in ab.values()) < 2.0 ** 24
        for t in list(want["h"]) + [want["g1"], want["g2"], want["raw"]]:
            s = torch.sort(t, 0)[0]
            assert bool((s[1:] != s[:-1]).all()) and bool((t == torch.round(t)).all()) and float(t.min()) > 0
    assert len({tuple(row) for row in x.tolist()}) > 150            # the embedded rows differ from sample to sample
