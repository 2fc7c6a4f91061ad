"""CPU tests of tests/_wgrad_restate.py, the float64 restatement tests/test_gpu_wgrad.py holds the weight-gradient kernels to:
the operand encoding round-trips, the restated formulas give the oracle MLP's autograd gradients (which pins the layer <->
parameter mapping, the ``cat`` column offsets and the re-association of the two feature linears, csrc/heads.hip), every case of
the table still has the plan property it exists for under all three cost tables, and the integer operands keep every sum of
|terms| below 2^23 (so that every float32 summation order and every bf16 / f16 plane split of them is exact)."""
import types

import pytest
import torch

import _wgrad_restate as WR
from oracle import ref_cpu as O


@pytest.mark.parametrize("ins_num", [1, 13, 127])
@pytest.mark.parametrize("M", [1, 33, 257])
def test_encode_decode_round_trip(M, ins_num):
    for kind in ("integer", "real"):
        ops, _ = WR.integer_operands(ins_num, M, 5) if kind == "integer" else WR.real_operands(ins_num, M, 5, O)
        save, dsave, graw = WR.encode(ops, M, junk_seed=3, integer=kind == "integer")
        Mp = WR.row_len(M)
        assert save.numel() == dsave.numel() == WR.SAVE_ROWS * Mp and graw.numel() == (4 + ins_num + 1) * Mp
        back, pad = WR.decode(save, dsave, graw, M)
        assert set(back) == set(ops)
        for k in ops:
            assert torch.equal(back[k], ops[k]), (kind, k)
            if k in WR.SAVE_KEYS:                                   # padding: finite non-zero junk in save, exact zeros in the gradients
                assert bool(torch.isfinite(pad[k]).all()) and bool((pad[k] != 0).all()), (kind, k)
            else:
                assert bool((pad[k] == 0).all()), (kind, k)
        # what the kernels must not read is NaN: the masks in both workspaces, the encodings' regions of dsave
        assert bool(torch.isnan(save[WR.R_BITS * Mp:]).all()) and bool(torch.isnan(dsave[WR.R_BITS * Mp:]).all())
        assert bool(torch.isnan(dsave[:WR.R_H * Mp]).all())
        assert not bool(torch.isnan(save[:WR.R_BITS * Mp]).any()) and not bool(torch.isnan(dsave[WR.R_H * Mp:WR.R_BITS * Mp]).any())
    # the layout itself, spelled out once: sample m of feature f of h_2 sits in block m / 32 at memory row rho with row_feature(rho) = f
    ops, _ = WR.integer_operands(ins_num, M, 5)
    ops["h"] = torch.arange(8 * 256 * M, dtype=torch.float32).reshape(8, 256, M)
    save, _, _ = WR.encode(ops, M)
    Mp = WR.row_len(M)
    for f, rho in ((0, 0), (4, 1), (1, 2), (7, 7), (12, 9), (250, 252)):
        m = M - 1
        at = (WR.R_H + 2 * 256) * Mp + (m // 32) * 256 * 32 + rho * 32 + m % 32
        assert float(save[at]) == float(ops["h"][2, f, m]), (f, rho)


@pytest.mark.parametrize("ins_num", [13, 93])
def test_restatement_equals_autograd_of_the_oracle(ins_num, monkeypatch):
    M = 40
    sd = {k: v.double().requires_grad_(True) for k, v in O.make_weights(11, ins_num, gain=1.7).items()}
    name_of = {id(v): k[:-len(".weight")] for k, v in sd.items() if k.endswith(".weight")}
    rec = {}

    def linear(x, w, b):                                            # every layer's input, and (hook) its pre-activation gradient
        y = torch.nn.functional.linear(x, w, b)
        name = name_of[id(w)]
        rec[name] = {"x": x.detach()}
        y.register_hook(lambda g, name=name: rec[name].__setitem__("dy", g.detach().clone()))
        return y
    monkeypatch.setattr(O, "F", types.SimpleNamespace(linear=linear, relu=torch.nn.functional.relu))
    g = torch.Generator().manual_seed(12)
    x = torch.randn(M, 90, generator=g, dtype=torch.float64)
    cot = torch.randn(M, 4 + ins_num + 1, generator=g, dtype=torch.float64)
    out = O.mlp_forward(sd, x)
    (out * cot).sum().backward()
    T = lambda t: t.T.contiguous()
    ops = {"pe": T(rec["mlps.0"]["x"]), "de": T(rec["rgb_feature_linears.0"]["x"][:, 256:]),
           "h": torch.stack([T(rec[f"mlps.{l + 1}"]["x"][:, :256]) for l in range(7)] + [T(rec["rgb_feature_linear"]["x"])]),
           "g1": T(rec["rgb_linear"]["x"]), "g2": T(rec["ins_linear"]["x"]),
           "dy": torch.stack([T(rec[f"mlps.{l}"]["dy"]) for l in range(8)]),
           "dg1": T(rec["rgb_feature_linears.0"]["dy"]), "dg2": T(rec["ins_feature_linears.0"]["dy"]),
           "graw": T(torch.cat([rec["rgb_linear"]["dy"], rec["density_linear"]["dy"], rec["ins_linear"]["dy"]], 1))}
    # (the pre-activation gradient of a ReLU layer is the hooked gradient of its linear output: the mask is already in it)
    assert torch.equal(ops["graw"], T(cot))
    save, dsave, graw = WR.encode(ops, M)
    assert save.dtype == torch.float64
    back, _ = WR.decode(save, dsave, graw, M)
    flat = WR.flat_gradient(back, {k: v.detach() for k, v in sd.items()}, ins_num)
    sl, total = WR.param_slices(ins_num)
    assert list(sl) == list(sd) and total == sum(v.numel() for v in sd.values())
    for k, (o, shape) in sl.items():
        want = sd[k].grad
        got = flat[o:o + want.numel()].view(shape)
        assert float(want.abs().max()) > 0, k
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (k, float((got - want).abs().max()), float(want.abs().max()))


@pytest.mark.parametrize("case", WR.CASES, ids=WR.case_id)
def test_cases_have_the_plan_property_they_exist_for(case):
    for mode in WR.MODES:
        WR.check_case_properties(case, mode)
        _, outs, _, _ = WR.plan_tables(mode, case.ins_num, case.M, case.max_wgs)
        WR.entry_map(outs, case.ins_num)                            # the outputs and the unfuse stage write every entry exactly once


@pytest.mark.parametrize("case", WR.CASES, ids=WR.case_id)
def test_integer_operands_are_exact_in_float32(case):
    ref = WR.case_reference(case, "integer")
    assert float(ref["abs"].max()) < 2.0 ** 23, float(ref["abs"].max())
    assert bool((ref["want"].abs() <= ref["abs"]).all())
    assert bool((ref["want"] * 2 == torch.round(ref["want"] * 2)).all())          # halves at the finest: 24 bits hold them
    assert torch.equal(ref["want"].float().double(), ref["want"])
    uf = WR.through_unfuse(case.ins_num)
    assert float(ref["want"][uf].abs().max()) > 0 and float(ref["want"][~uf].abs().max()) > 0
