"""CPU tests of tests/_dgrad_restate.py, the float64 restatement tests/test_gpu_dgrad.py holds the data-gradient kernels to: the
mask encoding round-trips and is the addressing of csrc/layout.h spelled out, the block-major dL/draw round-trips through the
weight-gradient restatement's decoder, the integer operands keep what their exactness rests on in every case, and the restated
formulas -- fed, with the oracle's activations, to the weight-gradient restatement -- give the oracle MLP's autograd gradients
(which ties BOTH restatements to the reference network, h.detach() and the layer-5 skip included)."""
import pytest
import torch

import _dgrad_restate as DR
import _wgrad_restate as WR
from oracle import ref_cpu as O


@pytest.mark.parametrize("M", [1, 32, 33, 161])
def test_mask_words_round_trip(M):
    g = torch.Generator().manual_seed(M)
    masks = DR.bernoulli_masks(M, g)
    Mp = WR.row_len(M)
    words = DR.mask_words(masks, M)
    assert words.shape == (Mp // 32, DR.BITS_WORDS) and words.dtype == torch.int32
    back, pad = DR.words_masks(words, M)
    for k in masks:
        assert torch.equal(back[k], masks[k]), k
        assert bool(pad[k].all()), k                               # padding bits: ones unless given
    pad = {k: torch.rand(*v.shape[:-1], Mp - M, generator=g) < 0.5 for k, v in masks.items()}
    back, pad2 = DR.words_masks(DR.mask_words(masks, M, pad), M)
    assert all(torch.equal(back[k], masks[k]) and torch.equal(pad2[k], pad[k]) for k in masks)
    save = DR.encode_save(masks, M)
    assert save.numel() == WR.SAVE_ROWS * Mp and bool(torch.isnan(save[:WR.R_BITS * Mp]).all())
    assert torch.equal(DR.save_words(save, M), words)


def test_mask_addressing_spelled_out():
    """One bit at a time, from the text of csrc/layout.h and csrc/mlp_common.h::apply_mask, not from the encoder's own tables."""
    M = 70
    for key, layer, f, m in (("h", 0, 0, 0), ("h", 3, 4, 33), ("h", 7, 255, 69), ("h", 2, 9, 31), ("h", 5, 100, 64), ("g1", None, 0, 5),
                             ("g1", None, 127, 69), ("g2", None, 36, 32), ("g2", None, 3, 0)):
        masks = {"h": torch.zeros(8, 256, M, dtype=torch.bool), "g1": torch.zeros(128, M, dtype=torch.bool), "g2": torch.zeros(128, M, dtype=torch.bool)}
        if key == "h":
            masks["h"][layer, f, m] = True
        else:
            masks[key][f, m] = True
        zeros = {k: torch.zeros(*v.shape[:-1], WR.row_len(M) - M, dtype=torch.bool) for k, v in masks.items()}
        words = DR.mask_words(masks, M, zeros)
        # the lane's register p = 16 b + r holds feature 32 b + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of sample lane & 31
        hit = [(lane, b, r) for lane in range(64) for b in range(8) for r in range(16)
               if 32 * b + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) == f and (lane & 31) == m % 32]
        assert len(hit) == 1
        lane, b, r = hit[0]
        p = 16 * b + r
        per_lane = 4 if key == "h" else 2
        base = layer * 256 if key == "h" else (2048 if key == "g1" else 2176)
        at = (m // 32, base + lane * per_lane + (p >> 5))
        want = torch.zeros_like(words)
        want[at] = 1 << (31 - (p & 31)) if (p & 31) else -(1 << 31)
        assert torch.equal(words, want), (key, layer, f, m)
        assert DR.where(f, m) == (m // 32, lane, p, p >> 5, 31 - (p & 31))


@pytest.mark.parametrize("ins_num,M", [(1, 1), (13, 33), (127, 161)])
def test_graw_t_round_trips_through_the_wgrad_decoder(ins_num, M):
    masks, graw = DR.real_operands(ins_num, M, 3)
    ref = DR.reference(masks, graw, DR.case_params(ins_num, "integer"), ins_num, dtype=torch.float32)
    Mp = WR.row_len(M)
    junk = torch.zeros(WR.SAVE_ROWS * Mp)
    ops, pad = WR.decode(junk, junk, ref["graw_t"], M)
    assert torch.equal(ops["graw"], graw) and bool((pad["graw"] == 0).all())
    out, pad, _ = DR.decode_outputs(junk, ref["graw_t"], M, ins_num + 1)
    assert torch.equal(out["graw"], graw) and bool((pad["graw"] == 0).all())


def check_integer(ref, headroom=1.0):
    top, bits = DR.integer_bound(ref["abs"])
    assert top * headroom < 2.0 ** 15 and bits < 22, (top, bits)
    for key in ("dy", "dg1", "dg2"):
        want, absum = ref["want"][key], ref["abs"][key]
        assert bool((want.abs() <= absum).all()), key
        assert torch.equal(want.float().double(), want), key
    assert bool((ref["want"]["F"] * 4 == torch.round(ref["want"]["F"] * 4)).all())      # the fold's entries: quarters, a single plane each
    return top, bits


@pytest.mark.parametrize("case", DR.CASES, ids=DR.case_id)
def test_integer_operands_are_exact_in_every_kernel(case):
    """The condition the exactness claim of the GPU test rests on (module docstring of tests/_dgrad_restate.py), asserted from the
    sums of |terms|; and the operands are not vacuous: from 31 samples on a fifth of every tensor is nonzero."""
    masks, graw, params, ref = DR.case_data(case, "integer")
    top, bits = check_integer(ref)
    print(f"{DR.case_id(case)}: largest sum of |terms| {top}, bits {bits:.2f}")
    for k, w in params.items():
        if k.endswith(".weight"):
            assert int((w != 0).sum(0).max()) <= DR.TERMS and set(w.abs().unique().tolist()) <= {0.0, 0.5, 1.0}, k
            if w.shape[0] == w.shape[1]:
                assert int((w != 0).sum(1).max()) <= DR.TERMS, k
    if case.M >= 31:
        want = ref["want"]
        for name, t in [(f"dy_{l}", want["dy"][l]) for l in range(8)] + [("dg1", want["dg1"]), ("dg2", want["dg2"])]:
            assert float((t != 0).float().mean()) > 0.2, name


def test_the_special_integer_operands_keep_the_bound_too():
    """The one-bit sweep's never-cancelling parameters under all-ones masks (its worst case), and the thin parameters of the
    gradient-scale test with 2^10 on top (the f16 planes stay in range)."""
    M = 161
    ones = {"h": torch.ones(8, 256, M, dtype=torch.bool), "g1": torch.ones(128, M, dtype=torch.bool), "g2": torch.ones(128, M, dtype=torch.bool)}
    params = DR.sweep_params()
    check_integer(DR.references(ones, torch.ones(4 + 14, M), params, 13, "integer"))
    want = DR.reference(ones, torch.ones(4 + 14, M), params, 13)
    assert all(bool((want[k] > 0).all()) for k in ("dy", "dg1", "dg2"))          # no path cancels: an open bit always shows
    masks, graw, params, ref = DR.scale_case_data()
    check_integer(ref, headroom=1024.0)


@pytest.mark.parametrize("ins_num,M", [(13, 40), (93, 33), (1, 7)])
def test_restatements_equal_autograd_of_the_oracle(ins_num, M):
    sd = {k: v.double().requires_grad_(True) for k, v in O.make_weights(21, ins_num, gain=1.7).items()}
    g = torch.Generator().manual_seed(22)
    x = torch.randn(M, 90, generator=g, dtype=torch.float64)
    cot = torch.randn(M, 4 + ins_num + 1, generator=g, dtype=torch.float64)
    out, acts = O.mlp_forward(sd, x, return_acts=True)
    (out * cot).sum().backward()
    p = {k: v.detach() for k, v in sd.items()}
    lin = lambda t, name: torch.nn.functional.linear(t, p[name + ".weight"], p[name + ".bias"])
    h = [a.detach()[:, :256] for a in acts]
    g1 = torch.relu(lin(torch.cat([lin(h[7], "rgb_feature_linear"), x[:, 63:]], 1), "rgb_feature_linears.0"))
    g2 = torch.relu(lin(lin(h[7], "ins_feature_linear"), "ins_feature_linears.0"))
    assert torch.equal(torch.cat([lin(g1, "rgb_linear"), lin(h[7], "density_linear"), lin(g2, "ins_linear")], 1), out.detach())
    T = lambda t: t.T.contiguous()
    masks = {"h": torch.stack([T(a) > 0 for a in h]), "g1": T(g1) > 0, "g2": T(g2) > 0}
    masks, _ = DR.words_masks(DR.mask_words(masks, M), M)          # (through the encoded form)
    ref = DR.reference(masks, T(cot), p, ins_num)
    ops = {"pe": T(x[:, :63]), "de": T(x[:, 63:]), "h": torch.stack([T(a) for a in h]), "g1": T(g1), "g2": T(g2),
           "dy": ref["dy"], "dg1": ref["dg1"], "dg2": ref["dg2"], "graw": WR.decode(torch.zeros(WR.SAVE_ROWS * WR.row_len(M), dtype=torch.float64),
                                                                                  torch.zeros(WR.SAVE_ROWS * WR.row_len(M), dtype=torch.float64), ref["graw_t"], M)[0]["graw"]}
    flat = WR.flat_gradient(ops, p, ins_num)
    sl, _ = WR.param_slices(ins_num)
    for k, (o, shape) in sl.items():
        want = sd[k].grad
        got = flat[o:o + want.numel()].view(shape)
        assert float(want.abs().max()) > 0, k
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (k, float((got - want).abs().max()), float(want.abs().max()))
