"""Float64 restatement of the data-gradient pass (csrc/mlp_bwd.hip, mlp_bwd_split.hip, mlp_bwd_f16.hip).  CPU only; shared by
tests/test_dgrad_restate.py (CPU) and tests/test_gpu_dgrad.py (GPU).  Nothing here reads what a kernel wrote.

Given the ReLU masks the data gradient is a LINEAR function of dL/draw, and the masks are an input -- 2304 bit words per 32-sample
block of the forward's workspace -- so this module writes all three operands itself and no forward takes part:
  save   the forward's workspace (csrc/layout.h::SaveLayout), of which the kernels read the bit region only: per block
         [8 layers][64 lanes][4 words] | g1 [64][2] at word 2048 | g2 [64][2] at word 2176.  Element p = 32 w + i of a lane is bit
         31 - i of its word w (csrc/mlp_common.h::pack_mask / apply_mask), p = 16 b + r, and register (b, r) of lane l holds
         feature 32 b + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of sample l & 31 of the block.  Everything else in the buffer is NaN.  The
         bits of the padding columns M .. Mp - 1 are an argument of the encoder and ONES by default (a kernel that let padding
         through would show);
  graw   dL/draw, [M][4 + C] as the kernels read it; in this module in feature order [4 + C, M] (rows 0 .. 2 rgb, 3 sigma, 4 .. logits);
  the parameters, as the state dict of the reference network (the kernels read packed transposes of them, and the product
  F = A[:, :256] . W_rgb_feature in place of the two matrices -- packing and fold are under test with the kernel).
Logical form of the masks: bool tensors in feature order, {"h": [8, 256, M], "g1": [128, M], "g2": [128, M]}.

Reference (``reference``): from networks/dm_nerf.py and the header of csrc/mlp_bwd.hip, on the UNFOLDED matrices, in any dtype
(float64 = the reference, float32 = the yardstick of the real-operand comparison) and with ``absolute=True`` on |operands| (= the sum
of |terms| along each element's path).  What it returns is what the kernels write: dy_0 .. dy_7, dg1, dg2 (tests/_wgrad_restate.py
documents their place in the gradient workspace) and the block-major copy of dL/draw.

Integer operands: dL/draw in {-1, 0, 1}; every weight matrix a sum of TERMS = 4 signed, scaled, thinned permutation-like matrices
(at most TERMS nonzeros per column, and per row where it is square; entries in {-1, -1/2, 0, 1/2, 1}), so every output names its few
inputs.  ``integer_bound`` states what exactness rests on: every sum of |terms|, at every one of the ten GEMM stages and in F, is
below 2^15 (no f16 plane leaves its range) AND, divided by the stage's grain (every value of a stage is a whole multiple of
2^-(number of matrices with halves behind it)), below 2^22 -- the 22 bits that two f16 planes rounded towards zero hold, which
is fewer than float32's 24 and the 24 of three bf16 planes.  Every weight is a single f16 / bf16 plane, so no product of two low
planes is dropped.  Measured here (tests/test_dgrad_restate.py asserts it per case): sum of |terms| <= 193, bits <= 17.5.
"""
import collections

import numpy as np
import torch

from _wgrad_restate import (DIR_CH, HW, POS_CH, R_BITS, R_G1, R_H, SAVE_ROWS, W, _get, _mem_feature, _put, decode, flat_gradient,  # noqa: F401
                            param_shapes, row_len)

BITS_WORDS = 8 * 64 * 4 + 2 * 64 * 2                              # 2304 per 32-sample block
WORD_G1, WORD_G2 = 2048, 2176
TERMS = 4
STAGE_ROUNDINGS = 259                                             # per GEMM stage behind an element: 256 products' sums, and change
FOLD_ROUNDINGS = 256                                              # F = A[:, :256] . W_rgb_feature is formed in float32


# ------------------------------------------------------------------------------------------
# masks: bool tensors <-> bit words
# ------------------------------------------------------------------------------------------
def reg_feature(rows):
    """[2, rows / 2]: the feature that register p = 16 b + r of a lane of half-wave ``half`` holds."""
    p = np.arange(rows // 2)
    b, r = p >> 4, p & 15
    return np.stack([32 * b + (r & 3) + 8 * (r >> 2) + 4 * half for half in (0, 1)])


def where(feature, sample):
    """(block, lane, register p, word, bit) of an element of an accumulator-layout tensor: for failure messages."""
    half, b, r = (feature >> 2) & 1, feature >> 5, (feature & 3) | (((feature >> 3) & 3) << 2)
    p = 16 * b + r
    return sample >> 5, (sample & 31) + 32 * half, p, p >> 5, 31 - (p & 31)


def _pack(t):
    """bool [rows, Mp] -> int32 words [Mp / 32][64 lanes][rows / 64]."""
    rows, Mp = t.shape
    P = rows // 2
    x = t.numpy()[reg_feature(rows)]                               # [half, p, Mp]
    x = x.reshape(2, P, Mp // 32, 32).transpose(2, 0, 3, 1)        # [block, half, sample in block, p]: lane = 32 half + sample
    x = x.reshape(Mp // 32, 64, P // 32, 32).astype(np.uint64)
    words = (x << (31 - np.arange(32, dtype=np.uint64))).sum(-1)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32))


def _unpack(words, rows):
    """The inverse of ``_pack``: int32 [blocks][64][rows / 64] -> bool [rows, 32 blocks]."""
    nb, P = words.shape[0], rows // 2
    u = words.numpy().view(np.uint32).astype(np.uint64)
    x = ((u[..., None] >> (31 - np.arange(32, dtype=np.uint64))) & 1).astype(bool)         # [block, lane, word, i]
    x = x.reshape(nb, 2, 32, P).transpose(1, 3, 0, 2).reshape(2, P, nb * 32)                # [half, p, Mp]
    out = np.zeros((rows, nb * 32), dtype=bool)
    out[reg_feature(rows)] = x
    return torch.from_numpy(out)


def _padded(t, Mp, pad):
    rows, M = t.shape
    full = torch.ones(rows, Mp, dtype=torch.bool)
    full[:, :M] = t
    if Mp > M and pad is not None:
        full[:, M:] = pad
    return full


def mask_words(masks, M, pad=None):
    """Logical masks -> int32 [Mp / 32][2304], the bit region of the workspace.  pad: the bits of the columns M .. Mp - 1, a dict of
    bool tensors with the masks' keys ([8, 256, Mp - M], [128, Mp - M]); None = all ones."""
    Mp = row_len(M)
    pad = pad or {}
    ph = pad.get("h")
    parts = [_pack(_padded(masks["h"][l], Mp, None if ph is None else ph[l])).reshape(Mp // 32, 256) for l in range(8)]
    parts += [_pack(_padded(masks[k], Mp, pad.get(k))).reshape(Mp // 32, 128) for k in ("g1", "g2")]
    words = torch.cat(parts, 1)
    assert words.shape == (Mp // 32, BITS_WORDS)
    return words


def words_masks(words, M):
    """The inverse of ``mask_words``: (masks, pad)."""
    nb = words.shape[0]
    h = torch.stack([_unpack(words[:, l * 256:(l + 1) * 256].reshape(nb, 64, 4), W) for l in range(8)])
    g1 = _unpack(words[:, WORD_G1:WORD_G1 + 128].reshape(nb, 64, 2), HW)
    g2 = _unpack(words[:, WORD_G2:WORD_G2 + 128].reshape(nb, 64, 2), HW)
    full = {"h": h, "g1": g1, "g2": g2}
    return {k: v[..., :M].clone() for k, v in full.items()}, {k: v[..., M:].clone() for k, v in full.items()}


def encode_save(masks, M, pad=None):
    """The forward workspace as the data-gradient kernels read it: NaN but for the bit region."""
    Mp = row_len(M)
    save = torch.full((SAVE_ROWS * Mp,), float("nan"), dtype=torch.float32)
    save.view(torch.int32)[R_BITS * Mp:] = mask_words(masks, M, pad).reshape(-1)
    return save


def save_words(save, M):
    """The bit region of a workspace (a CPU float32 tensor) as int32 [Mp / 32][2304]."""
    Mp = row_len(M)
    return save.view(torch.int32)[R_BITS * Mp:SAVE_ROWS * Mp].reshape(Mp // 32, BITS_WORDS).clone()


def encode_graw_t(graw, M):
    """Feature-order [4 + C, M] -> the block-major copy [Mp / 32][4 + C][32] the kernels write next to the gradients (flat)."""
    Mp = row_len(M)
    buf = torch.empty(graw.shape[0] * Mp, dtype=graw.dtype)
    _put(buf, 0, graw, Mp, False, None)
    return buf


def decode_outputs(dsave, graw_t, M, C):
    """What a kernel wrote -> ({"dy", "dg1", "dg2", "graw"} in feature order, the same keys' padding columns, the part of the
    workspace the kernels must leave alone: the regions of pe, de and the bit masks, as one flat tensor)."""
    Mp = row_len(M)
    out, pad = {}, {}
    parts = [_get(dsave, R_H + l * W, W, M, Mp, True) for l in range(8)]
    out["dy"], pad["dy"] = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    dg, dgp = _get(dsave, R_G1, 2 * HW, M, Mp, True)               # ONE 256-row tensor per block: dg1 | dg2
    out["dg1"], out["dg2"], pad["dg1"], pad["dg2"] = dg[:HW].clone(), dg[HW:].clone(), dgp[:HW].clone(), dgp[HW:].clone()
    out["graw"], pad["graw"] = _get(graw_t, 0, 4 + C, M, Mp, False)
    return out, pad, torch.cat([dsave[:R_H * Mp], dsave[R_BITS * Mp:]])


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def reference(masks, graw, params, ins_num, dtype=torch.float64, absolute=False):
    """{"dy": [8, 256, M], "dg1", "dg2": [128, M], "graw_t": the block-major copy of dL/draw (flat), "pre": the unmasked result of
    every stage, "F": the folded matrix} from the masks, dL/draw [4 + C, M] and the state dict (networks/dm_nerf.py:80-106)."""
    cv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    M = graw.shape[1]
    assert graw.shape[0] == 4 + ins_num + 1
    g = cv(graw)
    g_rgb, g_sigma, g_ins = g[0:3], g[3:4], g[4:]
    m_h, m_g1, m_g2 = (masks[k].to(dtype) for k in ("h", "g1", "g2"))
    Wt = lambda name: cv(params[name + ".weight"])
    pre = {}
    # ins branch (:95-97, :103): its input is h.detach() -- dg2 is a result, nothing of it reaches h_7
    pre["ins_linear^T"] = Wt("ins_linear").T @ g_ins
    dg2 = m_g2 * pre["ins_linear^T"]
    # rgb branch (:89-92, :102): rgb = rgb_linear(relu(rgb_feature_linears.0(cat[rgb_feature_linear(h_7), dirs])))
    pre["rgb_linear^T"] = Wt("rgb_linear").T @ g_rgb
    dg1 = m_g1 * pre["rgb_linear^T"]
    A = Wt("rgb_feature_linears.0")[:, :W]                         # (the direction columns lead to the encoding: no gradient)
    pre["A^T"] = A.T @ dg1
    dh = Wt("rgb_feature_linear").T @ pre["A^T"] + Wt("density_linear").T @ g_sigma         # + density_linear (:101)
    dy, dhs = [None] * 8, [None] * 8
    for l in range(7, -1, -1):
        dhs[l] = dh
        dy[l] = m_h[l] * dh
        if l > 0:
            dh = Wt(f"mlps.{l}")[:, :W].T @ dy[l]                  # mlps.5 reads cat[h_4, pts] (:87): its h columns only
    pre["dh"] = torch.stack(dhs)
    return {"dy": torch.stack(dy), "dg1": dg1, "dg2": dg2, "graw_t": encode_graw_t(g, M), "pre": pre,
            "F": A @ Wt("rgb_feature_linear")}


def roundings(key, layer=None):
    """The number of float32 roundings on the path of an element of dg1 / dg2 / dy_layer in the f32 kernel."""
    if key in ("dg1", "dg2"):
        return STAGE_ROUNDINGS
    return (2 + (7 - layer)) * STAGE_ROUNDINGS + FOLD_ROUNDINGS


def integer_bound(ref_abs):
    """(largest sum of |terms| over every stage and F, largest number of bits a value of any stage needs) from
    ``reference(..., absolute=True)`` of integer operands -- see the module docstring."""
    pre = ref_abs["pre"]
    # halvings behind a stage: one per matrix with halves on the path (F counts two)
    stages = [("ins_linear^T", pre["ins_linear^T"], 1), ("rgb_linear^T", pre["rgb_linear^T"], 1), ("A^T", pre["A^T"], 2), ("F", ref_abs["F"], 2)]
    stages += [(f"dh_{l}", pre["dh"][l], 3 + (7 - l)) for l in range(8)]
    top = max(float(t.max()) for _, t, _ in stages)
    bits = max(np.log2(max(float(t.max()), 1.0)) + k for _, t, k in stages)
    return top, bits


# ------------------------------------------------------------------------------------------
# operand generators
# ------------------------------------------------------------------------------------------
def sparse_matrix(n_out, n_in, g, terms=TERMS, positive=False):
    """A sum of ``terms`` signed, scaled permutation-like matrices whose nonzeros never coincide: column c has its entries in rows
    (pi(c) + t step) mod n_out, pi a random permutation of the columns taken mod n_out; each is 0 (one in four), +-1/2 or +-1.
    positive: every entry is +1/2 or +1 (a path through such matrices never cancels)."""
    k = min(terms, n_out)
    step = n_out // 2 + 1 if n_out > 2 else 1
    assert len({(t * step) % n_out for t in range(k)}) == k
    w = torch.zeros(n_out, n_in)
    pi = torch.randperm(n_in, generator=g) % n_out
    cols = torch.arange(n_in)
    for t in range(k):
        mag = torch.randint(1, 3, (n_in,), generator=g).float() * 0.5
        sign = torch.randint(0, 2, (n_in,), generator=g).float() * 2 - 1
        keep = (torch.randint(0, 4, (n_in,), generator=g) > 0).float()
        w[(pi + t * step) % n_out, cols] = mag if positive else mag * sign * keep
    return w


def integer_params(ins_num, seed, terms=TERMS, positive=False):
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, (n_out, n_in) in param_shapes(ins_num).items():
        params[name + ".weight"] = sparse_matrix(n_out, n_in, g, terms, positive)
        params[name + ".bias"] = torch.randint(-2, 3, (n_out,), generator=g).float() * 0.5          # (no bias reaches a data gradient)
    return params


def bernoulli_masks(M, g, p=0.5):
    return {"h": torch.rand(8, W, M, generator=g) < p, "g1": torch.rand(HW, M, generator=g) < p, "g2": torch.rand(HW, M, generator=g) < p}


def integer_operands(ins_num, M, seed):
    """(masks, dL/draw [4 + C, M]): Bernoulli(1/2) masks, dL/draw uniform in {-1, 0, 1}."""
    g = torch.Generator().manual_seed(seed)
    return bernoulli_masks(M, g), torch.randint(-1, 2, (4 + ins_num + 1, M), generator=g).float()


def real_operands(ins_num, M, seed):
    """(masks, dL/draw [4 + C, M]): dL/draw N(0, 1) with a third of the entries exactly 0 and channel c scaled by 2^(c mod 5 - 2);
    Bernoulli(1/2) masks but one trunk layer all ones (3 + seed mod 5), one all zeros (seed mod 3: nothing is left below it),
    exactly one bit of g1 per sample, g2 all ones."""
    g = torch.Generator().manual_seed(seed)
    masks = bernoulli_masks(M, g)
    masks["h"][3 + seed % 5] = True
    masks["h"][seed % 3] = False
    masks["g1"] = torch.zeros(HW, M, dtype=torch.bool)
    masks["g1"][torch.randint(0, HW, (M,), generator=g), torch.arange(M)] = True
    masks["g2"] = torch.ones(HW, M, dtype=torch.bool)
    s = (4 + ins_num + 1, M)
    graw = torch.randn(s, generator=g) * (torch.rand(s, generator=g) >= 1.0 / 3.0).float()
    graw = graw * torch.exp2(torch.remainder(torch.arange(s[0], dtype=torch.float32), 5) - 2)[:, None]
    return masks, graw


def real_params(ins_num, seed):
    from oracle import ref_cpu as O
    return {k: v.clone() for k, v in O.make_weights(seed, ins_num, gain=1.7).items()}


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
INS_WHY = collections.OrderedDict([
    (1, "C = 2: two logits in one block"), (13, "C = 14, the shipped configuration"), (31, "C = 32: one full logit block"),
    (32, "C = 33: one channel in a second block"), (93, "C = 94: three blocks"), (127, "C = 128: four full blocks, the maximum")])
M_WHY = collections.OrderedDict([
    (1, "one sample in a block of padding"), (31, "one padding column"), (32, "a full block, no padding"), (33, "a full block and one sample"),
    (128, "four blocks: exactly one workgroup"), (129, "second workgroup: one live wave, three that duplicate it"),
    (161, "second workgroup: two live waves, ragged tail"), (225, "second workgroup: four live waves, ragged tail")])
Case = collections.namedtuple("Case", "ins_num M")
CASES = [Case(i, m) for i in INS_WHY for m in M_WHY]              # the full cross: 48 cases of at most 225 samples


def case_id(c):
    return f"ins{c.ins_num}_M{c.M}"


def case_seed(case, kind):
    return 11 + 1009 * CASES.index(case) + (500 if kind == "real" else 0)


_PARAMS, _REF = {}, {}


def case_params(ins_num, kind):
    """The parameters of a case depend on ins_num and the kind only (one model per ins_num on the device).  Read-only."""
    key = (ins_num, kind)
    if key not in _PARAMS:
        _PARAMS[key] = integer_params(ins_num, 70 + ins_num) if kind == "integer" else real_params(ins_num, 170 + ins_num)
    return _PARAMS[key]


def references(masks, graw, params, ins_num, kind):
    ref = {"want": reference(masks, graw, params, ins_num), "abs": reference(masks, graw, params, ins_num, absolute=True)}
    if kind == "real":
        ref["f32"] = reference(masks, graw, params, ins_num, dtype=torch.float32)
    return ref


def case_data(case, kind):
    """(masks, dL/draw [4 + C, M], params, {"want": float64 reference, "abs": on |operands|, "f32": the yardstick (real only)}),
    computed once per (case, kind) and shared: treat all of it as read-only."""
    key = (CASES.index(case), kind)
    if key not in _REF:
        seed = case_seed(case, kind)
        masks, graw = integer_operands(case.ins_num, case.M, seed) if kind == "integer" else real_operands(case.ins_num, case.M, seed)
        params = case_params(case.ins_num, kind)
        _REF[key] = (masks, graw, params, references(masks, graw, params, case.ins_num, kind))
    return _REF[key]


def sweep_params():
    """ins_num 13, for the one-bit sweep: two terms per column, every entry +1/2 or +1, so that no path cancels and an open mask
    bit always shows (with dL/draw all ones)."""
    if "sweep" not in _PARAMS:
        _PARAMS["sweep"] = integer_params(13, 83, terms=2, positive=True)
    return _PARAMS["sweep"]


def scale_case_data():
    """(masks, dL/draw, params, references) of the f16x2 gradient-scale test: ins_num 13, M = 161, two terms per column -- every sum
    of |terms| stays below 2^5, so that 2^10 times it stays inside the f16 planes' range."""
    if "scale" not in _REF:
        masks, graw = integer_operands(13, 161, 97)
        params = integer_params(13, 98, terms=2)
        _REF["scale"] = (masks, graw, params, references(masks, graw, params, 13, "integer"))
    return _REF["scale"]
