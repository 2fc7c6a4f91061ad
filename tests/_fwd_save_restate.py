"""Float64 restatement of what the five training forwards put into their workspace (csrc/mlp_fwd_impl.h behind dmnerf_mlp_fwd_rays_train,
_train_fused and dmnerf_mlp_fwd_embedded_train, csrc/mlp_split_train.hip, csrc/mlp_f16_train.hip).  CPU only; shared by
tests/test_fwd_save_restate.py (CPU) and tests/test_gpu_fwd_save.py (GPU).  Nothing here reads what a kernel wrote.

The workspace (csrc/layout.h::SaveLayout, decoded with the helpers of tests/_wgrad_restate.py and tests/_dgrad_restate.py): pe [63] |
de [27] in Embedder.embed's column order | h_0 .. h_7 [256 each] | g1 [128] | g2 [128] in the permuted row order | ReLU bit words.
Tensors here are in FEATURE order with samples as columns: pe [63, M], de [27, M], h [8, 256, M], g1, g2 [128, M], raw [4 + C, M]
(rows 0 .. 2 rgb, 3 sigma, 4 .. the C = ins_num + 1 logits).

  forward_tensors   networks/dm_nerf.py:80-106 in any dtype (float64 = the referee, float32 = the yardstick); absolute=True gives the
                    sum of |terms| of every element's LAST GEMM (and of the two unsaved feature linears) on the actual operands.
  layer_from_saved  ONE tensor from given inputs -- the GPU test feeds it the kernel's own saved inputs, so that every comparison is
                    one GEMM deep (two for g1 and g2) and a wrong element cannot hide behind the roundings of the layers before it.
  encode_rows       the positional encoding; referee: sin / cos of the exact product 2^k float32(v), formed in np.longdouble.
  encode_algorithm  the kernels' own algorithm (comments of csrc/mlp_common.h::encode) in numpy float64 BEFORE its final rounding to
                    float32: it exists to measure, on the CPU, the absolute error of that algorithm against the referee.

Rays of a case (``case_rays``): M = N x S samples (``FACTORING``: every entry accepts any N >= 1, S >= 1), built so that the points
pts = o + d z (separate multiply and add, csrc/mlp_fwd_impl.h) come out as chosen values EXACTLY:
  axis rays     d = +-e_a, o_a = -0: pts_a = +-z exactly, the two other coordinates are o's (0 z = +-0);
  diagonal      d = (1, 1, 1), o = -0: pts = (z, z, z);
  tiny          d a permutation of (1e-20, 1, 0): the products 1e-20 x +-1e-18 are float32 denormals;
  seeded        o, d, z random, |pts| <= 13.
The chosen values (``SPECIALS``): 0, -0, +-1e-38; float32(pi / 4), float32(pi / 2), float32(pi) with their neighbours one ulp either
side and all their negatives (the folds at g = +-1 / 4, +-1 / 2 and the rint ties); +-15 and +-16 (about 8000 rad at k = 9); then
seeded values in [-16, 16].  Every case of 128 samples or more holds every special value (tests/test_fwd_save_restate.py asserts it).

Integer operands (``integer_set``, ``integer_rows``): DR.integer_params (DR.sparse_matrix: at most INT_TERMS nonzeros per column) times
two -- every weight and bias a whole number in {-2 .. 2} -- and rows in {-2 .. 2}.  Every value of every stage is then a whole number,
and with every sum of |terms| below 2^24 every float32 partial sum in any order is exact (tests/test_fwd_save_restate.py asserts the
bound on every case).  One-hot operands (``onehot_params``): one 1 per weight row and distinct positive biases (multiples of 8), so that
every feature of every saved tensor of a sample carries a different whole number.
"""
import math

import numpy as np
import torch

import _dgrad_restate as DR
from _wgrad_restate import (DIR_CH, HW, POS_CH, R_BITS, R_DE, R_G1, R_G2, R_H, R_PE, SAVE_ROWS, W, _get, _mem_feature,  # noqa: F401
                            param_shapes, row_len)

POS_L, DIR_L = 10, 4
TENSORS = [f"h_{l}" for l in range(8)] + ["g1", "g2", "rgb", "sigma", "logits"]
ROUNDINGS_EXTRA = DR.STAGE_ROUNDINGS - W                            # 3: "and change" on top of a GEMM's products


# ------------------------------------------------------------------------------------------
# the network
# ------------------------------------------------------------------------------------------
def forward_tensors(params, pe, de, dtype, absolute=False):
    """{"h": [8, 256, M], "g1", "g2": [128, M], "raw": [4 + C, M], "rgb_feature", "ins_feature": [256, M]} from the state dict and the
    encodings pe [63, M], de [27, M] (networks/dm_nerf.py:80-106).  absolute: every tensor is the sum of |terms| of its last GEMM on
    the operands the forward really has there."""
    P = lambda k: params[k].to(dtype)
    pe, de = pe.to(dtype), de.to(dtype)

    plain = lambda name, x: P(name + ".weight") @ x + P(name + ".bias")[:, None]
    lin = lambda name, x: P(name + ".weight").abs() @ x.abs() + P(name + ".bias").abs()[:, None]      # the sum of |terms|

    out_h, out_abs = [], []
    h = pe
    for l in range(8):                                             # :83-87
        if absolute:
            out_abs.append(lin(f"mlps.{l}", h))
        h = torch.relu(plain(f"mlps.{l}", h))
        out_h.append(h)
        if l == 4:
            h = torch.cat([h, pe], 0)                              # the skip: cat[h, pts] in front of mlps.5 (:87)
    h7 = out_h[7]
    rgb_feature = plain("rgb_feature_linear", h7)                  # no activation (:89)
    g1_in = torch.cat([rgb_feature, de], 0)                        # (:90)
    g1 = torch.relu(plain("rgb_feature_linears.0", g1_in))
    ins_feature = plain("ins_feature_linear", h7)                  # its input is h.detach(): the same values (:95-96)
    g2 = torch.relu(plain("ins_feature_linears.0", ins_feature))
    if absolute:
        return {"h": torch.stack(out_abs), "g1": lin("rgb_feature_linears.0", g1_in), "g2": lin("ins_feature_linears.0", ins_feature),
                "raw": torch.cat([lin("rgb_linear", g1), lin("density_linear", h7), lin("ins_linear", g2)], 0),
                "rgb_feature": lin("rgb_feature_linear", h7), "ins_feature": lin("ins_feature_linear", h7)}
    raw = torch.cat([plain("rgb_linear", g1), plain("density_linear", h7), plain("ins_linear", g2)], 0)      # cat[rgb, density, ins] (:105)
    return {"h": torch.stack(out_h), "g1": g1, "g2": g2, "raw": raw, "rgb_feature": rgb_feature, "ins_feature": ins_feature}


def layer_from_saved(params, name, inputs, dtype, absolute=False):
    """One tensor of ``TENSORS`` from GIVEN inputs (a dict with "pe", "de", "h" [8, 256, M], "g1", "g2" -- only what ``name`` needs is
    read): h_l from h_(l - 1), or pe (l = 0), or [h_4, pe] (l = 5); g1 from (h_7, de) through rgb_feature_linear and
    rgb_feature_linears.0; g2 from h_7 through ins_feature_linear and ins_feature_linears.0; sigma from h_7; rgb from g1; logits from
    g2.  absolute: on |operands|, i.e. the sum of |terms| over every sum on the element's path (both GEMMs of g1 and g2)."""
    cv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    act = (lambda t: t) if absolute else torch.relu
    lin = lambda nm, x: cv(params[nm + ".weight"]) @ x + cv(params[nm + ".bias"])[:, None]
    if name.startswith("h_"):
        l = int(name[2:])
        x = cv(inputs["pe"]) if l == 0 else (torch.cat([cv(inputs["h"][4]), cv(inputs["pe"])], 0) if l == 5 else cv(inputs["h"][l - 1]))
        return act(lin(f"mlps.{l}", x))
    if name == "g1":
        return act(lin("rgb_feature_linears.0", torch.cat([lin("rgb_feature_linear", cv(inputs["h"][7])), cv(inputs["de"])], 0)))
    if name == "g2":
        return act(lin("ins_feature_linears.0", lin("ins_feature_linear", cv(inputs["h"][7]))))
    if name == "sigma":
        return lin("density_linear", cv(inputs["h"][7]))
    if name == "rgb":
        return lin("rgb_linear", cv(inputs["g1"]))
    if name == "logits":
        return lin("ins_linear", cv(inputs["g2"]))
    raise KeyError(name)


def raw_rows(name, C):
    """The rows of raw [4 + C, M] that ``name`` (rgb, sigma, logits) is."""
    return {"rgb": slice(0, 3), "sigma": slice(3, 4), "logits": slice(4, 4 + C)}[name]


def roundings(name):
    """n of the f32 kernels' per-element bound n 2^-24 sum|terms|: the products of the element's GEMM + 3 (the rule and reasoning of
    DR.STAGE_ROUNDINGS), the two-GEMM tensors g1 and g2 with the inner GEMM's n on top."""
    x = ROUNDINGS_EXTRA
    if name.startswith("h_"):
        l = int(name[2:])
        return (POS_CH if l == 0 else (W + POS_CH if l == 5 else W)) + x
    return {"g1": (W + DIR_CH + x) + (W + x), "g2": (W + x) + (W + x), "sigma": W + x, "rgb": HW + x, "logits": HW + x}[name]


# ------------------------------------------------------------------------------------------
# the positional encoding
# ------------------------------------------------------------------------------------------
def encode_rows(v, L, dtype):
    """[3 + 6 L, M] in Embedder.embed's column order [x | sin f0 x | cos f0 x | sin f1 x | ...] (blocks of 3) from v [3, M] float32.
    dtype float32: the reference's own arithmetic (torch sin / cos of the float32 product).  Any other dtype: the referee -- sin and cos
    of the exact product 2^k float32(v), formed in np.longdouble, returned as float64."""
    assert v.dtype == torch.float32 and v.shape[0] == 3
    if dtype == torch.float32:
        rows = [v]
        for k in range(L):
            rows += [torch.sin(v * (2.0 ** k)), torch.cos(v * (2.0 ** k))]
        return torch.cat(rows, 0)
    x = v.numpy().astype(np.longdouble)
    rows = [x]
    for k in range(L):
        a = x * np.longdouble(2.0 ** k)                            # exact: a power of two times a float32
        rows += [np.sin(a), np.cos(a)]
    return torch.from_numpy(np.concatenate(rows, 0).astype(np.float64))


def _fma(a, b, c):
    """a b + c rounded once (to within 2^-64 of the product: extended precision, then one rounding to double)."""
    return (a.astype(np.longdouble) * b.astype(np.longdouble) + np.longdouble(c)).astype(np.float64)


def _sin_rev(t, quarter):
    """csrc/mlp_common.h::sin_rev_d at k = 0: sin(2 pi (t + quarter / 4)) for t in revolutions."""
    g = t + 0.25 * quarter
    g = g - np.rint(g)                                             # frac-to-nearest, exact; ties to even like v_rndne_f64
    ag = np.abs(g)
    gf = np.where(ag > 0.25, 0.5 - ag, ag)                         # fold to [-1/4, 1/4]
    x = gf * 6.283185307179586
    x2 = x * x
    p = np.full_like(x, 1.0 / 1307674368000.0)                     # 1 / 15!
    for c in (-1.0 / 6227020800.0, 1.0 / 39916800.0, -1.0 / 362880.0, 1.0 / 5040.0, -1.0 / 120.0, 1.0 / 6.0):
        p = _fma(p, x2, c)
    return np.copysign(x - x * x2 * p, g)


def encode_algorithm(v, L):
    """The kernels' algorithm in numpy float64, before the final rounding to float32: t = v / (2 pi) in double, ONE sin / cos pair per
    coordinate (frac-to-nearest, fold, degree-15 polynomial), the higher octaves by the double-angle recurrence s' = 2 s c,
    c' = fma(-2 s, s, 1).  [3 + 6 L, M] float64 in ``encode_rows``' order (rows 0 .. 2: v itself)."""
    assert v.dtype == torch.float32 and v.shape[0] == 3
    x = v.numpy().astype(np.float64)
    t = x * 0.15915494309189535
    sn, cs = _sin_rev(t, 0), _sin_rev(t, 1)
    rows = [x]
    for k in range(L):
        rows += [sn, cs]
        t2 = sn + sn
        sn, cs = t2 * cs, _fma(-t2, sn, 1.0)
    return torch.from_numpy(np.concatenate(rows, 0))


def ulp32_of(want):
    """Per element: the float32 spacing at |want| (float64 tensor), 2^-149 in the denormal range and at 0."""
    a = want.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def viewdirs(rays_d, dtype):
    """rays_d / ||rays_d|| (networks/render.py:37) -> [N, 3]."""
    d = rays_d.to(dtype)
    return d / torch.sqrt((d * d).sum(-1, keepdim=True))


# ------------------------------------------------------------------------------------------
# the cases and their rays
# ------------------------------------------------------------------------------------------
CASES = DR.CASES
FACTORING = {1: (1, 1), 31: (31, 1), 32: (4, 8), 33: (3, 11), 128: (8, 16), 129: (43, 3), 161: (7, 23), 225: (15, 15)}     # M = N x S
assert all(n * s == m for m, (n, s) in FACTORING.items()) and set(FACTORING) == set(DR.M_WHY)


def case_id(c):
    n, s = FACTORING[c.M]
    return f"ins{c.ins_num}_M{c.M}_{n}x{s}"


def _f32(x):
    return np.float32(x)


def _specials():
    out = [_f32(0.0), _f32(-0.0), _f32(1e-38), _f32(-1e-38)]
    for c in (math.pi / 4, math.pi / 2, math.pi):
        for s in (1.0, -1.0):
            v = _f32(s * c)
            out += [v, np.nextafter(v, _f32(np.inf)), np.nextafter(v, _f32(-np.inf))]
    out += [_f32(15.0), _f32(-15.0), _f32(16.0), _f32(-16.0)]
    return np.array(out, dtype=np.float32)


SPECIALS = _specials()                                              # 26 values
KINDS = ("x", "y", "z", "diag", "tiny", "seeded")
_RAYS = {}


def case_rays(case):
    """{"N", "S", "rays_o" [N, 3], "rays_d" [N, 3], "z" [N, S], "kinds"}: float32 CPU tensors, deterministic, computed once per case and
    shared (read-only).  The chosen values fill the exact slots (z of the axis and diagonal rays, then o of the axis rays) in order:
    the specials, rotated by the case's index below 128 samples, then seeded values in [-16, 16]."""
    idx = CASES.index(case)
    if idx in _RAYS:
        return _RAYS[idx]
    N, S = FACTORING[case.M]
    g = torch.Generator().manual_seed(9000 + idx)
    rot = 0 if case.M >= 128 else (5 * idx) % len(SPECIALS)
    seeded = (torch.rand(4 * case.M + 8, generator=g) * 32 - 16).numpy().astype(np.float32)
    values = iter(np.concatenate([np.roll(SPECIALS, -rot), seeded]))
    o = np.zeros((N, 3), dtype=np.float32)
    d = np.zeros((N, 3), dtype=np.float32)
    z = np.zeros((N, S), dtype=np.float32)
    kinds = [KINDS[(n + idx) % len(KINDS)] for n in range(N)]
    for n, kind in enumerate(kinds):                                # z first: the slots that every sample has
        if kind in ("x", "y", "z", "diag"):
            z[n] = [next(values) for _ in range(S)]
    for n, kind in enumerate(kinds):
        if kind in ("x", "y", "z"):
            a = "xyz".index(kind)
            sign = -1.0 if (n // len(KINDS)) % 2 else 1.0
            d[n, a] = sign
            z[n] *= sign                                            # pts_a = -0 + sign (sign z) = the chosen value
            o[n] = [next(values), next(values), next(values)]
            o[n, a] = -0.0
        elif kind == "diag":
            d[n] = 1.0
            o[n] = -0.0
        elif kind == "tiny":
            a = n % 3
            d[n, a], d[n, (a + 1) % 3], d[n, (a + 2) % 3] = 1e-20, 1.0, 0.0
            o[n, a], o[n, (a + 1) % 3], o[n, (a + 2) % 3] = -0.0, 0.5 * next(values), next(values)
            zz = (torch.rand(S, generator=g) * 12 - 6).numpy().astype(np.float32)
            zz[0::3] = 1e-18
            zz[1::3] = -1e-18
            z[n] = zz
        else:
            o[n] = (torch.rand(3, generator=g) * 8 - 4).numpy()
            d[n] = torch.randn(3, generator=g).clamp(-1.5, 1.5).numpy()
            z[n] = torch.sort(torch.rand(S, generator=g) * 5 + 1)[0].numpy()
    r = {"N": N, "S": S, "rays_o": torch.from_numpy(o), "rays_d": torch.from_numpy(d), "z": torch.from_numpy(z), "kinds": kinds}
    _RAYS[idx] = r
    return r


def ray_points(rays):
    """pts [3, M] = torch float32 rays_o + rays_d * z (networks/render.py:49: a multiply and an add), sample m = n S + s."""
    pts = rays["rays_o"][:, None, :] + rays["rays_d"][:, None, :] * rays["z"][..., None]
    return pts.reshape(-1, 3).T.contiguous()


def ray_dirs(rays, dtype):
    """viewdirs of every sample [3, M] in ``dtype``."""
    return viewdirs(rays["rays_d"], dtype)[:, None, :].expand(rays["N"], rays["S"], 3).reshape(-1, 3).T.contiguous()


def embedded_rows(rays):
    """[M, 90] float32 rows for the embedded entry: the reference's own float32 encoding of the case's points and directions."""
    return torch.cat([encode_rows(ray_points(rays), POS_L, torch.float32), encode_rows(ray_dirs(rays, torch.float32), DIR_L, torch.float32)], 0).T.contiguous()


def all_arguments():
    """Every float32 value the GPU test has a ray entry encode, over all cases: (points [3, n], directions [3, n])."""
    pts = torch.cat([ray_points(case_rays(c)) for c in CASES], 1)
    dirs = torch.cat([ray_dirs(case_rays(c), torch.float32) for c in CASES], 1)
    return pts, dirs


# ------------------------------------------------------------------------------------------
# integer and one-hot operands
# ------------------------------------------------------------------------------------------
INT_TERMS = 4
_PARAMS = {}


def integer_set(ins_num):
    """The integer parameters of ins_num: DR.integer_params times two (whole numbers in {-2 .. 2}).  Read-only."""
    key = ("integer", ins_num)
    if key not in _PARAMS:
        _PARAMS[key] = {k: v * 2 for k, v in DR.integer_params(ins_num, 270 + ins_num, terms=INT_TERMS).items()}
    return _PARAMS[key]


def integer_rows(case):
    """[M, 90] float32 rows in {-2 .. 2} for the embedded entry."""
    g = torch.Generator().manual_seed(31 + 1009 * CASES.index(case))
    return torch.randint(-2, 3, (case.M, POS_CH + DIR_CH), generator=g).float()


ONEHOT_SEED = {13: 4001, 93: 4001}                                 # the first from 4000 on with every value distinct, both entries


def onehot_params(ins_num):
    """One 1 per weight row (mlps.5: one among its h columns and, in 63 of its rows, one among its pe columns; the direction columns
    of rgb_feature_linears.0 stay 0) and distinct positive biases, multiples of 8: with inputs in {0 .. 3} every feature of a saved
    tensor of a sample is a different whole number (tests/test_fwd_save_restate.py asserts it).  The seed is the first for which that
    holds on the one-hot inputs of both entries."""
    key = ("onehot", ins_num)
    if key in _PARAMS:
        return _PARAMS[key]
    g = torch.Generator().manual_seed(ONEHOT_SEED[ins_num])
    params = {}
    for name, (n_out, n_in) in param_shapes(ins_num).items():
        w = torch.zeros(n_out, n_in)
        n_src = W if name in ("mlps.5", "rgb_feature_linears.0") else n_in
        src = torch.cat([torch.randperm(n_src, generator=g) for _ in range((n_out + n_src - 1) // n_src)])[:n_out]
        w[torch.arange(n_out), src] = 1.0
        if name == "mlps.5":
            w[torch.randperm(n_out, generator=g)[:POS_CH], W + torch.arange(POS_CH)] = 1.0
        params[name + ".weight"] = w
        params[name + ".bias"] = (torch.randperm(2 ** 17, generator=g)[:n_out] + 1).float() * 8
    _PARAMS[key] = params
    return params


ONEHOT_M = 161                                                      # two workgroups, a ragged tail


def onehot_rows():
    """[M, 90] rows in {0 .. 3}, different from sample to sample, for the embedded entry."""
    g = torch.Generator().manual_seed(77)
    return torch.randint(0, 4, (ONEHOT_M, POS_CH + DIR_CH), generator=g).float()


def onehot_rays():
    """Rays whose every point is 0, so that the position encoding is whole numbers (sin 0 = 0, cos 0 = 1): o = 0, d = e_(n mod 3),
    z = 0.  (The direction encoding is not: its columns carry no weight in ``onehot_params``.)"""
    N, S = FACTORING[ONEHOT_M]
    d = torch.zeros(N, 3)
    d[torch.arange(N), torch.arange(N) % 3] = 1.0
    return {"N": N, "S": S, "rays_o": torch.zeros(N, 3), "rays_d": d, "z": torch.zeros(N, S), "kinds": ["x"] * N}
