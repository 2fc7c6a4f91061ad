"""GPU tests (-m gpu) of what the five training forwards SAVE -- dmnerf_mlp_fwd_rays_train, _train_fused (csrc/mlp_fwd_impl.h),
_train_split (csrc/mlp_split_train.hip), _train_f16 (csrc/mlp_f16_train.hip) and dmnerf_mlp_fwd_embedded_train -- against the float64
restatement of tests/_fwd_save_restate.py, on every case of its table: every logit-block count (C = 2 .. 128) crossed with 1 .. 225
samples (one sample in a block of padding, full blocks, a second workgroup with one, two and four live waves, ragged tails); the ray
entries get each M as N x S rays (the factoring is in the case id).  The data- and weight-gradient tests write this workspace
themselves; here it is read as the forwards leave it: pe, de, h_0 .. h_7, g1, g2, the ReLU bit words, and raw.

Every call gets a workspace of SAVE_ROWS x Mp floats and a raw of M (4 + C) floats, each with a guard of 32 rows' worth behind it, all
NaN.  Hygiene, checked after EVERY call of this module: the guards are still NaN (an overrun would be seen, it is not provoked), every
element of every tensor in the columns below M is written, the bit words of those columns are (saved activation > 0) re-encoded.
What the padding columns M .. Mp - 1 hold is unspecified and not looked at.

  a. INTEGER operands (embedded entry): every element of pe, de, h_0 .. h_7, g1, g2 and raw equals the float64 value; pe and de are the
     input rows bit for bit.  A failure names tensor, feature, sample, block, lane and register, with a count per tensor.
  b. THE ENCODING, read out of the four ray entries: pe rows 0 .. 2 are torch's float32 rays_o + rays_d * z bit for bit; de rows 0 .. 2
     against the float64 normalisation by the real-operand rule below; every sin / cos row against the referee's encoding of the SAVED
     rows 0 .. 2 (the encoder apart from the point arithmetic): |got - want| <= 1/2 float32 ulp of want + 4 x ALG_ABS.  The half ulp is
     the one final rounding; ALG_ABS is the error of the algorithm itself, measured on the CPU on these arguments
     (tests/test_fwd_save_restate.py::test_encoding_algorithm_against_the_referee prints it and holds the constant below to it), never
     a kernel's output; 4 is the project's usual margin.  4 x ALG_ABS = 8.4e-9 IS ABOVE 1e-9: the double-angle recurrence multiplies
     the polynomial's truncation error at the fold (6e-12) by up to 4 per octave, which csrc/mlp_common.h's header does not count; the
     measured value is kept -- a seventh of a float32 half ulp at 1, thirty times inside the encoding's 2.4e-7 contract.  All four
     entries give the same bits.
  c. LAYER BY LAYER from the kernel's own saved inputs (real parameters, all five entries): want = layer_from_saved(saved inputs) in
     float64, so every comparison is one GEMM deep (two for g1, g2).  f32 entries (fmaf chains, csrc/mlp_fwd_impl.h's header), per
     ELEMENT: |got - want| <= n 2^-24 sum|terms|, n = the products of the element's GEMM(s) + 3 each (DR.STAGE_ROUNDINGS).  The other
     three, per tensor: max|got - want| <= FACTOR x max|float32 CPU evaluation - float64| + 8 float32 ulp of max|want|, FACTOR = 4
     (the rule of tests/test_gpu_ray_edges.py, test_gpu_wgrad.py, test_gpu_dgrad.py).  ReLU needs no care: |relu a - relu b| <= |a - b|.
  e. ROW ORDER by one-hot weights (C = 14 and 94; f32 ray entry and embedded entry): every feature of every saved tensor of a sample
     carries its own whole number, and memory row rho holds feature (rho & ~7) | ((rho & 7) >> 1) | ((rho & 1) << 2).
  f. Two calls on the same inputs give the same bits.

OBSERVED on an MI355X: see OBSERVED below the imports (the module prints these figures when it finishes).
"""

import pytest
import torch

import _dgrad_restate as DR
import _fwd_save_restate as FR
import _gpu
import _wgrad_restate as WR
from _gpu import ulp32

pytestmark = pytest.mark.gpu

# pytest -s tests/test_fwd_save_restate.py -k algorithm   ->   "ALG_ABS = 2.063e-09" (points, octave k = 9)
ALG_ABS = 2.07e-9
FACTOR = 4.0

OBSERVED = """
Measured on an MI355X, all 48 cases, 148 tests in 5.4 s; nothing failed and no kernel was changed.
a, e, f: exact in every element; d held after every call.
b: the four ray entries give the same bits; pe rows 0 .. 2 bit-equal; de rows 0 .. 2 inside the 8 ulp alone (0.00 x the yardstick); the
   sin / cos rows need at most 1/2 ulp + 7.77e-10 = 0.38 x ALG_ABS (the rule allows 4): pe sin(2^9 x), argument -4.4853..., ins13_M161_7x23.
c: the largest multiple of the float32 yardstick's error a tensor needed on top of the 8 ulp (the rule allows 4 -- no family needs
   more), over all cases:
     entry     h_0   h_1   h_2   h_3   h_4   h_5   h_6   h_7   g1    g2    rgb   sigma logits   largest error, ulp of max|want|
     f32       0     0     0.04  0.94  0     0.04  0     0     1.98  0.32  0     0     0        17.0 (g1; yardstick 7.0)
     embedded  0     0     0     0.94  0.24  0     0     0     0.51  1.03  0     0     0        12.8 (g2; yardstick 6.8)
     fused     0     0     0.04  0.94  0     0.04  0     0     0     0     0     0     0        10.0 (h_3; yardstick 4.7)
     bf16x3    0     0.34  0.72  0.65  0.54  0     0.61  0.44  0.34  0.17  0     0     0.11     11.6 (h_2; yardstick 7.2)
     f16x2     0     0.26  1.05  0.11  0.19  0.02  0.64  0.24  0.37  0     0.90  1.76  0.08     13.8 (sigma; yardstick 6.3)
   (f32 and embedded are held to the per-element bound, not to this rule; the row is printed for comparison.)  Of the per-element
   bound n 2^-24 sum|terms| the f32 and embedded entries used at most 0.11 (h_0: 63 products of arguments up to 16), 0.035 elsewhere
   (logits), 0.0014 for the two-GEMM tensors g1 and g2.
"""

ENTRIES = {"f32": ("dmnerf_mlp_fwd_rays_train", "blob"), "fused": ("dmnerf_mlp_fwd_rays_train_fused", "blob_fused"),
           "bf16x3": ("dmnerf_mlp_fwd_rays_train_split", "blob_split"), "f16x2": ("dmnerf_mlp_fwd_rays_train_f16", "blob_f16"),
           "embedded": ("dmnerf_mlp_fwd_embedded_train", "blob")}
RAY_ENTRIES = ("f32", "fused", "bf16x3", "f16x2")
FMAF_CHAINS = ("f32", "embedded")
GUARD_ROWS = 32
STATS, ENC_STATS, MODELS = {}, {}, {}


@pytest.fixture(scope="module")
def A():
    yield _gpu.namespace()
    MODELS.clear()
    for entry, st in sorted(ENC_STATS.items()):
        print(f"\n[fwd save] encoding {entry:8s}: largest (|got - want| - 1/2 ulp) = {st['over']:.3e} = {st['over'] / ALG_ABS:.2f} x ALG_ABS (the rule allows 4) at {st['where']}; "
              f"de rows 0 .. 2 need {st['de_ratio']:.2f} x the float32 yardstick + 8 ulp")
    for (entry, name), st in sorted(STATS.items()):
        print(f"\n[fwd save] {entry:8s} {name:6s}: needs {st['ratio']:.2f} x the float32 yardstick's error + 8 ulp ({st['where']}); largest error {st['ulps']:.1f} ulp of "
              f"max|want|, yardstick {st['ulps_y']:.1f} ulp" + (f"; per-element bound used to {st['bound']:.4f}" if entry in FMAF_CHAINS else ""))


def model(A, key, params, ins_num):
    """One DM_NeRF per parameter set, kept on the device (its blobs are packed once)."""
    if key not in MODELS:
        MODELS[key] = _gpu.model_from(params, ins_num, train=True)
    return MODELS[key]


def run(A, m, entry, M, rays=None, x=None):
    """One call of an entry on NaN-filled buffers with their guards: (save, raw) on the CPU, guards included."""
    L, lib = A.L, A.lib
    C, Mp = m.ins_num + 1, WR.row_len(M)
    assert lib.dmnerf_train_save_floats(M) == WR.SAVE_ROWS * Mp
    save = torch.full((WR.SAVE_ROWS * Mp + GUARD_ROWS * WR.SAVE_ROWS,), float("nan"), device="cuda")
    raw = torch.full((M * (4 + C) + GUARD_ROWS * (4 + C),), float("nan"), device="cuda")
    fn, blob = getattr(lib, ENTRIES[entry][0]), getattr(m, ENTRIES[entry][1])()
    if entry == "embedded":
        xd = x.cuda().contiguous()
        assert tuple(xd.shape) == (M, 90) and xd.dtype == torch.float32
        rc = fn(L.ptr(blob), m.ins_num, L.ptr(xd), M, L.ptr(raw), L.ptr(save), L.stream())
    else:
        o, d, z = (rays[k].cuda().contiguous() for k in ("rays_o", "rays_d", "z"))
        N, S = rays["N"], rays["S"]
        assert N * S == M and tuple(o.shape) == (N, 3) and tuple(d.shape) == (N, 3) and tuple(z.shape) == (N, S)
        rc = fn(L.ptr(blob), m.ins_num, L.ptr(o), L.ptr(d), L.ptr(z), N, S, L.ptr(raw), L.ptr(save), L.stream())
    L.check(rc, "training forward, " + entry)
    torch.cuda.synchronize()
    return save.cpu(), raw.cpu()


def decode(tag, save, raw, M, C):
    """The tensors a forward wrote, in feature order, after the hygiene checks (d) that every call of this module gets."""
    Mp = WR.row_len(M)
    n_save, n_raw = WR.SAVE_ROWS * Mp, M * (4 + C)
    assert bool(torch.isnan(save[n_save:]).all()), (tag, "wrote behind the workspace", int((~torch.isnan(save[n_save:])).sum()), (~torch.isnan(save[n_save:])).nonzero()[:4].flatten().tolist())
    assert bool(torch.isnan(raw[n_raw:]).all()), (tag, "wrote behind raw", int((~torch.isnan(raw[n_raw:])).sum()), (~torch.isnan(raw[n_raw:])).nonzero()[:4].flatten().tolist())
    ws = save[:n_save]
    t = {"pe": WR._get(ws, WR.R_PE, WR.POS_CH, M, Mp, False)[0], "de": WR._get(ws, WR.R_DE, WR.DIR_CH, M, Mp, False)[0],
         "h": torch.stack([WR._get(ws, WR.R_H + l * 256, 256, M, Mp, True)[0] for l in range(8)]),
         "g1": WR._get(ws, WR.R_G1, 128, M, Mp, True)[0], "g2": WR._get(ws, WR.R_G2, 128, M, Mp, True)[0],
         "raw": raw[:n_raw].view(M, 4 + C).T.contiguous()}
    unwritten = {k: int(torch.isnan(v).sum()) for k, v in t.items() if bool(torch.isnan(v).any())}
    assert not unwritten, (tag, "NaN or unwritten elements in the columns below M", unwritten)
    words = DR.save_words(ws, M)
    saved, pad = DR.words_masks(words, M)
    mine = {k: t[k] > 0 for k in ("h", "g1", "g2")}
    for k in mine:
        diff = mine[k] != saved[k]
        assert not bool(diff.any()), (tag, "bit words are not (saved > 0)", k, int(diff.sum()), diff.nonzero()[:4].tolist())
    assert torch.equal(DR.mask_words(mine, M, pad), words), (tag, "bit words do not re-encode")
    return t


def pick(t, name, C):
    if name.startswith("h_"):
        return t["h"][int(name[2:])]
    return t[name] if name in t else t["raw"][FR.raw_rows(name, C)]


def first_wrong(name, bad, got, want, limit=4):
    lines = []
    for f, s in bad.nonzero()[:limit].tolist():
        at = " (block %d, lane %d, register %d)" % DR.where(f, s)[:3] if name in FR.TENSORS[:10] else f" (block {s >> 5}, lane {s & 31})"
        lines.append(f"{name}[feature {f}, sample {s}]{at}: got {float(got[f, s])!r}, want {float(want[f, s])!r}")
    return lines


def exact(tag, t, want, C):
    """Every element of pe, de, h_0 .. h_7, g1, g2 and raw equals ``want`` (float64, feature order)."""
    lines, counts = [], {}
    for name in ["pe", "de"] + FR.TENSORS:
        got, w = pick(t, name, C), pick(want, name, C)
        bad = got.double() != w
        if bool(bad.any()):
            counts[name] = f"{int(bad.sum())} of {bad.numel()}"
            lines += first_wrong(name, bad, got, w)
    if counts:
        pytest.fail(f"{tag}: wrong elements per tensor {counts}\n  " + "\n  ".join(lines[:24]))


# ------------------------------------------------------------------------------------------
# a. integer operands
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_integer_operands_are_saved_exactly(A, case):
    params, x = FR.integer_set(case.ins_num), FR.integer_rows(case)
    m = model(A, (case.ins_num, "integer"), params, case.ins_num)
    C = case.ins_num + 1
    tag = f"{FR.case_id(case)} embedded, integer operands"
    t = decode(tag, *run(A, m, "embedded", case.M, x=x), case.M, C)
    pe, de = x[:, :63].T.contiguous(), x[:, 63:].T.contiguous()
    assert torch.equal(t["pe"].view(torch.int32), pe.view(torch.int32)) and torch.equal(t["de"].view(torch.int32), de.view(torch.int32)), (tag, "pe / de are not the input rows")
    want = FR.forward_tensors(params, pe, de, torch.float64)
    want.update(pe=pe.double(), de=de.double())
    exact(tag, t, want, C)


# ------------------------------------------------------------------------------------------
# b. the encoding
# ------------------------------------------------------------------------------------------
def describe_row(row, L):
    if row < 3:
        return "xyz"[row]
    k, r = divmod(row - 3, 6)
    return f"{'sin' if r < 3 else 'cos'}(2^{k} {'xyz'[r % 3]})"


@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_encoding_read_out_of_the_ray_entries(A, case):
    rays = FR.case_rays(case)
    m = model(A, (case.ins_num, "real"), DR.case_params(case.ins_num, "real"), case.ins_num)
    M, C = case.M, case.ins_num + 1
    pts = FR.ray_points(rays)
    d64, d32 = FR.ray_dirs(rays, torch.float64), FR.ray_dirs(rays, torch.float32)
    first, failures = None, []
    for entry in RAY_ENTRIES:
        tag = f"{FR.case_id(case)} {entry}"
        t = decode(tag, *run(A, m, entry, M, rays=rays), M, C)
        st = ENC_STATS.setdefault(entry, {"over": 0.0, "where": "-", "de_ratio": 0.0})
        bad = t["pe"][:3].view(torch.int32) != pts.view(torch.int32)
        if bool(bad.any()):
            c, s = bad.nonzero()[0].tolist()
            failures.append((entry, "pe rows 0 .. 2 are not float32 o + d z", int(bad.sum()), f"{'xyz'[c]} of sample {s} (ray kind {rays['kinds'][s // rays['S']]}): got {float(t['pe'][c, s])!r}, want {float(pts[c, s])!r}"))
        e, y = float((t["de"][:3].double() - d64).abs().max()), float((d32.double() - d64).abs().max())
        u = ulp32(float(d64.abs().max()))
        st["de_ratio"] = max(st["de_ratio"], max(e - 8 * u, 0.0) / max(y, 1e-300))
        if e > FACTOR * y + 8 * u:
            failures.append((entry, "de rows 0 .. 2", "err", e, "yardstick", y, "ulp", u))
        for key, L in (("pe", FR.POS_L), ("de", FR.DIR_L)):
            got = t[key]
            want = FR.encode_rows(got[:3].contiguous(), L, torch.float64)          # of the SAVED rows 0 .. 2
            over = (got.double() - want).abs() - 0.5 * FR.ulp32_of(want)
            worst = int(over.flatten().argmax())
            row, s = worst // M, worst % M
            if float(over.max()) > st["over"]:
                st["over"], st["where"] = float(over.max()), f"{FR.case_id(case)} {key} {describe_row(row, L)} of sample {s}, argument {float(got[row % 3 if row < 3 else (row - 3) % 3, s])!r}"
            badm = over > 4 * ALG_ABS
            if bool(badm.any()):
                failures.append((entry, key, f"{int(badm.sum())} of {badm.numel()} outside 1/2 ulp + 4 ALG_ABS; worst {describe_row(row, L)} of sample {s} (block {s >> 5}, lane {s & 31} / {(s & 31) + 32}), "
                                 f"argument {float(got[(row - 3) % 3 if row >= 3 else row, s])!r}: got {float(got[row, s])!r}, want {float(want[row, s])!r}, over by {float(over.max()):.3e}"))
        if first is None:
            first = t
        else:
            for key in ("pe", "de"):
                diff = t[key].view(torch.int32) != first[key].view(torch.int32)
                if bool(diff.any()):
                    failures.append((entry, key, "not the bits of the f32 entry", int(diff.sum()), diff.nonzero()[:4].tolist()))
    assert not failures, (FR.case_id(case), failures)


# ------------------------------------------------------------------------------------------
# c. layer by layer from the kernel's own inputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FR.CASES, ids=FR.case_id)
def test_every_layer_from_the_kernels_own_saved_inputs(A, case):
    rays = FR.case_rays(case)
    params = DR.case_params(case.ins_num, "real")
    m = model(A, (case.ins_num, "real"), params, case.ins_num)
    M, C = case.M, case.ins_num + 1
    failures = []
    for entry in ENTRIES:
        tag = f"{FR.case_id(case)} {entry}"
        if entry == "embedded":
            x = FR.embedded_rows(rays)
            t = decode(tag, *run(A, m, entry, M, x=x), M, C)
            assert torch.equal(t["pe"].view(torch.int32), x[:, :63].T.contiguous().view(torch.int32)) and torch.equal(t["de"].view(torch.int32), x[:, 63:].T.contiguous().view(torch.int32)), (tag, "pe / de are not the input rows")
        else:
            t = decode(tag, *run(A, m, entry, M, rays=rays), M, C)
        for name in FR.TENSORS:
            got = pick(t, name, C)
            want = FR.layer_from_saved(params, name, t, torch.float64)
            f32 = FR.layer_from_saved(params, name, t, torch.float32)
            err = (got.double() - want).abs()
            scale, e, y = float(want.abs().max()), float(err.max()), float((f32.double() - want).abs().max())
            u = ulp32(scale)
            ratio = max(e - 8 * u, 0.0) / max(y, 1e-300)
            eu, yu = (e / u, y / u) if u > 0 else (0.0, 0.0)
            st = STATS.setdefault((entry, name), {"ratio": 0.0, "ulps": 0.0, "ulps_y": 0.0, "where": "-", "bound": 0.0})
            if ratio > st["ratio"]:
                st["ratio"], st["where"] = ratio, FR.case_id(case)
            st["ulps"], st["ulps_y"] = max(st["ulps"], eu), max(st["ulps_y"], yu)
            print(f"{tag} {name}: err {e:.3e} = {eu:.1f} ulp of max|want| {scale:.3e}, yardstick {y:.3e} = {yu:.1f} ulp, needs {ratio:.2f} x + 8 ulp")
            if entry in FMAF_CHAINS:
                bound = FR.roundings(name) * 2.0 ** -24 * FR.layer_from_saved(params, name, t, torch.float64, absolute=True)
                used = err / bound.clamp(min=1e-300)
                st["bound"] = max(st["bound"], float(used.max()))
                bad = err > bound
                if bool(bad.any()):
                    failures.append((entry, name, f"{int(bad.sum())} of {bad.numel()} outside the per-element bound", first_wrong(name, bad, got, want, 2), "worst uses", float(used.max())))
            elif e > FACTOR * y + 8 * u:
                failures.append((entry, name, "err", e, "yardstick", y, "ulp", u, "needs", ratio, first_wrong(name, err == err.max(), got, want, 1)))
    assert not failures, (FR.case_id(case), failures)


# ------------------------------------------------------------------------------------------
# e. row order, by one-hot weights
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_num", [13, 93])
def test_row_order_pinned_by_onehot_weights(A, ins_num):
    params = FR.onehot_params(ins_num)
    m = model(A, (ins_num, "onehot"), params, ins_num)
    M, C = FR.ONEHOT_M, ins_num + 1
    Mp = WR.row_len(M)
    x, rays = FR.onehot_rows(), FR.onehot_rays()
    for entry in ("f32", "embedded"):
        tag = f"one-hot weights, ins_num {ins_num}, {entry}"
        save, raw = run(A, m, entry, M, rays=rays, x=x)
        t = decode(tag, save, raw, M, C)
        if entry == "embedded":
            pe, de = x[:, :63].T.contiguous(), x[:, 63:].T.contiguous()
        else:
            pe, de = t["pe"], t["de"]                              # whole numbers (every point is 0); de carries no weight
            assert bool((pe == torch.round(pe)).all()) and float(pe.abs().max()) == 1.0
        want = FR.forward_tensors(params, pe, de, torch.float64)
        want.update(pe=pe.double(), de=de.double())
        exact(tag, t, want, C)
        # ... and the memory rows spelled out, without the decoder's own table: row rho of every block holds one feature's values
        for name, row0, rows in [(f"h_{l}", WR.R_H + l * 256, 256) for l in range(8)] + [("g1", WR.R_G1, 128), ("g2", WR.R_G2, 128)]:
            mem = save[row0 * Mp:(row0 + rows) * Mp].view(Mp // 32, rows, 32)
            w = pick(want, name, C)
            for rho in range(rows):
                feature = (rho & ~7) | ((rho & 7) >> 1) | ((rho & 1) << 2)
                got = mem[:, rho, :].reshape(Mp)[:M].double()
                if not torch.equal(got, w[feature]):
                    s = int((got != w[feature]).nonzero()[0])
                    holds = (w[:, s] == got[s]).nonzero().flatten().tolist()
                    pytest.fail(f"{tag}: memory row {rho} of {name} should hold feature {feature}; at sample {s} it holds {float(got[s])!r}, the value of feature {holds}, want {float(w[feature, s])!r}")


# ------------------------------------------------------------------------------------------
# f. determinism
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [DR.Case(13, 161), DR.Case(127, 33)], ids=FR.case_id)
def test_two_calls_give_the_same_bits(A, case):
    rays = FR.case_rays(case)
    m = model(A, (case.ins_num, "real"), DR.case_params(case.ins_num, "real"), case.ins_num)
    M, C = case.M, case.ins_num + 1
    x = FR.embedded_rows(rays)
    for entry in ENTRIES:
        a, b = (decode(f"{FR.case_id(case)} {entry}, call {i}", *run(A, m, entry, M, rays=rays, x=x), M, C) for i in (1, 2))
        for k in a:                                                # (the columns below M: the padding columns are unspecified)
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (entry, k, int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()))
