"""GPU tests (-m gpu) of the three data-gradient entries -- dmnerf_mlp_bwd_data (csrc/mlp_bwd.hip, f32 MFMA), _split
(csrc/mlp_bwd_split.hip, bf16x3) and _f16 (csrc/mlp_bwd_f16.hip, f16x2, with dmnerf_grad_scale) -- against the float64 restatement of
tests/_dgrad_restate.py, on every case of its table: every logit-block count and edge (C = 2 .. 128) crossed with sample counts of
1 .. 225 (one sample in a block of padding, full blocks, a second workgroup with one, two and four live waves, ragged tails).

The test writes the operands itself -- the ReLU bit masks (so no forward runs and no pre-activation sits near a ReLU boundary),
dL/draw and the parameters, loaded into a DM_NeRF whose blob(), blob_t(), blob_t_split() and blob_t_f16() the entries read, so the
transposed packers and the fold F = A[:, :256] . W_rgb_feature are under test with the kernels -- and calls the C entries directly.
The gradient workspace and the block-major dL/draw (with 32 guard rows behind it) are NaN before every call; the forward workspace
is NaN but for the bit words, and the bits of the padding columns are ONES.

INTEGER operands (tests/test_dgrad_restate.py asserts what their exactness rests on): every element of dy_0 .. dy_7, dg1, dg2 and the
dL/draw copy equals the float64 reference, the padding columns are exact zeros, the regions of pe, de and the bit masks and the
guard rows are still NaN.  A failure names tensor, feature, sample, block, lane, register, word and bit, with a count per tensor.
One bit at a time (all masks zero but one bit per probed sample and the all-ones columns above it, never-cancelling parameters):
exactly the expected entries are nonzero, which pins each word, bit, lane and half-wave.  The masks mean what the three training
forwards save: re-encoding (saved activation > 0) gives the saved bit words.  f16x2: with d_scale = {2^10, 2^-10} every output is
exactly 2^10 times the unscaled one; dmnerf_grad_scale writes exactly {2^(6 - e), 2^(e - 6)} for max |finite| = f 2^e.

REAL operands: per tensor, max |kernel - float64| <= FACTOR x max |float32 CPU evaluation of the same formulas - float64| + 8 float32
ulp of max |want| (the rule of tests/test_gpu_ray_edges.py and tests/test_gpu_wgrad.py, FACTOR = 4), the dL/draw copy bit-equal, and for
the f32 kernel per ELEMENT |got - want| <= n 2^-24 sum|terms| with n = 259 per GEMM stage behind the element + the fold's 256.

OBSERVED on an MI355X (the module prints these figures per kernel and tensor when it finishes): see OBSERVED below the imports.
"""
import math

import pytest
import torch

import _dgrad_restate as DR
import _gpu
import _wgrad_restate as WR
from _gpu import ulp32

pytestmark = pytest.mark.gpu

OBSERVED = """
Measured on an MI355X, all 48 cases.  Integer operands: all three kernels exact in every element of every case; the one-bit sweep,
the forwards' masks, the 2^10 scale and dmnerf_grad_scale exact as well.  Real operands -- the largest multiple of the float32
yardstick's error a tensor needed on top of the 8 ulp (the rule allows 4), and the largest error in float32 ulp of the tensor's
max |want| [the yardstick's own]:
  kernel          dg1          dg2               dy_7              dy_6 .. dy_1 (worst tensor)
  f32             0 x 0.6 [0.6]  0 x 5.4 [5.4]     0 x 5.3 [8.4]     0.67 x 11.5 [12.6]
  bf16x3          0 x 0.6 [0.6]  0 x 7.7 [5.4]     0 x 4.8 [8.4]     1.54 x 16.4 [12.6]
  f16x2 scaled    0 x 0.6 [0.6]  0.52 x 8.5 [5.4]  0 x 6.0 [8.4]     3.18 x 32.1 [12.6]   (on 2^s dL/draw, s from dmnerf_grad_scale)
  f16x2 unscaled  0 x 0.6 [0.6]  0.52 x 8.5 [5.4]  0 x 6.0 [8.4]     71.54 x 675 [12.6]
(dy_0, and in a third of the cases dy_1 / dy_2, lie below the all-zeros layer: exact zeros from every kernel.)  The f32 kernel used at
most 0.023 of its per-element bound.
ONE FAMILY NEEDS MORE THAN 4: the f16x2 kernel WITHOUT the gradient scale, trunk tensors dy_6 .. dy_1 -- 71.54 x at ins_num 1, M = 1
(dy_2: 1.57e-7 = 675 ulp of its max |want| of 0.003), 46 / 46 / 25 / 13 x for dy_3 .. dy_6 there, 38 x at ins_num 31, M = 1, about 5 .. 6 x
at (13, 1), (93, 1), (13, 33), (31, 31).  Cause, from the arithmetic: a f16x2 operand is hi = f16(x) and lo = f16(x - hi), both rounded
towards zero, and below |x| = 2^-4 the lo plane is a f16 SUBNORMAL with an absolute spacing of 2^-24 (tests/test_gpu_wgrad.py found
the same in the weight gradient; csrc/layout.h says it of the weights).  These operands are small -- one bit of g1 per sample and
unit-size dL/draw leave every trunk gradient below 0.1, in the failing cases below 0.03 -- so EVERY dy entry a layer consumes carries
up to 6e-8 of absolute error whatever its size, and the errors observed are 1 .. 4 x 2^-24 in absolute terms independent of
max |want|.  A float64 CPU emulation of the split (hi + lo planes rounded towards zero, the lo . lo product dropped, exact sums)
gives at ins_num 1, M = 1: dy_6 .. dy_2 = 7.4e-8, 9.9e-8, 1.35e-7, 1.89e-7, 1.48e-7 against the kernel's 6.6e-8, 1.04e-7, 1.38e-7,
1.94e-7, 1.57e-7.  This is what dmnerf_grad_scale exists for: on 2^s dL/draw (max in [32, 64)) the same kernel on the same operands
needs at most 3.18 x -- the "f16x2 scaled" row, held to the plain rule.  The unscaled family's factor is twice the observed multiple;
every other family keeps 4.
"""

KERNELS = ("f32", "bf16x3", "f16x2")
FACTOR = 4.0          # the multiple of the float32 yardstick's error a tensor may take on top of 8 ulp: the rule
# ... and the one family that needs more (OBSERVED: ONE FAMILY NEEDS MORE THAN 4): twice the observed multiple
FACTOR_F16X2_UNSCALED_TRUNK = 2 * 71.54


def factor(kern, name):
    return FACTOR_F16X2_UNSCALED_TRUNK if kern == "f16x2" and name in TENSORS[1:7] else FACTOR          # dy_1 .. dy_6

TENSORS = [f"dy_{l}" for l in range(8)] + ["dg1", "dg2"]
STATS = {}
MODELS = {}


@pytest.fixture(scope="module")
def A():
    yield _gpu.namespace()
    MODELS.clear()
    for (kern, name), st in sorted(STATS.items()):
        print(f"\n[dgrad] {kern:12s} {name:5s}: needs {st['ratio']:.2f} x the float32 yardstick's error + 8 ulp ({st['where']}); largest error "
              f"{st['ulps']:.1f} ulp of max|want|, yardstick {st['ulps_y']:.1f} ulp" + (f"; f32 per-element bound used to {st['bound']:.4f}" if kern == "f32" else ""))


def model(A, key, params, ins_num):
    """One DM_NeRF per parameter set, kept on the device (its four blobs are packed once)."""
    if key not in MODELS:
        MODELS[key] = _gpu.model_from(params, ins_num, train=True)
    return MODELS[key]


def run(A, m, kern, M, save, graw_rows, scale=None, transposed=True):
    """One call of an entry: (gradient workspace, block-major dL/draw with its guard rows) on the CPU.  save: device workspace;
    graw_rows: device [M, 4 + C]."""
    L, lib = A.L, A.lib
    C, Mp = m.ins_num + 1, WR.row_len(M)
    assert save.numel() == lib.dmnerf_train_save_floats(M) == WR.SAVE_ROWS * Mp and save.is_contiguous()
    assert tuple(graw_rows.shape) == (M, 4 + C) and graw_rows.is_contiguous() and graw_rows.dtype == torch.float32
    dsave = torch.full((WR.SAVE_ROWS * Mp,), float("nan"), device="cuda")
    gt = torch.full(((4 + C) * Mp + 32 * 32,), float("nan"), device="cuda")
    gtp = L.ptr(gt) if transposed else None
    if kern == "f32":
        rc = lib.dmnerf_mlp_bwd_data(L.ptr(m.blob()), L.ptr(m.blob_t()), m.ins_num, L.ptr(save), L.ptr(graw_rows), M, L.ptr(dsave), gtp, L.stream())
    elif kern == "bf16x3":
        rc = lib.dmnerf_mlp_bwd_data_split(L.ptr(m.blob_t_split()), m.ins_num, L.ptr(save), L.ptr(graw_rows), M, L.ptr(dsave), gtp, L.stream())
    else:
        rc = lib.dmnerf_mlp_bwd_data_f16(L.ptr(m.blob_t_f16()), m.ins_num, L.ptr(save), L.ptr(graw_rows), M, L.ptr(dsave), gtp,
                                         None if scale is None else L.ptr(scale), L.stream())
    L.check(rc, "data gradient, " + kern)
    torch.cuda.synchronize()
    return dsave.cpu(), gt.cpu()


def operands_on_device(masks, graw, M, pad=None):
    return DR.encode_save(masks, M, pad).cuda(), graw.T.contiguous().cuda()


def split_guard(gt, M, C):
    n = (4 + C) * WR.row_len(M)
    return gt[:n], gt[n:]


def exact(tag, kern, dsave, gt, want, M, C, times=1.0):
    """Every element the float64 value (times a power of two), padding exact zeros, the rest of both buffers still NaN."""
    gt, guard = split_guard(gt, M, C)
    out, pad, untouched = DR.decode_outputs(dsave, gt, M, C)
    exp = {"dy": want["dy"] * times, "dg1": want["dg1"] * times, "dg2": want["dg2"] * times, "graw": WR._get(want["graw_t"], 0, 4 + C, M, WR.row_len(M), False)[0] * times}
    lines, counts = [], {}
    for key in ("dg2", "dg1", "dy", "graw"):
        got = out[key]
        bad = torch.isnan(got) | (got.double() != exp[key])
        for l in (range(8) if key == "dy" else (None,)):
            b = bad[l] if key == "dy" else bad
            if bool(b.any()):
                name = f"dy_{l}" if key == "dy" else key
                counts[name] = f"{int(b.sum())} of {b.numel()}"
                for f, s in b.nonzero()[:4].tolist():
                    g_, w_ = (got[l, f, s], exp[key][l, f, s]) if key == "dy" else (got[f, s], exp[key][f, s])
                    at = "" if key == "graw" else " (block %d, lane %d, register %d, mask word %d bit %d)" % DR.where(f, s)
                    lines.append(f"{name}[feature {f}, sample {s}]{at}: got {float(g_)!r}, want {float(w_)!r}")
        p = pad[key]
        if p.numel() and bool(((p != 0) | torch.isnan(p)).any()):
            counts[key + " padding"] = f"{int(((p != 0) | torch.isnan(p)).sum())} of {p.numel()} not 0"
    if not bool(torch.isnan(untouched).all()):
        counts["pe / de / bit regions of dsave"] = f"{int((~torch.isnan(untouched)).sum())} written"
    if not bool(torch.isnan(guard).all()):
        counts["guard rows behind the d raw copy"] = f"{int((~torch.isnan(guard)).sum())} written"
    if counts:
        pytest.fail(f"{tag} kernel {kern}: wrong elements per tensor {counts}\n  " + "\n  ".join(lines[:24]))


@pytest.mark.parametrize("case", DR.CASES, ids=DR.case_id)
def test_integer_operands_give_the_float64_gradients_exactly(A, case):
    masks, graw, params, ref = DR.case_data(case, "integer")
    m = model(A, (case.ins_num, "integer"), params, case.ins_num)
    save, gr = operands_on_device(masks, graw, case.M)
    for kern in KERNELS:
        dsave, gt = run(A, m, kern, case.M, save, gr)
        exact(DR.case_id(case), kern, dsave, gt, ref["want"], case.M, case.ins_num + 1)


@pytest.mark.parametrize("case", DR.CASES, ids=DR.case_id)
def test_real_operands_against_float64(A, case):
    masks, graw, params, ref = DR.case_data(case, "real")
    m = model(A, (case.ins_num, "real"), params, case.ins_num)
    save, gr = operands_on_device(masks, graw, case.M)
    C, M = case.ins_num + 1, case.M
    pick = lambda d, name: d["dy"][int(name[3:])] if name.startswith("dy_") else d[name]
    failures = []
    for kern in KERNELS + ("f16x2 scaled",):
        if kern == "f16x2 scaled":                                 # as training runs it: on 2^s dL/draw, s from dmnerf_grad_scale; 2^-s is exact
            sc = torch.zeros(4, device="cuda")
            A.L.check(A.lib.dmnerf_grad_scale(A.L.ptr(gr), gr.numel(), A.L.ptr(sc), A.L.stream()), "dmnerf_grad_scale")
            dsave, gt = (t * float(sc[1]) for t in run(A, m, "f16x2", M, save, gr, scale=sc))
        else:
            dsave, gt = run(A, m, kern, M, save, gr)
        gt, guard = split_guard(gt, M, C)
        out, pad, untouched = DR.decode_outputs(dsave, gt, M, C)
        assert bool(torch.isnan(untouched).all()) and bool(torch.isnan(guard).all()), (DR.case_id(case), kern, "wrote outside its tensors")
        assert torch.equal(gt.view(torch.int32), ref["f32"]["graw_t"].view(torch.int32)), (DR.case_id(case), kern, "the d raw copy is not bit-equal")
        for name in TENSORS:
            got, want, f32, absum = (pick(d, name) for d in (out, ref["want"], ref["f32"], ref["abs"]))
            assert not bool(torch.isnan(got).any()), (DR.case_id(case), kern, name, "NaN or unwritten elements", int(torch.isnan(got).sum()))
            assert bool((pick(pad, name) == 0).all()), (DR.case_id(case), kern, name, "padding columns not 0")
            err = (got.double() - want).abs()
            scale, e, y = float(want.abs().max()), float(err.max()), float((f32.double() - want).abs().max())
            u = ulp32(scale)
            ratio = max(e - 8 * u, 0.0) / max(y, 1e-300)
            eu, yu = (e / u, y / u) if u > 0 else (0.0, 0.0)       # (max|want| = 0 below the all-zeros layer: the rule asks for exact zeros)
            st = STATS.setdefault((kern, name), {"ratio": 0.0, "ulps": 0.0, "ulps_y": 0.0, "where": "-", "bound": 0.0})
            if ratio > st["ratio"]:
                st["ratio"], st["where"] = ratio, DR.case_id(case)
            st["ulps"], st["ulps_y"] = max(st["ulps"], eu), max(st["ulps_y"], yu)
            print(f"{DR.case_id(case)} {kern} {name}: err {e:.3e} = {eu:.1f} ulp of max|want| {scale:.3e}, yardstick {y:.3e} = {yu:.1f} ulp, needs {ratio:.2f} x + 8 ulp")
            if e > factor(kern, name) * y + 8 * u:
                failures.append((kern, name, "err", e, "yardstick", y, "ulp", u, "needs", ratio))
            if kern == "f32":
                n = DR.roundings("dy" if name.startswith("dy_") else name, int(name[3:]) if name.startswith("dy_") else None)
                bound = n * 2.0 ** -24 * absum
                used = float((err / bound.clamp(min=1e-300)).max())
                st["bound"] = max(st["bound"], used)
                bad = err > bound
                if bool(bad.any()):
                    f, s = (err / bound.clamp(min=1e-300)).flatten().argmax().item() // M, (err / bound.clamp(min=1e-300)).flatten().argmax().item() % M
                    failures.append(("f32", name, "per-element bound", f"feature {f}, sample {s}", float(err[f, s]), float(bound[f, s]), int(bad.sum())))
    assert not failures, (DR.case_id(case), failures)


# ------------------------------------------------------------------------------------------
# mask addressing, one bit at a time
# ------------------------------------------------------------------------------------------
SWEEP_M, SWEEP_SAMPLES = 161, (0, 31, 32, 160)


@pytest.mark.parametrize("tensor", [f"h_{l}" for l in range(8)] + ["g1", "g2"])
def test_one_mask_bit_opens_one_element(A, tensor):
    """ins_num 13, M = 161.  Per run one target element (tensor, feature) in each of the samples 0, 31, 32 and 160 (samples are
    independent columns), the features 0, 4, 31, 32, 255 (127) rotated over the samples in five runs, so that every (feature, sample)
    pair is probed.  All masks are zero but the target bit and, in the target's sample, all of the trunk layers above it."""
    M, ins_num = SWEEP_M, 13
    params = DR.sweep_params()
    m = model(A, "sweep", params, ins_num)
    graw = torch.ones(4 + ins_num + 1, M)
    feats = (0, 4, 31, 32, 255) if tensor.startswith("h_") else (0, 4, 31, 32, 127)
    gr = graw.T.contiguous().cuda()
    for j in range(5):
        masks = {"h": torch.zeros(8, 256, M, dtype=torch.bool), "g1": torch.zeros(128, M, dtype=torch.bool), "g2": torch.zeros(128, M, dtype=torch.bool)}
        targets = [(feats[(i + j) % 5], s) for i, s in enumerate(SWEEP_SAMPLES)]
        for f, s in targets:
            if tensor.startswith("h_"):
                l = int(tensor[2:])
                masks["h"][l, f, s] = True
                masks["h"][l + 1:, :, s] = True
            else:
                masks[tensor][f, s] = True
        want = DR.reference(masks, graw, params, ins_num)
        # the reference itself has exactly the expected support: the targets, and the full columns above a trunk target
        hit = want["dy"][int(tensor[2:])] if tensor.startswith("h_") else want["d" + tensor]
        assert sorted(hit.nonzero().tolist()) == sorted([f, s] for f, s in targets)
        total = sum(int((want[k] != 0).sum()) for k in ("dy", "dg1", "dg2"))
        assert total == 4 * ((1 + 256 * (7 - int(tensor[2:]))) if tensor.startswith("h_") else 1)
        save = DR.encode_save(masks, M).cuda()
        for kern in KERNELS:
            dsave, gt = run(A, m, kern, M, save, gr)
            exact(f"one bit of {tensor}, targets {targets}", kern, dsave, gt, want, M, ins_num + 1)


# ------------------------------------------------------------------------------------------
# the masks mean what the forwards save
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ins_num,N,S", [(13, 3, 11), (13, 7, 23), (93, 3, 11), (93, 7, 23)])
def test_masks_are_what_the_training_forwards_save(A, ins_num, N, S):
    L, lib = A.L, A.lib
    M = N * S
    Mp = WR.row_len(M)
    m = model(A, (ins_num, "real"), DR.case_params(ins_num, "real"), ins_num)
    g = torch.Generator().manual_seed(400 + ins_num + M)
    rays_o, rays_d = torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda()
    z = torch.sort(torch.rand(N, S, generator=g) * 5 + 1, -1)[0].cuda()
    for name, fn, blob in (("f32", lib.dmnerf_mlp_fwd_rays_train, m.blob()), ("bf16x3", lib.dmnerf_mlp_fwd_rays_train_split, m.blob_split()),
                           ("f16x2", lib.dmnerf_mlp_fwd_rays_train_f16, m.blob_f16())):
        raw = torch.empty(N, S, 4 + ins_num + 1, device="cuda")
        save = torch.full((lib.dmnerf_train_save_floats(M),), float("nan"), device="cuda")
        assert save.numel() == WR.SAVE_ROWS * Mp
        L.check(fn(L.ptr(blob), ins_num, L.ptr(rays_o), L.ptr(rays_d), L.ptr(z), N, S, L.ptr(raw), L.ptr(save), L.stream()), "training forward, " + name)
        torch.cuda.synchronize()
        save = save.cpu()
        acts = {"h": torch.stack([WR._get(save, WR.R_H + l * 256, 256, M, Mp, True)[0] for l in range(8)]),
                "g1": WR._get(save, WR.R_G1, 128, M, Mp, True)[0], "g2": WR._get(save, WR.R_G2, 128, M, Mp, True)[0]}
        assert not any(bool(torch.isnan(v).any()) for v in acts.values()) and all(float(v.min()) >= 0 for v in acts.values()), name
        words = DR.save_words(save, M)
        saved, pad = DR.words_masks(words, M)
        mine = {k: v > 0 for k, v in acts.items()}
        for k in mine:
            diff = (mine[k] != saved[k])
            assert not bool(diff.any()), (name, k, int(diff.sum()), diff.nonzero()[:4].tolist())
            assert bool(mine[k].any()) and not bool(mine[k].all()), (name, k)      # both bit values occur
        assert torch.equal(DR.mask_words(mine, M, pad), words), name


# ------------------------------------------------------------------------------------------
# f16x2 gradient scale
# ------------------------------------------------------------------------------------------
def test_f16x2_gradient_scale_multiplies_every_output_exactly(A):
    masks, graw, params, ref = DR.scale_case_data()
    M, ins_num = graw.shape[1], 13
    m = model(A, "scale", params, ins_num)
    save, gr = operands_on_device(masks, graw, M)
    plain = run(A, m, "f16x2", M, save, gr)
    exact("no scale", "f16x2", *plain, ref["want"], M, ins_num + 1)
    ones = run(A, m, "f16x2", M, save, gr, scale=torch.tensor([1.0, 1.0], device="cuda"))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(plain, ones)), "d_scale = None is not {1, 1}"
    scaled = run(A, m, "f16x2", M, save, gr, scale=torch.tensor([1024.0, 2.0 ** -10], device="cuda"))
    exact("d_scale = {2^10, 2^-10}", "f16x2", *scaled, ref["want"], M, ins_num + 1, times=1024.0)


def scale_inputs():
    """(label, tensor to pass (possibly a view one float into its storage), expected max |finite| or 0)."""
    g = torch.Generator().manual_seed(9)
    big = 512 * 4096 * 4 + 4099                                    # more than one trip of the grid-stride loop, and a scalar tail
    out = []

    def make(label, n, at, peak, offset=0, specials=True):
        peak = float(torch.tensor(peak, dtype=torch.float32))
        t = torch.randn(n + offset, generator=g) * 0.25 * abs(peak)
        t.clamp_(-0.99 * abs(peak), 0.99 * abs(peak))
        v = t[offset:]
        if specials and n >= 3:
            idx = [i for i in {0, n // 3, n - 1, n - 2} if i != at]
            for i, bad in zip(idx, (float("inf"), float("nan"), float("-inf"), float("nan"))):
                v[i] = bad
        v[at] = peak
        out.append((label, t, offset, abs(peak)))
    make("n = 1", 1, 0, 3.7e-5)
    make("n = 3, negative maximum last", 3, 2, -0.83)
    make("n = 4097, maximum in the scalar tail", 4097, 4096, 1.7e-3)
    make("n = 4097, maximum first", 4097, 0, 91.0)
    make("n = 4097, maximum a power of two", 4097, 2000, 2.0 ** -13)
    make("n = 4097 from a pointer one float off (scalar path), maximum last", 4097, 4096, -5.3e-6, offset=1)
    make("n = 4096 from a pointer one float off, maximum first", 4096, 0, 0.031, offset=1)
    make("large n, maximum last", big, big - 1, 2.9e-4)
    make("large n, maximum in a later trip", big, big - 3 * 512 * 256 * 4 - 2, -7.7)
    make("large n, maximum first", big, 0, 0.5)
    out.append(("all zeros", torch.zeros(4097), 0, 0.0))
    out.append(("zeros, inf and nan only", torch.tensor([0.0, float("inf"), float("nan"), 0.0, float("-inf")]), 0, 0.0))
    return out


def test_grad_scale_writes_the_exact_pair(A):
    """One four-float buffer for all calls, zeroed once: the scratch words are 0 again after every call."""
    L, lib = A.L, A.lib
    buf = torch.zeros(4, device="cuda")
    for label, t, offset, peak in scale_inputs():
        finite = t[offset:][torch.isfinite(t[offset:])]
        assert float(finite.abs().max()) == peak if finite.numel() else peak == 0.0
        if peak > 0:
            f, e = math.frexp(peak)
            assert 0.5 <= f < 1 and (label.find("power of two") < 0 or f == 0.5)
            want = [2.0 ** (6 - e), 2.0 ** (e - 6)]
        else:
            want = [1.0, 1.0]
        dev = t.cuda()
        view = dev[offset:]
        assert view.data_ptr() == dev.data_ptr() + 4 * offset
        for call in range(2):                                      # the second call: same buffer, not re-zeroed
            buf[:2] = float("nan")
            L.check(lib.dmnerf_grad_scale(L.ptr(view), view.numel(), L.ptr(buf), L.stream()), "dmnerf_grad_scale")
            torch.cuda.synchronize()
            got = buf.cpu()
            assert got[:2].tolist() == want, (label, call, got.tolist(), want)
            assert got.view(torch.int32)[2:].tolist() == [0, 0], (label, call, "scratch words", got.view(torch.int32).tolist())
        del dev, view


# ------------------------------------------------------------------------------------------
# small guards
# ------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_the_transposed_copy_is_optional(A):
    case = DR.Case(93, 161)
    masks, graw, params, _ = DR.case_data(case, "real")
    m = model(A, (case.ins_num, "real"), params, case.ins_num)
    save, gr = operands_on_device(masks, graw, case.M)
    for kern in KERNELS:
        a, b = run(A, m, kern, case.M, save, gr), run(A, m, kern, case.M, save, gr)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), kern
        c = run(A, m, kern, case.M, save, gr, transposed=False)     # graw_t = null: allowed, every store of the copy is dropped
        assert torch.equal(c[0].view(torch.int32), a[0].view(torch.int32)), kern
        assert bool(torch.isnan(c[1]).all()), kern
