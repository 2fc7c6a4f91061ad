"""Float64 restatement of the split-K weight gradient (csrc/wgrad.hip, wgrad_split.hip, wgrad_f16.hip with their common second stage
wgrad_reduce_kernel and csrc/heads.hip::head_unfuse_kernel).  CPU only; shared by tests/test_wgrad_restate.py (CPU) and
tests/test_gpu_wgrad.py (GPU).  Nothing here reads what a kernel wrote.

The weight gradient is a bilinear function of three buffers, which this module writes itself, so neither the forward nor the
ReLU masks take part in the comparison:
  save   the forward's workspace (csrc/layout.h::SaveLayout): pe [63] | de [27] | h_0 .. h_7 [256 each] | g1 [128] | g2 [128] | bit
         masks [72 rows' worth, never read by these kernels];
  dsave  the data-gradient pass's workspace, same offsets: dy_0 .. dy_7 in the h regions (pre-activation gradients of mlps.l), and
         in the g1 | g2 region ONE 256-row tensor per 32-sample block: rows 0 .. 127 = dg1, rows 128 .. 255 = dg2 (the regions of
         pe, de and the masks are not read);
  graw   the transposed d raw [Mp / 32][4 + C][32]: rows 0 .. 2 rgb, row 3 sigma, rows 4 .. the C = ins_num + 1 logits.
Every tensor is block-major [Mp / 32][rows][32] with Mp = (M + 31) & ~31.  pe, de and graw keep their rows in feature order; memory
row rho of every other tensor holds feature (rho & ~7) | ((rho & 7) >> 1) | ((rho & 1) << 2).  The padding columns M .. Mp - 1
are exact zeros in dsave and graw and finite NON-ZERO junk in save (a kernel that let padding through would show).  What the
kernels must not read (the regions named above) is NaN.

Reference (``flat_gradient``): from networks/dm_nerf.py and the algebra in the header of csrc/heads.hip, on the DECODED per-layer
matrices; in any dtype (float64 = the reference, float32 = the yardstick of the real-operand comparison) and with ``absolute=True``
on |operands| (= sum of |terms| over every sum on an entry's path, the G / Q stage and the unfuse stage included).

Cases (``CASES``): (ins_num, M, max_wgs) and the plan property each exists for; ``plan_properties`` reads the property from the
plan tables and ``check_case_properties`` asserts it, for all three cost tables.  Shape class (4, 8) (index 1 of
csrc/wgrad_common.h) is produced by no job of the current plan -- the only 128-row A operand, dg1 against de, has a 27-row B -- so no
case reaches it and none is made up for it.
"""
import collections
import ctypes

import numpy as np
import torch

W, HW, POS_CH, DIR_CH = 256, 128, 63, 27
BITS_ROWS = 72
R_PE, R_DE, R_H, R_G1, R_G2, R_BITS = 0, POS_CH, POS_CH + DIR_CH, POS_CH + DIR_CH + 8 * W, POS_CH + DIR_CH + 8 * W + HW, POS_CH + DIR_CH + 8 * W + 2 * HW
SAVE_ROWS = R_BITS + BITS_ROWS                                    # 2466

PARAM_ORDER = [f"mlps.{i}" for i in range(8)] + ["rgb_feature_linear", "ins_feature_linear", "rgb_feature_linears.0",
                                                  "ins_feature_linears.0", "density_linear", "ins_linear", "rgb_linear"]


def param_shapes(ins_num):
    sh = {"mlps.0": (W, POS_CH)}
    for l in range(1, 8):
        sh[f"mlps.{l}"] = (W, W + POS_CH) if l == 5 else (W, W)
    sh.update({"rgb_feature_linear": (W, W), "ins_feature_linear": (W, W), "rgb_feature_linears.0": (HW, W + DIR_CH),
               "ins_feature_linears.0": (HW, W), "density_linear": (1, W), "ins_linear": (ins_num + 1, HW), "rgb_linear": (3, HW)})
    return sh


def param_slices(ins_num):
    """name.weight / name.bias -> (offset, shape) in the flat vector (split_flat_grads order = state_dict order)."""
    out, o = collections.OrderedDict(), 0
    for name, (n_out, n_in) in param_shapes(ins_num).items():
        out[name + ".weight"] = (o, (n_out, n_in)); o += n_out * n_in
        out[name + ".bias"] = (o, (n_out,)); o += n_out
    return out, o


def row_len(M):
    return (M + 31) & ~31


def _mem_feature(rows):
    rho = np.arange(rows)
    return (rho & ~7) | ((rho & 7) >> 1) | ((rho & 1) << 2)


# ------------------------------------------------------------------------------------------
# encode / decode
# ------------------------------------------------------------------------------------------
def _put(buf, row0, t, Mp, perm, pad):
    """Feature-order [rows, M] -> block-major [Mp / 32][rows][32] at row offset row0 of a workspace; pad: [rows, Mp - M] or 0."""
    rows, M = t.shape
    full = torch.zeros(rows, Mp, dtype=buf.dtype)
    full[:, :M] = t
    if Mp > M and pad is not None:
        full[:, M:] = pad
    if perm:
        full = full[torch.from_numpy(_mem_feature(rows))]          # memory row rho <- feature row_feature(rho)
    buf[row0 * Mp:(row0 + rows) * Mp] = full.view(rows, Mp // 32, 32).permute(1, 0, 2).reshape(-1)


def _get(buf, row0, rows, M, Mp, perm):
    t = buf[row0 * Mp:(row0 + rows) * Mp].view(Mp // 32, rows, 32).permute(1, 0, 2).reshape(rows, Mp)
    if perm:
        t = t[torch.from_numpy(np.argsort(_mem_feature(rows)))]
    return t[:, :M].clone(), t[:, M:].clone()


def encode(ops, M, junk_seed=0, integer=False):
    """ops: pe [63, M], de [27, M], h [8, 256, M], g1, g2 [128, M], dy [8, 256, M], dg1, dg2 [128, M], graw [4 + C, M]
    (feature order) -> save, dsave, graw buffers as the kernels read them, in the operands' dtype (float32 for the kernels)."""
    Mp = row_len(M)
    dt = ops["pe"].dtype
    g = torch.Generator().manual_seed(1000 + junk_seed)

    def junk(rows):
        if Mp == M:
            return None
        if integer:
            return (torch.randint(0, 2, (rows, Mp - M), generator=g) * 2 - 1).float() * 3.0
        j = torch.randn(rows, Mp - M, generator=g)
        return j + torch.sign(j) * 2.0 + (j == 0).float()

    save = torch.full((SAVE_ROWS * Mp,), float("nan"), dtype=dt)
    dsave = torch.full((SAVE_ROWS * Mp,), float("nan"), dtype=dt)
    _put(save, R_PE, ops["pe"], Mp, False, junk(POS_CH))
    _put(save, R_DE, ops["de"], Mp, False, junk(DIR_CH))
    for l in range(8):
        _put(save, R_H + l * W, ops["h"][l], Mp, True, junk(W))
        _put(dsave, R_H + l * W, ops["dy"][l], Mp, True, None)
    _put(save, R_G1, ops["g1"], Mp, True, junk(HW))
    _put(save, R_G2, ops["g2"], Mp, True, junk(HW))
    _put(dsave, R_G1, torch.cat([ops["dg1"], ops["dg2"]], 0), Mp, True, None)      # ONE 256-row tensor per block
    C4 = ops["graw"].shape[0]
    graw = torch.empty(C4 * Mp, dtype=dt)
    _put(graw, 0, ops["graw"], Mp, False, None)
    return save, dsave, graw


def decode(save, dsave, graw, M):
    """The inverse of ``encode``: (ops, padding) -- padding holds the columns M .. Mp - 1 of every tensor, same keys."""
    Mp = row_len(M)
    ops, pad = {}, {}

    def take(key, buf, row0, rows, perm):
        ops[key], pad[key] = _get(buf, row0, rows, M, Mp, perm)
    take("pe", save, R_PE, POS_CH, False)
    take("de", save, R_DE, DIR_CH, False)
    take("g1", save, R_G1, HW, True)
    take("g2", save, R_G2, HW, True)
    take("dg12", dsave, R_G1, 2 * HW, True)
    for key, buf in (("h", save), ("dy", dsave)):
        parts = [_get(buf, R_H + l * W, W, M, Mp, True) for l in range(8)]
        ops[key], pad[key] = torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts])
    for d in (ops, pad):
        d["dg1"], d["dg2"] = d["dg12"][:HW].clone(), d["dg12"][HW:].clone()
        del d["dg12"]
    take("graw", graw, 0, graw.numel() // Mp, False)
    return ops, pad


# ------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------
def flat_gradient(ops, params, ins_num, dtype=torch.float64, absolute=False):
    """The flat parameter gradient (split_flat_grads order) from decoded operands and the parameters head_unfuse reads."""
    cv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    pe, de, h, g1, g2 = (cv(ops[k]) for k in ("pe", "de", "h", "g1", "g2"))
    dy, dg1, dg2, graw = (cv(ops[k]) for k in ("dy", "dg1", "dg2", "graw"))
    grads = {}
    for l in range(8):                                             # mlps.l: y_l = W_l x_l + b_l, x_0 = pe, x_5 = [h_4 | pe] (dm_nerf.py:87)
        x = pe if l == 0 else (torch.cat([h[4], pe], 0) if l == 5 else h[l - 1])
        grads[f"mlps.{l}.weight"] = dy[l] @ x.T
        grads[f"mlps.{l}.bias"] = dy[l].sum(1)
    h7 = h[7]
    G, Q, s1, s2 = dg1 @ h7.T, dg2 @ h7.T, dg1.sum(1), dg2.sum(1)
    W_rf, b_rf = cv(params["rgb_feature_linear.weight"]), cv(params["rgb_feature_linear.bias"])
    W_if, b_if = cv(params["ins_feature_linear.weight"]), cv(params["ins_feature_linear.bias"])
    A, W_ih = cv(params["rgb_feature_linears.0.weight"])[:, :W], cv(params["ins_feature_linears.0.weight"])
    grads["rgb_feature_linear.weight"], grads["rgb_feature_linear.bias"] = A.T @ G, A.T @ s1
    grads["ins_feature_linear.weight"], grads["ins_feature_linear.bias"] = W_ih.T @ Q, W_ih.T @ s2
    grads["rgb_feature_linears.0.weight"] = torch.cat([G @ W_rf.T + torch.outer(s1, b_rf), dg1 @ de.T], 1)      # cat[feature, dirs] (:90)
    grads["rgb_feature_linears.0.bias"] = s1
    grads["ins_feature_linears.0.weight"] = Q @ W_if.T + torch.outer(s2, b_if)
    grads["ins_feature_linears.0.bias"] = s2
    for name, rows, x in (("density_linear", graw[3:4], h7), ("ins_linear", graw[4:], g2), ("rgb_linear", graw[0:3], g1)):
        grads[name + ".weight"] = rows @ x.T
        grads[name + ".bias"] = rows.sum(1)
    sl, total = param_slices(ins_num)
    flat = torch.empty(total, dtype=dtype)
    for k, (o, shape) in sl.items():
        assert tuple(grads[k].shape) == shape, (k, grads[k].shape, shape)
        flat[o:o + grads[k].numel()] = grads[k].reshape(-1)
    return flat


UNFUSED = ("rgb_feature_linear.weight", "rgb_feature_linear.bias", "ins_feature_linear.weight", "ins_feature_linear.bias",
           "rgb_feature_linears.0.weight", "ins_feature_linears.0.weight")


def through_unfuse(ins_num):
    """Bool per flat entry: formed by head_unfuse_kernel from G / Q (the 27 direction columns of rgb_feature_linears.0 are not)."""
    sl, total = param_slices(ins_num)
    m = torch.zeros(total, dtype=torch.bool)
    for k in UNFUSED:
        o, shape = sl[k]
        v = torch.ones(shape, dtype=torch.bool)
        if k == "rgb_feature_linears.0.weight":
            v[:, W:] = False
        m[o:o + v.numel()] = v.reshape(-1)
    return m


# ------------------------------------------------------------------------------------------
# operand generators
# ------------------------------------------------------------------------------------------
def _shapes(ins_num, M):
    return {"pe": (POS_CH, M), "de": (DIR_CH, M), "h": (8, W, M), "g1": (HW, M), "g2": (HW, M),
            "dy": (8, W, M), "dg1": (HW, M), "dg2": (HW, M), "graw": (4 + ins_num + 1, M)}


SAVE_KEYS = ("pe", "de", "h", "g1", "g2")


def integer_operands(ins_num, M, seed):
    """save in {-2 .. 2}, dy and d raw in {-1, 0, 1}, every parameter in {-1, -1/2, 0, 1/2, 1}: with every sum of |terms| below 2^23
    each float32 summation order, and each bf16 / f16 plane split, gives the same bits as float64."""
    g = torch.Generator().manual_seed(seed)
    ops = {k: (torch.randint(-2, 3, s, generator=g) if k in SAVE_KEYS else torch.randint(-1, 2, s, generator=g)).float()
           for k, s in _shapes(ins_num, M).items()}
    params = {}
    for name, (n_out, n_in) in param_shapes(ins_num).items():
        params[name + ".weight"] = torch.randint(-2, 3, (n_out, n_in), generator=g).float() * 0.5
        params[name + ".bias"] = torch.randint(-2, 3, (n_out,), generator=g).float() * 0.5
    return ops, params


def real_operands(ins_num, M, seed, O):
    """save: |N(0, 1)| with a third of the entries exactly 0; dy and d raw: N(0, 1) with a third exactly 0, row r scaled by
    2^(r mod 5 - 2); parameters: the oracle's ``make_weights``."""
    g = torch.Generator().manual_seed(seed)
    ops = {}
    for k, s in _shapes(ins_num, M).items():
        t = torch.randn(s, generator=g)
        if k in SAVE_KEYS:
            t = t.abs()
        t = t * (torch.rand(s, generator=g) >= 1.0 / 3.0).float()
        if k not in SAVE_KEYS:
            r = torch.arange(s[-2], dtype=torch.float32)
            t = t * torch.exp2(torch.remainder(r, 5) - 2)[:, None]
        ops[k] = t
    return ops, {k: v.clone() for k, v in O.make_weights(seed, ins_num).items()}


def flat_params(params, ins_num):
    sl, total = param_slices(ins_num)
    flat = torch.empty(total, dtype=torch.float32)
    for k, (o, shape) in sl.items():
        flat[o:o + params[k].numel()] = params[k].reshape(-1)
    return flat


# ------------------------------------------------------------------------------------------
# the plan tables and the cases
# ------------------------------------------------------------------------------------------
JOB = np.dtype([("a_off", "<i8"), ("b_off", "<i8"), ("a_R", "<i4"), ("b_R", "<i4"), ("a_row0", "<i4"), ("b_row0", "<i4"),
                ("part_off", "<i8"), ("bias_off", "<i8"), ("a_src", "<i4"), ("b_src", "<i4"), ("rowsA", "<i4"), ("rowsB", "<i4"),
                ("cls", "<i4"), ("chunk0", "<i4"), ("nchunk", "<i4"), ("follow", "<i4"), ("next", "<i4"), ("pad", "<i4")])
OUT = np.dtype([("part_off", "<i8"), ("slice_stride", "<i8"), ("bias_part_off", "<i8"), ("bias_slice_stride", "<i8"),
                ("out_off", "<i8"), ("bias_out_off", "<i8"), ("n_slices", "<i4"), ("rowsA", "<i4"), ("rowsB", "<i4"), ("ldp", "<i4"),
                ("ld_out", "<i4"), ("col_off", "<i4"), ("bias_sub", "<i4"), ("ldb", "<i4"), ("perm_a", "<i4"), ("perm_b", "<i4"),
                ("to_scratch", "<i4"), ("bias_split", "<i4"), ("bias_out_off2", "<i8")])
MODES = {"f32": ("dmnerf_wgrad_plan_sizes", "dmnerf_wgrad_plan"), "bf16x3": ("dmnerf_wgrad_plan_sizes_split", "dmnerf_wgrad_plan_split"),
         "f16x2": ("dmnerf_wgrad_plan_sizes_f16", "dmnerf_wgrad_plan_f16")}


def plan_tables(mode, ins_num, M, max_wgs):
    """(jobs, outs, part_floats, n_wgs) of the host plan (csrc/wgrad.hip::make_plan through its C entries): structured numpy arrays."""
    from dm_nerf_amd import _lib
    lib = _lib.load()
    f_sizes, f_plan = (getattr(lib, n) for n in MODES[mode])
    jb, ob, pf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    nj, no = ctypes.c_int(), ctypes.c_int()
    _lib.check(f_sizes(ins_num, M, max_wgs, ctypes.byref(jb), ctypes.byref(ob), ctypes.byref(pf), ctypes.byref(nj), ctypes.byref(no)), "sizes")
    assert jb.value % JOB.itemsize == 0 and jb.value >= nj.value * JOB.itemsize and ob.value == no.value * OUT.itemsize, "struct layouts of this test are stale"
    hj, ho = np.empty(jb.value, dtype=np.uint8), np.empty(ob.value, dtype=np.uint8)
    _lib.check(f_plan(ins_num, M, max_wgs, hj.ctypes.data_as(ctypes.c_void_p), jb.value, ho.ctypes.data_as(ctypes.c_void_p), ob.value), "plan")
    return hj.view(JOB), ho.view(OUT), pf.value, nj.value


Case = collections.namedtuple("Case", "ins_num M max_wgs followers mixed_wgs slices min_nchunk cls why")
# followers: at least this many follower items; mixed_wgs: at least this many workgroups whose items are of different shape classes;
# slices: "tail" = max n_slices > 8 and not a multiple of 8, "gt16" = that and > 16; min_nchunk: some item has at most this many
# chunks; cls: a shape class of csrc/wgrad_common.h that some job must have.  Every threshold holds for all three cost tables.
CASES = [
    Case(13, 1, 256, 3, 0, None, 2, None, "nchunk 1 under ring depths up to 6 (clamped refills); one real sample in a block of padding; a 3-follower chain of skinny classes"),
    Case(13, 32, 256, 3, 0, None, 2, None, "nchunk 1, a full block: no padding column"),
    Case(13, 33, 256, 3, 0, None, 2, None, "nchunk 2: one full block and one sample in a block of padding"),
    Case(13, 257, 256, 0, 0, None, None, None, "9 chunks: one slice just above the 8-chunk minimum"),
    Case(13, 511, 32, 0, 0, None, None, None, "first 2-slice outputs (8 + 8 chunks)"),
    Case(13, 3000, 32, 8, 3, None, None, None, ">= 8 follower items; >= 3 workgroups whose items are of different shape classes"),
    Case(13, 3000, 256, 0, 0, "tail", None, None, "outputs with 11 slices (one unrolled trip + tail of 3), G / Q scratch output included"),
    Case(93, 6001, 32, 0, 1, None, None, 7, "class (3, 4): C = 94; mixed-class workgroups"),
    Case(127, 4001, 40, 9, 0, None, None, 8, "class (4, 4): C = 128; >= 9 followers"),
    Case(59, 8001, 256, 0, 0, "gt16", None, 6, "class (2, 4); 25 - 28 slices (three trips + tail); ~250 workgroups"),
    Case(1, 4001, 32, 0, 0, None, None, None, "C = 2: two valid rows in a 32-row A block"),
    Case(13, 12001, 256, 0, 0, "gt16", None, None, "26 - 29 slices; every workgroup of a 256-CU launch used; M not a multiple of 32"),
]


def case_id(c):
    return f"ins{c.ins_num}_M{c.M}_wgs{c.max_wgs}"


def wg_items(jobs, n_wgs):
    """Per workgroup: its items in the order it runs them (leader, then its followers from ``next`` on)."""
    return [np.concatenate([jobs[i:i + 1], jobs[jobs["next"][i]:jobs["next"][i] + jobs["follow"][i]]]) if jobs["follow"][i] > 0 else jobs[i:i + 1]
            for i in range(n_wgs)]


def plan_properties(jobs, outs, n_wgs):
    items = wg_items(jobs, n_wgs)
    return {"followers": int(len(jobs) - n_wgs),
            "longest_chain": int(jobs["follow"][:n_wgs].max()),
            "mixed_wgs": sum(1 for it in items if len(set(it["cls"].tolist())) > 1),
            "max_slices": int(outs["n_slices"].max()),
            "scratch_slices": int(outs["n_slices"][outs["to_scratch"] == 1].max()),
            "min_nchunk": int(jobs["nchunk"].min()),
            "classes": set(jobs["cls"].tolist()),
            "n_wgs": int(n_wgs)}


def check_case_properties(case, mode):
    """Asserts that the plan of ``case`` under the cost table ``mode`` still has what the case exists for; returns the properties."""
    jobs, outs, _, n_wgs = plan_tables(mode, case.ins_num, case.M, case.max_wgs)
    p = plan_properties(jobs, outs, n_wgs)
    tag = (case_id(case), mode, case.why, p)
    nchunks = row_len(case.M) // 32
    assert p["followers"] >= case.followers, tag
    if case.followers == 3:
        assert p["longest_chain"] >= 3, tag                        # one workgroup runs four items of skinny classes
    assert p["mixed_wgs"] >= case.mixed_wgs, tag
    if case.slices:
        assert p["max_slices"] > 8 and p["max_slices"] % 8 != 0, tag
        assert p["scratch_slices"] > 8 and p["scratch_slices"] % 8 != 0, tag
        if case.slices == "gt16":
            assert p["max_slices"] > 16 and p["scratch_slices"] > 16, tag
    if case.min_nchunk is not None:
        assert p["min_nchunk"] <= case.min_nchunk and nchunks <= case.min_nchunk, tag
    if case.cls is not None:
        assert case.cls in p["classes"], tag
    if case.M == 257:
        assert nchunks == 9 and p["max_slices"] == 1, tag
    if case.M == 511:
        assert p["max_slices"] == 2 and bool((jobs["nchunk"][np.isin(jobs["part_off"], outs["part_off"][outs["n_slices"] == 2])] == 8).all()), tag
    if case.max_wgs == 256 and case.M >= 8001:
        assert p["n_wgs"] >= 240, tag                              # (nearly) every workgroup of a 256-CU launch
    return p


def entry_map(outs, ins_num):
    """Per flat gradient entry: the output (index into ``outs``) whose partial tiles it was reduced from -- for the entries formed by
    head_unfuse_kernel the scratch output [G ; Q] -- following the addressing of wgrad_reduce_kernel.  Asserts that the outputs and
    the unfuse stage together write every entry exactly once."""
    sl, total = param_slices(ins_num)
    owner = np.full(total, -1, dtype=np.int64)
    count = np.zeros(total, dtype=np.int64)
    scratch = -1
    for k, o in enumerate(outs):
        ra, rb = np.arange(o["rowsA"]), np.arange(o["rowsB"])
        ro = _mem_feature(o["rowsA"])[ra] if o["perm_a"] else ra
        co = _mem_feature(o["rowsB"])[rb] if o["perm_b"] else rb
        if o["to_scratch"]:
            scratch = k
        else:
            idx = (o["out_off"] + ro[:, None] * o["ld_out"] + o["col_off"] + co[None, :]).reshape(-1)
            owner[idx] = k
            np.add.at(count, idx, 1)
        if o["bias_out_off"] >= 0:
            lo = o["bias_split"] > 0
            idx = np.where(lo & (ro >= o["bias_split"]), o["bias_out_off2"] + ro - o["bias_split"], o["bias_out_off"] + ro)
            owner[idx] = k
            np.add.at(count, idx, 1)
    assert scratch >= 0
    uf = through_unfuse(ins_num).numpy()
    owner[uf] = scratch
    count[uf] += 1
    assert bool((count == 1).all()), "an entry of the flat gradient is written by no output, or by two"
    return owner


def describe_entry(flat_index, owner, outs, ins_num):
    """'parameter[index], job k: rowsA x rowsB in n slices' for a failure message."""
    sl, _ = param_slices(ins_num)
    for name, (o, shape) in sl.items():
        n = int(np.prod(shape))
        if o <= flat_index < o + n:
            idx = tuple(int(i) for i in np.unravel_index(flat_index - o, shape))
            k = int(owner[flat_index])
            ou = outs[k]
            via = " through head_unfuse" if ou["to_scratch"] and not name.endswith("linears.0.bias") else ""
            return f"{name}{list(idx)}: output {k} ({int(ou['rowsA'])} x {int(ou['rowsB'])} rows, {int(ou['n_slices'])} slices{via})"
    return f"flat[{flat_index}]"


# ------------------------------------------------------------------------------------------
# references per case, computed once
# ------------------------------------------------------------------------------------------
def case_seed(case, kind):
    return 7 + 1000 * CASES.index(case) + (500 if kind == "real" else 0)


def case_buffers(case, kind, O=None):
    """(save, dsave, graw, flat parameters, params dict) of a case: float32 CPU tensors, deterministic."""
    seed = case_seed(case, kind)
    ops, params = integer_operands(case.ins_num, case.M, seed) if kind == "integer" else real_operands(case.ins_num, case.M, seed, O)
    save, dsave, graw = encode(ops, case.M, junk_seed=seed, integer=kind == "integer")
    return save, dsave, graw, flat_params(params, case.ins_num), params


_REF = {}


def case_data(case, kind):
    """((save, dsave, graw, flat parameters), reference) of a case.  The buffers are made anew on every call (deterministic; up to
    120 MB each), the reference -- {"want": float64 flat gradient, "abs": sum of |terms| per entry, "f32": the float32 yardstick
    (real operands only)} -- is computed once per (case, kind) and shared: treat it as read-only."""
    from oracle import ref_cpu as O
    save, dsave, graw, flat, params = case_buffers(case, kind, O)
    key = (CASES.index(case), kind)
    if key not in _REF:
        ops, _ = decode(save, dsave, graw, case.M)
        ref = {"want": flat_gradient(ops, params, case.ins_num), "abs": flat_gradient(ops, params, case.ins_num, absolute=True)}
        if kind == "real":
            ref["f32"] = flat_gradient(ops, params, case.ins_num, dtype=torch.float32)
        _REF[key] = ref
    return (save, dsave, graw, flat), _REF[key]


def case_reference(case, kind):
    key = (CASES.index(case), kind)
    return _REF[key] if key in _REF else case_data(case, kind)[1]
