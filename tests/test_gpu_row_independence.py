"""GPU tests (-m gpu): a sample's output depends on that sample alone, also when a NEIGHBOUR is not finite.

Sharded frames are bit-identical for every world size (test_gpu_manipulator_frame.py, test_distributed_gloo.py) because every
kernel treats rows independently.  These tests hold each inference path to that with poison: a batch runs clean, then again with one
row (or one ray) made non-finite, and every OTHER row must be EQUAL to the clean run; in the poisoned row a non-finite entry appears
only where the float32 oracle's is non-finite (a NaN in the last direction-encoding column may reach rgb, never density or ins).
(Only "where", not "wherever": the kernels' ReLU is an integer max with 0 (mlp_common.h relu1), which keeps a NaN whose sign bit is
clear and maps one whose sign bit is set to 0, as it does -inf; torch.relu keeps every NaN.  A NaN the hardware generates -- inf - inf
after an Inf input, 0 * inf in the normalisation of a zero direction -- can therefore end at a ReLU where the reference's propagates.)
Poisoned positions: the first row, either side of a 128-row tile boundary (126 / 127 / 128) and the last row.  The generic path (dm_nerf_amd/generic.py) is
run at encodings whose width is not a multiple of 32 (27 / 39 and 3 columns): its GEMMs fetch the A operand in 32-column chunks from
each row start (csrc/gemm_nt.hip, gemm_chain.hip), so a row shorter than the chunks would read its neighbour's first columns."""
import types

import numpy as np
import pytest
import torch

from _gpu import A  # noqa: F401
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

M_ROWS = 300                                   # two full 128-row tiles and a ragged third
ROWS = [0, 126, 127, 128, M_ROWS - 1]
NAN, INF = float("nan"), float("inf")

# (D, W, multires, multires_views, ins_num): the shipped shape and two generic ones
SHIPPED = (8, 256, 10, 4, 13)
GENERIC = [(6, 128, 6, 4, 13),                 # 39- and 27-column encodings (rows of 40 / 28 floats before padding)
           (3, 64, 0, 0, 5)]                   # 3-column encodings: one chunk spans the row and seven more


def make_model(A, shape, seed):
    D, W, Lp, Lv, ins_num = shape
    inp, inv = 3 + 6 * Lp, 3 + 6 * Lv
    sd = O.make_weights(seed, ins_num, W=W, D=D, gain=1.7, sigma_bias=0.3, input_ch_pts=inp, input_ch_views=inv)
    m = A.M.DM_NeRF(D, W, inp, inv, [4], ins_num)
    m.load_state_dict(sd)
    return m.cuda().eval(), sd


def embedded_rows(shape, seed):
    _, _, Lp, Lv, _ = shape
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(M_ROWS, 3, generator=g) * 2 - 1) * 5.0
    dirs = torch.nn.functional.normalize(torch.randn(M_ROWS, 3, generator=g), dim=-1)
    return torch.cat([O.embed(pts, Lp), O.embed(dirs, Lv)], -1)


def assert_only_row_changed(clean, poisoned, r, what):
    """Every row but ``r`` equal to the clean run (bit for bit, NaN never equal: the clean run has none)."""
    assert bool(torch.isfinite(clean).all()), what
    keep = torch.ones(clean.shape[0], dtype=torch.bool)
    keep[r] = False
    diff = (clean[keep] != poisoned[keep]).reshape(int(keep.sum()), -1).any(-1)
    bad = torch.nonzero(keep).reshape(-1)[diff].tolist()
    assert not bad, f"{what}: poisoning row {r} changed rows {bad}"


def assert_nonfinite_within_oracle(got, want, what):
    """Every non-finite entry of the poisoned row is non-finite in the oracle's too (see the module docstring for why not '==')."""
    extra = ~torch.isfinite(got) & torch.isfinite(want)
    assert not bool(extra.any()), (what, extra.nonzero().tolist()[:8])


def run_embedded_poison(A, m, sd, shape, x, monkeypatch, chain):
    D, W, Lp, Lv, _ = shape
    inp, inv = 3 + 6 * Lp, 3 + 6 * Lv
    monkeypatch.setenv("DMNERF_GENERIC_CHAIN", chain)
    with torch.no_grad():
        clean = m(x.cuda()).cpu()
        for col in (0, inp + inv - 1):                                   # first position column, last direction-encoding column
            for val in (NAN, INF):
                for r in ROWS:
                    xp = x.clone()
                    xp[r, col] = val
                    got = m(xp.cuda()).cpu()
                    what = f"D={D} W={W} chain={chain} col={col} value={val} row={r}"
                    assert_only_row_changed(clean, got, r, what)
                    want = O.mlp_forward(sd, xp[r:r + 1], input_ch_pts=inp, input_ch_views=inv, D=D)[0]
                    assert_nonfinite_within_oracle(got[r], want, what)
                    if col == inp + inv - 1:                             # a direction column: rgb only
                        assert bool(torch.isfinite(got[r, 3:]).all()), what


def test_embedded_rows_shipped_shape(A, monkeypatch):
    """DM_NeRF.forward on pre-embedded rows, the shipped 8 x 256 kernel (csrc/mlp_fwd_embedded.hip)."""
    m, sd = make_model(A, SHIPPED, 71)
    assert m._fused_ok()
    run_embedded_poison(A, m, sd, SHIPPED, embedded_rows(SHIPPED, 5), monkeypatch, "1")


@pytest.mark.parametrize("chain", ["1", "0"], ids=["chained", "layer_by_layer"])
@pytest.mark.parametrize("shape", GENERIC, ids=["D6_W128_L6-4", "D3_W64_L0-0"])
def test_embedded_rows_generic_shapes(A, shape, chain, monkeypatch):
    """DM_NeRF.forward on pre-embedded rows through the generic path, with its trunk chained (csrc/gemm_chain.hip) and layer by
    layer (csrc/gemm_nt.hip)."""
    m, sd = make_model(A, shape, 72)
    assert not m._fused_ok() and bool(A.lib.dmnerf_mlp_chain_supported(shape[1], 3 + 6 * shape[2]))
    run_embedded_poison(A, m, sd, shape, embedded_rows(shape, 6), monkeypatch, chain)


N_RAYS = 7
RAYS = [0, 1, 2, N_RAYS - 1]           # 64 coarse samples per ray: rays 0 / 1 fill the first 128-row tile, ray 2 starts the second


def camera_rays():
    K = O.dmsr_intrinsics(480, 640)
    ro, rd = O.get_rays_k(480, 640, K, O.pose_spherical(40.0, -65.0, 7.0))
    sel = torch.from_numpy(np.random.RandomState(9).choice(480 * 640, N_RAYS, replace=False))
    return ro.reshape(-1, 3)[sel].contiguous(), rd.reshape(-1, 3)[sel].contiguous()


def oracle_raw(sd, shape, ro, rd, z):
    """raw of one ray's samples as the reference computes it: pts = o + d z, viewdirs = d / |d| (render.py:37,49), both encoded."""
    D, W, Lp, Lv, _ = shape
    pts = ro[None, :] + rd[None, :] * z[:, None]
    vd = (rd / torch.norm(rd)).expand(z.shape[0], 3)
    x = torch.cat([O.embed(pts, Lp), O.embed(vd, Lv)], -1)
    return O.mlp_forward(sd, x, input_ch_pts=3 + 6 * Lp, input_ch_views=3 + 6 * Lv, D=D)


def run_ray_poison(A, shape, args, monkeypatch, chain="1"):
    mc, sd_c = make_model(A, shape, 81)
    mf, _ = make_model(A, shape, 82)
    monkeypatch.setenv("DMNERF_GENERIC_CHAIN", chain)
    ro, rd = camera_rays()
    z = O.z_val_sample(N_RAYS, 4.0, 15.0, 64).contiguous()
    with torch.no_grad():
        clean = {k: v.cpu() for k, v in A.R.dm_nerf(torch.stack([ro, rd]).cuda(), None, None, mc, mf, z.cuda(), args).items()}
        for name in ("rays_d=0", "rays_o=+inf"):
            for r in RAYS:
                ro_p, rd_p = ro.clone(), rd.clone()
                if name == "rays_d=0":
                    rd_p[r] = 0.0
                else:
                    ro_p[r] = INF
                got = {k: v.cpu() for k, v in A.R.dm_nerf(torch.stack([ro_p, rd_p]).cuda(), None, None, mc, mf, z.cuda(), args).items()}
                what = f"shape={shape} chain={chain} {name} ray={r}"
                for k in clean:                                          # coarse and fine: raw, z, rgb, ins, depth of every other ray
                    assert_only_row_changed(clean[k], got[k], r, f"{what} {k}")
                assert_nonfinite_within_oracle(got["raw_coarse"][r], oracle_raw(sd_c, shape, ro_p[r], rd_p[r], z[r]), what)
                if name == "rays_d=0":                                   # NaN view directions: rgb only
                    assert bool(torch.isfinite(got["raw_coarse"][r, :, 3:]).all()), what


@pytest.mark.parametrize("mode", ["f32", "fuse_heads", "mfma_split", "mfma_split=f16x2"])
def test_rays_end_to_end_shipped_shape(A, mode, monkeypatch):
    """dm_nerf per ray, coarse and fine, for the shipped shape's fused render in every inference mode (selected as
    test_gpu_parity.py does).  f16x2 splits each element on its own (split_f16.h): no batch-wide scale excuses a difference."""
    key, _, val = mode.partition("=")
    extra = {} if mode == "f32" else {key: (val or True)}
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None, **extra)
    run_ray_poison(A, SHIPPED, args, monkeypatch)


@pytest.mark.parametrize("chain", ["1", "0"], ids=["chained", "layer_by_layer"])
def test_rays_end_to_end_generic_shape(A, chain, monkeypatch):
    """dm_nerf per ray, coarse and fine, through the generic path (dmnerf_ray_embed + the layer GEMMs)."""
    args = types.SimpleNamespace(perturb=False, N_importance=128, is_train=False, N_ins=None)
    run_ray_poison(A, GENERIC[0], args, monkeypatch, chain)
