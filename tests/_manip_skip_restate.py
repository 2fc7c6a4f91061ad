"""Restatement of the manipulation render that skips empty space (``manipulator(..., skip=grid)``), written against its stated
semantics and sharing no code with the product's skip route:

* a sample whose cell of the grid is clear (or that lies outside the box of a grid with ``outside == "empty"``) is not evaluated and
  its row of every network output ``raw [.., 4 + C]`` is the EMPTY ROW ``E = (0, 0, 0, 0 | 0, .., 0, 1)``;
* the result is the DENSE chain with exactly those rows replaced.

So the chains below call the dense public pieces (``manipulator_nerf``, ``manipulator_render``, ``importance_resample``,
``sort_rows``, ``exchanger`` / ``edit_exchanger``) and apply ``fill_rows`` after every network call, with the flags of the numpy
select of tests/_skip_restate.py.  ``zero_rows=True`` is the naive variant (all-zero rows: label 0 for the exchanger) that the power
check of tests/test_gpu_manip_skip.py tells apart."""
import numpy as np
import torch

import _skip_restate as RS


def empty_row(C):
    """E: sigma, rgb and the object logits 0, the last ("empty") logit 1."""
    row = torch.zeros(4 + C, dtype=torch.float32)
    row[-1] = 1.0
    return row


def fill_rows(raw, flag, C, zero_rows=False):
    """``raw [.., 4 + C]`` with the rows whose ``flag [..]`` is 0 replaced by E (``zero_rows``: by zeros); flagged rows bit for bit."""
    assert raw.shape[-1] == 4 + C
    flag = torch.as_tensor(np.asarray(flag) if not torch.is_tensor(flag) else flag).to(raw.device).reshape(raw.shape[:-1])
    row = torch.zeros(4 + C, dtype=raw.dtype) if zero_rows else empty_row(C).to(raw.dtype)
    return torch.where((flag != 0)[..., None], raw, row.to(raw.device).expand_as(raw))


class GridSpec:
    """A grid as plain data: occupancy ``occ [dx,dy,dz]`` bool, box ``lo`` / ``hi``, the ``outside`` policy."""

    def __init__(self, occ, lo, hi, outside):
        self.occ, self.lo, self.hi, self.outside = np.asarray(occ, dtype=bool), tuple(lo), tuple(hi), outside
        self.dims = tuple(self.occ.shape)
        self.words = RS.pack_bits(self.occ)

    def flags(self, rays, z):
        """uint8 ``[N,S]`` of the samples ``o + d z`` (tests/_skip_restate.select)."""
        o, d = rays[0].detach().cpu().numpy(), rays[1].detach().cpu().numpy()
        return RS.select(o, d, z.detach().cpu().numpy(), self.words, self.lo, self.hi, self.dims, self.outside)[0]


class Net:
    """The dense network call followed by ``fill_rows`` at the levels named; tallies (evaluated, samples) of the filled calls and
    keeps every output (``self.raws``)."""

    def __init__(self, MA, mc, mf, args, spec, levels, zero_rows=False, split=None):
        self.MA, self.models, self.args, self.spec, self.levels = MA, {"coarse": mc, "fine": mf}, args, spec, tuple(levels)
        self.zero_rows, self.split = zero_rows, split
        self.counts, self.raws = [0, 0], []

    def __call__(self, rays, level, z=None):
        a = self.args
        raw, z = self.MA.manipulator_nerf(rays, None, None, self.models[level], a.N_samples, a.near, a.far, z_vals=z, split=self.split)
        if level in self.levels:
            flag = self.spec.flags(rays, z)
            raw = fill_rows(raw, flag, raw.shape[-1] - 4, self.zero_rows)
            self.counts[0] += int(flag.sum())
            self.counts[1] += int(flag.size)
        self.raws.append(raw)
        return raw, z


def chain_reference(MA, Hh, net, ori_rays, f_tar_rays, args, us):
    """The reference form of ``manipulator``: every moved object has target rays; the original's fine network on the merged depths
    is evaluated once per object, as the reference does."""
    us = list(us)
    n_imp = args.N_importance
    ori_raw, ori_z = net(ori_rays, "coarse")
    _, w, _, _ = MA.manipulator_render(ori_raw, ori_z, ori_rays[1])
    ori_z_full = Hh.importance_resample(ori_z, w, n_imp, u=us.pop(0))
    ori_raw_full, _ = net(ori_rays, "fine", ori_z_full)
    _, _, _, ori_acc = MA.manipulator_render(ori_raw_full, ori_z_full, ori_rays[1])
    tar_raws, tar_z0, tar_zs, tar_accs = [], [], [], []
    tar_rgb = tar_acc = None
    for tar_rays in f_tar_rays:
        tar_raw, tar_z = net(tar_rays, "coarse")
        tar_rgb, tw, _, _ = MA.manipulator_render(tar_raw, tar_z, tar_rays[1])
        tar_z_full, zs = Hh.importance_resample(tar_z, tw, n_imp, u=us.pop(0), return_samples=True)
        tar_raw_full, _ = net(tar_rays, "fine", tar_z_full)
        _, _, _, tar_acc = MA.manipulator_render(tar_raw_full, tar_z_full, tar_rays[1])
        tar_raws.append(tar_raw); tar_z0.append(tar_z); tar_zs.append(zs); tar_accs.append(tar_acc)
    ori_raw, _, _, _ = MA.exchanger(ori_raw, tar_raws, ori_acc, tar_accs, args.target_labels)
    _, w, _, _ = MA.manipulator_render(ori_raw, ori_z, ori_rays[1])
    _, ori_zs = Hh.importance_resample(ori_z, w, n_imp, u=us.pop(0), return_samples=True)
    all_zs = torch.cat(tar_zs, dim=-1)
    ori_z = MA.sort_rows(torch.cat([ori_z, ori_zs, all_zs], dim=-1))
    for idx, tar_rays in enumerate(f_tar_rays):
        ori_raw, _ = net(ori_rays, "fine", ori_z)
        tar_raws[idx], _ = net(tar_rays, "fine", MA.sort_rows(torch.cat([tar_z0[idx], ori_zs, all_zs], dim=-1)))
    ori_raw, _, _, _ = MA.exchanger(ori_raw, tar_raws, ori_acc, tar_accs, args.target_labels)
    rgb, _, _, ins = MA.manipulator_render(ori_raw, ori_z, ori_rays[1])
    return rgb, ins, tar_rgb, tar_acc


def chain_edit(MA, Hh, net, ori_rays, f_tar_rays, args, us, kinds, keep_labels):
    """The edit form: ``f_tar_rays`` holds rays for the MOVE and COPY entries only, a REMOVE reads no target, ``keep_labels`` zeroes
    every row whose own label is outside the set; the original's fine network on the merged depths is evaluated once."""
    us = list(us)
    n_imp = args.N_importance
    labels = [int(v) for v in args.target_labels]
    kinds = [MA.MOVE] * len(labels) if kinds is None else list(kinds)
    has_rays = [k != MA.REMOVE for k in kinds]

    def per_edit(with_rays):
        it = iter(with_rays)
        return [next(it) if h else None for h in has_rays]
    ori_raw, ori_z = net(ori_rays, "coarse")
    _, w, _, _ = MA.manipulator_render(ori_raw, ori_z, ori_rays[1])
    ori_z_full = Hh.importance_resample(ori_z, w, n_imp, u=us.pop(0))
    ori_raw_full, _ = net(ori_rays, "fine", ori_z_full)
    _, _, _, ori_acc = MA.manipulator_render(ori_raw_full, ori_z_full, ori_rays[1])
    tar_raws, tar_z0, tar_zs, tar_accs = [], [], [], []
    tar_rgb = tar_acc = None
    for tar_rays in f_tar_rays:
        tar_raw, tar_z = net(tar_rays, "coarse")
        tar_rgb, tw, _, _ = MA.manipulator_render(tar_raw, tar_z, tar_rays[1])
        tar_z_full, zs = Hh.importance_resample(tar_z, tw, n_imp, u=us.pop(0), return_samples=True)
        tar_raw_full, _ = net(tar_rays, "fine", tar_z_full)
        _, _, _, tar_acc = MA.manipulator_render(tar_raw_full, tar_z_full, tar_rays[1])
        tar_raws.append(tar_raw); tar_z0.append(tar_z); tar_zs.append(zs); tar_accs.append(tar_acc)
    accs = per_edit(tar_accs)
    ori_raw, _ = MA.edit_exchanger(ori_raw, per_edit(tar_raws), ori_acc, accs, labels, kinds, keep_labels, want_label=False)
    _, w, _, _ = MA.manipulator_render(ori_raw, ori_z, ori_rays[1])
    _, ori_zs = Hh.importance_resample(ori_z, w, n_imp, u=us.pop(0), return_samples=True)
    ori_zm = MA.sort_rows(torch.cat([ori_z, ori_zs] + tar_zs, dim=-1))
    ori_raw, _ = net(ori_rays, "fine", ori_zm)
    for idx, tar_rays in enumerate(f_tar_rays):
        tar_raws[idx], _ = net(tar_rays, "fine", MA.sort_rows(torch.cat([tar_z0[idx], ori_zs] + tar_zs, dim=-1)))
    ori_raw, _ = MA.edit_exchanger(ori_raw, per_edit(tar_raws), ori_acc, accs, labels, kinds, keep_labels, want_label=False)
    rgb, _, _, ins = MA.manipulator_render(ori_raw, ori_zm, ori_rays[1])
    if not f_tar_rays:
        tar_rgb, tar_acc = torch.zeros_like(rgb), torch.zeros_like(ins)
    return rgb, ins, tar_rgb, tar_acc


def chain(MA, Hh, net, ori_rays, f_tar_rays, args, us, kinds=None, keep_labels=None):
    """``manipulator``'s dispatch: the edit form as soon as ``kinds`` or ``keep_labels`` is given."""
    if kinds is not None or keep_labels is not None:
        return chain_edit(MA, Hh, net, ori_rays, list(f_tar_rays), args, us, kinds, keep_labels)
    return chain_reference(MA, Hh, net, ori_rays, f_tar_rays, args, us)


def manipulator_render_cpu(raw, z_vals, rays_d):
    """The compositing of the manipulation render, restated in torch on the CPU (used when the oracle has none):
    alpha = 1 - exp(-relu(sigma) dist), weight = alpha * prod(1 - alpha + 1e-10) over the samples in front, rgb through a sigmoid,
    the object map = sigmoid of the weighted logit sum, all C channels kept."""
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dists = torch.cat([dists, torch.full_like(dists[..., :1], 1e10)], -1) * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-torch.relu(raw[..., 3]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1. - alpha + 1e-10], -1), -1)[:, :-1]
    w = alpha * trans
    return (torch.sum(w[..., None] * torch.sigmoid(raw[..., :3]), -2), w, torch.sum(w * z_vals, -1),
            torch.sigmoid(torch.sum(w[..., None] * raw[..., 4:], -2)))


# ---- the shared case of the tests: rays of one camera and of a moved camera against a box around the scene
BOX_LO, BOX_HI = (-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)
NEAR, FAR = 4.0, 15.0


def random_spec(dims, frac, seed, outside):
    occ = np.random.RandomState(seed).rand(*dims) < frac
    return GridSpec(occ, BOX_LO, BOX_HI, outside)


def case_rays(O, n=130, T=2, start=90000, stride=97):
    """``n`` rays of a 480 x 640 frame (every ``stride``-th pixel) and the same pixels seen from ``T`` moved cameras -> CPU tensors
    ``ori [2,n,3]``, ``tars`` list of ``[2,n,3]``."""
    K = O.dmsr_intrinsics(480, 640)
    pose = O.pose_spherical(30.0, -65.0, 7.0)
    ang = 0.2
    trans = [torch.tensor([[np.cos(ang), -np.sin(ang), 0., 0.3], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]],
                          dtype=torch.float32),
             torch.tensor([[1., 0., 0., -0.4], [0., 1., 0., 0.25], [0., 0., 1., 0.], [0., 0., 0., 1.]])]
    out = []
    for p in [pose] + [t @ pose for t in trans[:T]]:
        ro, rd = O.get_rays_k(480, 640, K, p)
        idx = slice(start, start + n * stride, stride)
        out.append(torch.stack([ro.reshape(-1, 3)[idx], rd.reshape(-1, 3)[idx]]).float().contiguous())
    return out[0], out[1:]


def case_draws(n, n_imp, count, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, n_imp, generator=g) for _ in range(count)]


# ---- the power case (test 4): a skipped sample must not be taken for the moved object 0
POWER = dict(seeds=(61, 62), ins_num=13, label=0, bias0=0.2, dims=(9, 11, 10), frac=0.3, grid_seed=41, outside="empty")


def power_weights(O):
    """The two state dicts of the power case: ``make_weights`` (gain 1.7, sigma_bias 0.3) with ``ins_linear.bias[0] += bias0``, so
    that object 0 wins the accumulated label on many rays (only there can the exchanger move anything) while the per-sample labels
    of the original still vary (only a sample of ANOTHER label is wrongly overwritten by an all-zero target row)."""
    sds = []
    for seed in POWER["seeds"]:
        sd = O.make_weights(seed, POWER["ins_num"], gain=1.7, sigma_bias=0.3)
        sd["ins_linear.bias"] = sd["ins_linear.bias"].clone()
        sd["ins_linear.bias"][0] += POWER["bias0"]
        sds.append(sd)
    return sds


def oracle_chain(O, sds, ori, tars, spec, labels, us, n_samples, n_imp, zero_rows):
    """The reference form on the CPU oracle (``oracle.ref_cpu.manipulator`` with its ``net`` hook): the oracle's network, then
    ``fill_rows`` with the restated flags, at both levels."""
    def net(rays, sd, N_samples=None, near=None, far=None, z_vals=None):
        raw, z = O.manipulator_nerf(rays, sd, N_samples, near, far, z_vals=z_vals)
        return fill_rows(raw, spec.flags(rays, z), raw.shape[-1] - 4, zero_rows), z
    with torch.no_grad():
        return O.manipulator(sds[0], sds[1], ori, tars, n_samples, n_imp, NEAR, FAR, labels, us=[u.clone() for u in us], net=net)
