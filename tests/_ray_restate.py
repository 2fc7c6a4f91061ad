"""float64 restatement of the per-ray stages (plain torch on the CPU, no import from the package or the oracle), the edge-case
generators shared by tests/test_ray_restate.py (CPU) and tests/test_gpu_ray_edges.py (GPU), and the tolerance rule of both.

THE RULE FOR DISCRETE DECISIONS.  Every discrete decision is taken in float32, exactly as the reference takes it; everything
continuous is float64.  The discrete decisions are
  * the relu gate of the density, ``raw[..., 3] > 0``;
  * the penalizer's three masks, ``p < d_before``, ``p > d_after`` and their complement, with ``p = z |d|``,
    ``d_before = (depth - tol) |d|`` and ``d_after = (depth + tol) |d|`` all formed in float32;
  * ``searchsorted(cdf, u, right=True)`` on the float32 CDF and the float32 draw;
  * ``denom < 1e-5`` on the float32 difference of the two float32 CDF entries.
A float64 evaluation that took them in float64 would answer another question on the inputs below (a sample exactly on a band
edge, a draw exactly on a knot of the CDF), and the comparison would measure the decision, not the arithmetic.

What is restated: ``render_train`` (networks/render.py:6-28; gradients are autograd's on the float64 graph, the object-code path
detached from the density as in the reference), the CDF of ``sample_pdf`` from its weights and the tail of ``sample_pdf`` given a
CDF (networks/helpers.py:123-155), and ``emptiness_penalizer`` (networks/penalizer.py:5-55) with its gradient.  The float32
constants the reference forms as float32 tensors (2 deta_w^2 and 0.4 sqrt(2 pi)) are inputs: they are formed in float32 here too.

Tolerance (``bound``): per ray and per output (for d raw also per channel group rgb | sigma | ins) the error against float64
may be 4 x the float32 oracle's own error on that ray and group plus 8 float32 ulp of the group's scale, the scale being
``max |want|`` of the ray's group floored at 1e-3 of the group's maximum over the case.  Where the restatement is exactly 0
the value under test must be exactly 0 (``zeros_kept``)."""
import math

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
TOL, DETA_W = 0.05, 0.05                      # the penalizer settings every test of the suite uses


# ------------------------------------------------------------------------------------------
# restatements
# ------------------------------------------------------------------------------------------
def render_train(raw, z, rays_d, raw64=None, dtype=F64):
    """``render_train``: raw [N,S,4+C] float32 (``raw64``: the leaf to differentiate, default ``raw.to(dtype)``),
    z [N,S], rays_d [N,3] -> (rgb_map, weights, depth_map, ins_map) in ``dtype``.  S = 1 is one sample of length 1e10 |d| (the
    reference's ``expand`` leaves it no sample at all: weights [N,0] and all-zero maps)."""
    r = raw.to(dtype) if raw64 is None else raw64
    gate = raw[..., 3] > 0                                                   # float32 decision
    zz = z.to(dtype)
    dists = torch.cat([zz[:, 1:] - zz[:, :-1], torch.full_like(zz[:, :1], 1e10)], -1)
    dists = dists * torch.linalg.vector_norm(rays_d.to(dtype), dim=-1, keepdim=True)
    sigma = torch.where(gate, r[..., 3], torch.zeros_like(r[..., 3]))
    e = torch.exp(-sigma * dists)
    alpha = 1. - e
    # 1 - alpha + 1e-10: float64 forms it as e + 1e-10 (1 - (1 - e) would round e to a multiple of 1e-16, a relative 1e-6 of
    # the 1e-10 a saturated sample leaves); float32 (the S = 1 yardstick, the sampling inputs) keeps the reference's operations
    f = e + 1e-10 if dtype == F64 else 1. - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(f[:, :1]), f], -1), -1)[:, :-1]
    w = alpha * T
    rgb_map = (w[..., None] * torch.sigmoid(r[..., :3])).sum(-2)
    depth_map = (w * zz).sum(-1)
    ins_map = torch.sigmoid((w.detach()[..., None] * r[..., 4:]).sum(-2))[..., :-1]
    return rgb_map, w, depth_map, ins_map


def cotangent_sets(ct):
    """The three losses of the compositing tests: all four outputs, rgb + ins (what the reference's losses produce), ins only."""
    return {"all": (0, 1, 2, 3), "rgb_ins": (0, 3), "ins": (3,)}


def composite_loss(outs, ct, which):
    return sum((outs[i] * ct[i].to(outs[i].dtype).to(outs[i].device)).sum() for i in which)


def render_train_grads(raw, z, rays_d, ct):
    """d raw (float64) of the three losses of ``cotangent_sets``."""
    out = {}
    for name, which in cotangent_sets(ct).items():
        r = raw.double().requires_grad_(True)
        g, = torch.autograd.grad(composite_loss(render_train(raw, z, rays_d, raw64=r), ct, which), r, allow_unused=True)
        out[name] = torch.zeros_like(r) if g is None else g
    return out


def cdf_from_weights(w):
    """The CDF of ``sample_pdf`` [N, nb] in float64 from the float32 weights [N, nb-1]."""
    w = w.double() + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    return torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)


def sample_tail(bins, cdf, u):
    """The tail of ``sample_pdf`` given a float32 CDF: (samples float64 [N,n], inds int64 [N,n]).  u: [n] or [N,n] float32."""
    assert bins.dtype == F32 and cdf.dtype == F32 and u.dtype == F32
    N, nb = cdf.shape
    u = u.expand(N, -1).contiguous() if u.dim() == 1 else u.contiguous()
    inds = torch.searchsorted(cdf.contiguous(), u, right=True)              # float32 decision
    below, above = (inds - 1).clamp(min=0), inds.clamp(max=nb - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    small = (c1 - c0) < 1e-5                                                 # float32 decision (float32 difference, float32 1e-5)
    b0, b1 = torch.gather(bins, 1, below).double(), torch.gather(bins, 1, above).double()
    denom = torch.where(small, torch.ones_like(c0, dtype=F64), c1.double() - c0.double())
    t = (u.double() - c0.double()) / denom
    return b0 + t * (b1 - b0), inds


def pen_consts(deta_w=DETA_W):
    """(2 deta_w^2, 0.4 sqrt(2 pi)) as the reference forms them: float32 tensors (penalizer.py:7-10)."""
    two_w2 = float((2 * (torch.tensor([deta_w]) ** 2)).item())
    norm = float((torch.tensor([0.4]) * torch.sqrt(torch.tensor([2 * np.pi]))).item())
    return two_w2, norm


def pen_masks(z, depth, rays_d, tol=TOL):
    """(mask_before, mask_after, mask_middle) as float32 0/1 tensors, decided in float32."""
    nrm = torch.norm(rays_d[..., None, :], dim=-1)
    dep = depth.reshape(-1, 1)
    p = z * nrm
    mb = (p < (dep - tol) * nrm).float()
    ma = (p > (dep + tol) * nrm).float()
    return mb, ma, 1 - (ma + mb)


def emptiness_penalizer(raw, z, depth, rays_d, tol=TOL, deta_w=DETA_W, raw64=None):
    """``emptiness_penalizer`` in float64 -> the scalar loss (0-dim).  depth: [N] float32 (detached in the reference's caller)."""
    r = raw.double() if raw64 is None else raw64
    k2w, kh = pen_consts(deta_w)
    mb, ma, mm = (m.double() for m in pen_masks(z, depth, rays_d, tol))
    nrm = torch.linalg.vector_norm(rays_d.double(), dim=-1, keepdim=True)
    dd = depth.double().reshape(-1, 1) * nrm - z.double() * nrm
    G = torch.exp(-(dd ** 2) / k2w) / kh + 1e-8
    P = torch.sigmoid(r[..., 4:])
    C = P.shape[-1]
    gt = torch.zeros_like(P)
    gt[..., -1] = 1
    lb = -gt * torch.log(P + 1e-8) - (1 - gt) * torch.log(1 - P + 1e-8)
    loss_b = (lb * ((1 - G) * mb)[..., None]).sum() / (C * mb.sum().clamp(min=1e-8))
    lm = -torch.log(1 - P[..., -1] + 1e-8)
    loss_m = (lm * (G * mm)).sum() / mm.sum().clamp(min=1e-8)
    return loss_b + loss_m


def emptiness_penalizer_grad(raw, z, depth, rays_d, tol=TOL, deta_w=DETA_W):
    r = raw.double().requires_grad_(True)
    loss = emptiness_penalizer(raw, z, depth, rays_d, tol, deta_w, raw64=r)
    g, = torch.autograd.grad(loss, r)
    return loss.detach(), g


# ------------------------------------------------------------------------------------------
# the tolerance rule
# ------------------------------------------------------------------------------------------
def ulp32(x):
    """The float32 ulp of each (float64) magnitude (2^-149 throughout the subnormal range and below); 0 at 0."""
    x = x.double().abs()
    e = torch.floor(torch.log2(torch.where(x > 0, x, torch.ones_like(x)))).clamp(min=-126.0)
    return torch.where(x > 0, torch.pow(torch.tensor(2.0, dtype=F64), e - 23), torch.zeros_like(x))


def _rows(t):
    return t.detach().cpu().double().reshape(t.shape[0], -1)


def ray_scale(want):
    s = _rows(want).abs().max(1).values
    return torch.maximum(s, 1e-3 * s.max())


def bound(want, o32):
    """Per ray: (allowed error, the oracle's error, the scale).  want: float64 [N, ...]; o32: the float32 oracle's value."""
    err_o = (_rows(o32) - _rows(want)).abs().max(1).values
    scale = ray_scale(want)
    return 4 * err_o + 8 * ulp32(scale), err_o, scale


def compare(got, want, o32, what, stats=None):
    """Asserts the tolerance rule and the exact zeros for one output of one case; every element takes part.  Returns
    (the largest multiple of the oracle's error that a ray needed on top of the 8 ulp, the largest error in ulp of the ray's scale)."""
    assert tuple(got.shape) == tuple(want.shape) == tuple(o32.shape), (what, got.shape, want.shape, o32.shape)
    if want.numel() == 0:
        return 0.0, 0.0
    g = _rows(got)
    assert bool(torch.isfinite(g).all()), (what, "not finite")
    allowed, err_o, scale = bound(want, o32)
    err = (g - _rows(want)).abs().max(1).values
    ulps = float(torch.where(scale > 0, err / ulp32(scale).clamp(min=1e-300), torch.zeros_like(err)).max())
    # the factor of the oracle's error this output needs on top of the 8 ulp (the rule allows 4)
    over = (err - 8 * ulp32(scale)).clamp(min=0)
    ratio = float(torch.where(over > 0, over / err_o.clamp(min=1e-300), over).max())
    if stats is not None:
        stats["ratio"] = max(stats.get("ratio", 0.0), ratio)
        stats["ulps"] = max(stats.get("ulps", 0.0), ulps)
    print(f"{what}: worst ray err {float(err.max()):.3e} (oracle {float(err_o.max()):.3e}), needs {ratio:.2f} x the oracle's error + 8 ulp, {ulps:.2f} ulp of the scale")
    bad = err > allowed
    assert not bool(bad.any()), (what, "rays", bad.nonzero().flatten().tolist(), "err", err[bad].tolist(), "allowed", allowed[bad].tolist(),
                                 "oracle", err_o[bad].tolist(), "scale", scale[bad].tolist())
    zeros_kept(got, want, what)
    return ratio, ulps


def zeros_kept(got, want, what):
    z = _rows(want) == 0
    g = _rows(got)
    assert bool((g[z] == 0).all()), (what, "nonzero where the float64 value is exactly 0", int((g[z] != 0).sum()), float(g[z].abs().max()))


def d_raw_groups(t):
    """d raw [N,S,4+C] -> its three channel groups."""
    return {"rgb": t[..., :3], "sigma": t[..., 3:4], "ins": t[..., 4:]}


# ------------------------------------------------------------------------------------------
# compositing cases
# ------------------------------------------------------------------------------------------
# (S, C): S in {1, 2, 63, 64, 65, 129, 1280} x C in {1, 2, 17, 28, 29, 60, 61, 128}, pruned; S = 1, 65 and 1280 keep a C on both
# sides of 4 + C = 32; (2, 128) and (5, 94) are the backward cases whose coefficient row outgrows the sample row
COMPOSITE_SHAPES = ((1, 1), (1, 28), (1, 29), (2, 2), (2, 128), (5, 94), (63, 17), (63, 61), (64, 28), (64, 60), (65, 1), (65, 28),
                    (65, 29), (65, 128), (129, 2), (129, 61), (1280, 17), (1280, 28), (1280, 29))


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1)))


def _z_row(S, g):
    """Sorted depths in [4, 15): one per cell of width 11 / S, at least 0.2 cells apart."""
    return (4 + 11 * (torch.arange(S, dtype=F64) + 0.1 + 0.8 * torch.rand(S, generator=g, dtype=F64)) / S).float()


def _dist_row(z, d):
    nrm = torch.linalg.vector_norm(d)
    return torch.cat([z[1:] - z[:-1], torch.tensor([1e10])]) * nrm


def composite_ray(kind, S, C, g):
    """One ray (raw [S,4+C], z [S], d [3]) of the named kind; every kind starts from the same benign ray."""
    raw = torch.randn(S, 4 + C, generator=g)
    raw[:, 3] = raw[:, 3] + 0.1                                            # densities of both signs
    z = _z_row(S, g)
    d = torch.randn(3, generator=g)
    d = d * (0.5 + torch.rand(1, generator=g)) / torch.linalg.vector_norm(d)      # |d| in [0.5, 1.5)
    mid = S // 2

    def opaque(samples, tau):
        # sigma dist = tau in float32 terms (tau = 130 > 104: expf(-tau) is 0; the last sample's dist is 1e10 |d|)
        dist = _dist_row(z, d)
        for s, t in zip(samples, tau):
            s = min(s, S - 1)
            raw[s, 3] = t / dist[s]

    if kind == "benign":
        pass
    elif kind == "spike_mid":
        opaque([mid], [130.])
    elif kind == "spike_two":
        opaque([mid, mid + 1], [130., 130.])
    elif kind == "spike_first":
        opaque([0], [130.])
    elif kind == "spike_63":
        opaque([63], [130.])
    elif kind == "spike_64":
        opaque([64], [130.])
    elif kind == "alpha_round":                                            # alpha rounds to 1, exp(-tau) is not 0
        opaque(sorted({S // 3, mid, (2 * S) // 3}), [25., 50., 75.])
    elif kind == "empty":
        raw[:, 3] = -raw[:, 3].abs() - 1e-3
        raw[mid, 3] = 0.0
    elif kind == "last_only":
        raw[:, 3] = -raw[:, 3].abs() - 1e-3
        raw[S - 1, 3] = 0.7
    elif kind == "zero_dir":
        d = torch.zeros(3)
    elif kind == "equal_z":
        k = min(mid, S - 2)
        if k >= 0:
            z[k + 1] = z[k]
            raw[k, 3] = 200.0                                              # an open gate over a step of length 0
    elif kind == "rgb_sat":
        m = torch.rand(S, 3, generator=g) < 0.5
        sgn = torch.where(torch.rand(S, 3, generator=g) < 0.5, -90.0, 90.0)
        raw[:, :3] = torch.where(m, sgn, raw[:, :3])
    else:
        raise KeyError(kind)
    return raw, z, d


def composite_batches(S):
    """The two batches of every shape: N = 5 with the hardest ray alone in the partial block, and N = 5 or 6."""
    if S >= 65:
        return {"a": ("alpha_round", "empty", "last_only", "rgb_sat", "spike_63"),
                "b": ("spike_mid", "spike_two", "spike_first", "zero_dir", "equal_z", "spike_64")}
    return {"a": ("alpha_round", "empty", "last_only", "rgb_sat", "spike_two"),
            "b": ("spike_mid", "spike_first", "zero_dir", "equal_z", "benign")}


def composite_case(S, C, batch):
    kinds = composite_batches(S)[batch]
    g = _gen(1, S, C, ord(batch))
    rays = [composite_ray(k, S, C, g) for k in kinds]
    N = len(kinds)
    ct = [torch.randn(N, 3, generator=g), torch.randn(N, S, generator=g), torch.randn(N, generator=g), torch.randn(N, C - 1, generator=g)]
    return {"name": f"S{S}_C{C}_{batch}", "kinds": kinds, "raw": torch.stack([r[0] for r in rays]).contiguous(),
            "z": torch.stack([r[1] for r in rays]).contiguous(), "d": torch.stack([r[2] for r in rays]).contiguous(), "ct": ct,
            "S": S, "C": C}


def composite_case_ids():
    return [(S, C, b) for S, C in COMPOSITE_SHAPES for b in ("a", "b")]


_composite_cache = {}


def composite_reference(S, C, batch, oracle):
    """The case, its float64 truth and the float32 oracle's values (``oracle``: the module with the reference's
    ``render_train``); computed once per case.  At S = 1 the reference's own code has no sample left (see ``render_train``), so
    the float32 yardstick there is the float32 evaluation of this file's statement, which keeps the reference's operations."""
    key = (S, C, batch)
    if key not in _composite_cache:
        case = composite_case(S, C, batch)
        raw, z, d, ct = case["raw"], case["z"], case["d"], case["ct"]
        f32_render = oracle.render_train if S > 1 else (lambda r, zz, dd: render_train(r.detach(), zz, dd, raw64=r, dtype=F32))
        with torch.no_grad():
            want = [t.detach() for t in render_train(raw, z, d)]
            o32 = [t.detach() for t in f32_render(raw, z, d)]
        want_g = render_train_grads(raw, z, d, ct)
        o32_g = {}
        for name, which in cotangent_sets(ct).items():
            r = raw.clone().requires_grad_(True)
            gr, = torch.autograd.grad(composite_loss(f32_render(r, z, d), ct, which), r, allow_unused=True)
            o32_g[name] = torch.zeros_like(r) if gr is None else gr
        case.update(want=want, o32=o32, want_g=want_g, o32_g=o32_g)
        _composite_cache[key] = case
    return _composite_cache[key]


# ------------------------------------------------------------------------------------------
# penalizer cases
# ------------------------------------------------------------------------------------------
PEN_SHAPES = tuple((S, C) for S in (1, 64, 65) for C in (1, 13, 94))
PEN_BATCHES = {"mixed": ("inside", "above", "edge_before", "edge_after", "below"),     # N = 5
               "floor_before": ("below", "edge_first", "below", "edge_first", "below"),      # no sample before the band: sum m_b = 0
               "no_middle": ("above", "below", "above", "below", "above", "below")}          # no sample inside it: sum m_m = 0


def pen_ray(kind, S, C, g, tol=TOL):
    raw = torch.randn(S, 4 + C, generator=g) * 2
    z = _z_row(S, g)
    d = torch.randn(3, generator=g)
    k = S // 2
    t32 = torch.tensor(tol, dtype=F32)
    if kind == "below":                                                    # the band lies in front of every sample
        depth = z[0] - 1.0
    elif kind == "above":                                                  # every sample lies in front of the band
        depth = z[-1] + 1.0
    elif kind == "inside":
        depth = z[k] + 0.01
    elif kind in ("edge_before", "edge_first"):                            # z[k] |d| == (depth - tol) |d| in float32: not "before" (strict <)
        k = 0 if kind == "edge_first" else k                               # (edge_first: and no sample in front of it)
        depth = z[k] + t32
        z[k] = depth - t32
    elif kind == "edge_after":                                            # z[k] |d| == (depth + tol) |d| in float32: not "after" (strict >)
        depth = z[k] - t32
        z[k] = depth + t32
    else:
        raise KeyError(kind)
    return raw, z, d, depth.reshape(())


def pen_case(S, C, batch):
    g = _gen(2, S, C, len(batch))
    rays = [pen_ray(k, S, C, g) for k in PEN_BATCHES[batch]]
    case = {"name": f"S{S}_C{C}_{batch}", "kinds": PEN_BATCHES[batch], "S": S, "C": C}
    for i, key in enumerate(("raw", "z", "d", "depth")):
        case[key] = torch.stack([r[i] for r in rays]).contiguous()
    assert bool((case["z"][:, 1:] >= case["z"][:, :-1]).all())
    mb, ma, mm = pen_masks(case["z"], case["depth"], case["d"])
    if batch == "floor_before":
        assert float(mb.sum()) == 0 and float(mm.sum()) > 0
    if batch == "no_middle":
        assert float(mm.sum()) == 0 and float(mb.sum()) > 0
    if batch == "mixed":                                                   # the sample on each edge counts as inside the band
        assert float(mm[2, S // 2]) == 1 and float(mm[3, S // 2]) == 1
    return case


def pen_case_ids():
    return [(S, C, b) for S, C in PEN_SHAPES for b in PEN_BATCHES]


_pen_cache = {}


def pen_reference(S, C, batch, oracle):
    key = (S, C, batch)
    if key not in _pen_cache:
        case = pen_case(S, C, batch)
        raw, z, d, depth = case["raw"], case["z"], case["d"], case["depth"]
        loss, grad = emptiness_penalizer_grad(raw, z, depth, d)
        r = raw.clone().requires_grad_(True)
        l32 = oracle.emptiness_penalizer(r, z, depth[:, None], d, TOL, DETA_W).sum()
        g32, = torch.autograd.grad(l32, r)
        case.update(want_loss=loss, want_grad=grad, o32_loss=l32.detach(), o32_grad=g32)
        _pen_cache[key] = case
    return _pen_cache[key]


# ------------------------------------------------------------------------------------------
# sampling cases
# ------------------------------------------------------------------------------------------
SAMPLE_NB = (2, 3, 64, 65, 512)
SAMPLE_N = (1, 63, 65, 128)
SAMPLE_BATCHES = {"a": ("zeros", "spike_first", "spike_mid", "spike_last", "benign", "ray_spike_two", "ray_empty", "ray_alpha_round",
                        "ray_spike_mid"),                                              # N = 9
                  "b": ("benign", "spike_mid", "zeros", "ray_spike_first", "ray_spike_mid")}      # N = 5, a saturated ray last


def sample_row(kind, nb, g):
    """(bins [nb], weights [nb-1]).  ``ray_*``: the weights[1:-1] the float32 compositing of that ray produces, on its z_mid."""
    if kind.startswith("ray_"):
        S = nb + 1
        raw, z, d = composite_ray(kind[4:], S, 2, g)
        w = render_train(raw[None], z[None], d[None], dtype=F32)[1][0]
        return (.5 * (z[1:] + z[:-1])).contiguous(), w[1:-1].contiguous()
    bins = _z_row(nb, g)
    w = torch.zeros(nb - 1)
    if kind == "spike_first":
        w[0] = 1.0
    elif kind == "spike_mid":
        w[(nb - 1) // 2] = 1.0
    elif kind == "spike_last":
        w[-1] = 1.0
    elif kind == "benign":
        w = torch.rand(nb - 1, generator=g)
    elif kind != "zeros":
        raise KeyError(kind)
    return bins, w


def sample_case(nb, batch):
    g = _gen(3, nb, ord(batch))
    rows = [sample_row(k, nb, g) for k in SAMPLE_BATCHES[batch]]
    return {"name": f"nb{nb}_{batch}", "kinds": SAMPLE_BATCHES[batch], "nb": nb,
            "bins": torch.stack([r[0] for r in rows]).contiguous(), "w": torch.stack([r[1] for r in rows]).contiguous()}


def sample_case_ids():
    return [(nb, b) for nb in SAMPLE_NB for b in SAMPLE_BATCHES]


def u_candidates(cdf, seed, n_random=29):
    """Per row of a float32 CDF [N, nb]: 0, 1, every knot, ``nextafter`` on both sides of every knot (kept inside [0, 1]) and
    random draws -> [N, 2 + 3 nb + n_random] float32."""
    N, nb = cdf.shape
    g = _gen(4, seed, nb)
    zero, one = torch.zeros(N, 1), torch.ones(N, 1)
    lo = torch.nextafter(cdf, torch.full_like(cdf, -1.0)).clamp(0.0, 1.0)
    hi = torch.nextafter(cdf, torch.full_like(cdf, 2.0)).clamp(0.0, 1.0)
    return torch.cat([zero, one, cdf.clamp(0.0, 1.0), lo, hi, torch.rand(N, n_random, generator=g)], -1).contiguous()


def u_chunks(cand, n):
    """The candidates in pieces of n draws [N, n]; the last piece is filled up from the front."""
    L = cand.shape[1]
    out = []
    for s in range(0, L, n):
        c = cand[:, s:s + n]
        if c.shape[1] < n:
            c = torch.cat([c, cand[:, :n - c.shape[1]]], -1) if L >= n else cand.repeat(1, math.ceil(n / L))[:, :n]
        out.append(c.contiguous())
    return out


def check_cdf(cdf, w, what, strict=True):
    """Stage (i): the float32 CDF under test against the float64 one.  Each entry is one float32 rounding of a double-accumulated
    sum of float32 quotients: <= 2 ulp at 1.0 (``strict``; ATen's float32 ``sum`` of 511 weights is not held to it)."""
    cdf = cdf.detach().cpu()
    err = float((cdf.double() - cdf_from_weights(w)).abs().max())
    print(f"{what}: cdf err {err:.3e}")
    assert bool(torch.isfinite(cdf).all()), what
    assert err <= (2.4e-7 if strict else 1e-6), (what, err)
    assert bool((cdf[:, 1:] >= cdf[:, :-1]).all()), (what, "cdf not monotone")
    assert bool((cdf[:, 0] == 0).all()), (what, "cdf[0] != 0")
    return err


def check_samples(samples, inds, bins, cdf, u, what):
    """Stage (ii), given the CDF under test: indices exact, every sample within 4 ulp of the row's max |bins| of the float64
    evaluation (four float32 roundings of at most half an ulp of that scale each, times two).  Returns the worst distance in ulp."""
    samples, cdf, u = samples.detach().cpu(), cdf.detach().cpu(), u.detach().cpu()
    want, want_inds = sample_tail(bins, cdf, u)
    assert bool(torch.isfinite(samples).all()), (what, "samples not finite")
    if inds is not None:
        assert torch.equal(inds.detach().cpu(), want_inds), (what, "inds", int((inds.detach().cpu() != want_inds).sum()))
    ulp = ulp32(bins.abs().max(-1, keepdim=True).values)
    dist = (samples.double() - want).abs() / ulp
    worst = float(dist.max())
    assert worst <= 4.0, (what, "samples", worst, (dist > 4).nonzero()[:8].tolist())
    return worst


# ------------------------------------------------------------------------------------------
# importance_resample and sort_rows cases
# ------------------------------------------------------------------------------------------
RESAMPLE_SHAPES = ((3, 5), (65, 63), (513, 128), (513, 511), (64, 960))       # (S, n_imp); S + n_imp = 1024 twice


def resample_case(S, n_imp):
    """N = 5: z_coarse with repeated values, weights zero / spiked / saturated-ray / benign, the saturated ray last."""
    g = _gen(5, S, n_imp)
    kinds = ("zeros_repeated", "benign_repeated", "spike_mid", "zeros", "ray_spike_mid")
    zs, ws = [], []
    for kind in kinds:
        if kind.startswith("ray_"):
            raw, z, d = composite_ray(kind[4:], S, 2, g)
            w = render_train(raw[None], z[None], d[None], dtype=F32)[1][0]
        else:
            z = _z_row(S, g)
            w = torch.zeros(S)
            if kind == "spike_mid":
                w[S // 2] = 1.0
            if kind.startswith("benign"):
                w = torch.rand(S, generator=g)
            if kind.endswith("repeated"):                                  # runs of equal depths: their midpoints ARE coarse depths
                for k in range(0, S - 1, 4):
                    z[k + 1] = z[k]
                if S >= 8:
                    z[5] = z[6] = z[4]
        zs.append(z)
        ws.append(w)
    return {"name": f"S{S}_n{n_imp}", "kinds": kinds, "S": S, "n_imp": n_imp, "z": torch.stack(zs).contiguous(), "w": torch.stack(ws).contiguous()}


def resample_u(case, cdf):
    """[N, n_imp] draws for a resample case from the CDF of its weights[1:-1]: knots first (so that all-zero weights put
    samples exactly on repeated coarse depths), then their neighbours, 0, 1 and random draws."""
    cand = u_candidates(cdf, case["S"] * 1000 + case["n_imp"])
    cand = torch.cat([cand[:, 2:], cand[:, :2]], -1)
    return u_chunks(cand, case["n_imp"])[0]


SORT_K = (1, 2, 64, 65, 2048)


def sort_case(K, N=7):
    g = _gen(6, K, N)
    inf = float("inf")
    rnd = torch.randn(K, generator=g)
    rows = [torch.full((K,), 1.5),                                                           # all equal
            torch.randint(0, 5, (K,), generator=g).float(),                                  # many duplicates
            torch.sort(rnd).values,                                                          # already sorted
            torch.sort(rnd, descending=True).values,                                         # reversed
            torch.tensor([0.0, -0.0, 1.0, -1.0])[torch.randint(0, 4, (K,), generator=g)],    # +-0.0
            torch.tensor([inf, -inf, 0.5, inf, -inf, -2.0])[torch.randint(0, 6, (K,), generator=g)],   # +-inf
            torch.randn(K, generator=g)]
    order = (6, 2, 3, 1, 4, 0, 5)[:N] if N < 7 else range(7)
    return torch.stack([rows[i] for i in order]).contiguous()
