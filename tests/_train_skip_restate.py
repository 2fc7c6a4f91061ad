"""numpy / torch-CPU restatement of the training step that skips empty space (``autograd.run_network_train_skip``,
csrc/train_skip.hip): the selection (``_skip_restate``'s cell arithmetic), the padded length, gather and scatter as index
expressions, and the gradients of ``sum(raw * G * flag)`` in float64 through the oracle model.  Also the hand-written scenes the
GPU tests run on.  Nothing here shares code with the product."""
import numpy as np
import torch

import _skip_restate as SR

F = np.float32


def padded_length(n_sel, bucket):
    """``n_sel`` rounded up to a multiple of ``bucket`` (0 stays 0)."""
    return -(-int(n_sel) // int(bucket)) * int(bucket)


def gather_samples(rays_o, rays_d, z, sel, n_pad):
    """-> ``o' [n_pad, 3], d' [n_pad, 3], z' [n_pad]``: row i < len(sel) is sample ``sel[i]``'s ray and depth; the padding repeats
    the last selected sample."""
    o, d, z = np.asarray(rays_o, dtype=F), np.asarray(rays_d, dtype=F), np.asarray(z, dtype=F)
    S = z.shape[1]
    sel = np.asarray(sel, dtype=np.int64)
    assert len(sel) <= n_pad and (len(sel) > 0 or n_pad == 0)
    idx = np.concatenate([sel, np.full(n_pad - len(sel), sel[-1] if len(sel) else 0, dtype=np.int64)])
    return o[idx // S], d[idx // S], z.reshape(-1)[idx]


def rows_scatter(dst, src, sel):
    """``dst[sel[i]] = src[i]`` for ``i < len(sel)``; every other row of ``dst`` is kept.  -> a copy."""
    out = np.array(dst, copy=True)
    sel = np.asarray(sel, dtype=np.int64)
    out[sel] = np.asarray(src)[:len(sel)]
    return out


def rows_gather(src, sel, n_pad):
    """``out[i] = src[sel[i]]`` for ``i < len(sel)``, exact zeros for the padded rows."""
    src = np.asarray(src)
    sel = np.asarray(sel, dtype=np.int64)
    out = np.zeros((n_pad,) + src.shape[1:], dtype=src.dtype)
    out[:len(sel)] = src[sel]
    return out


def masked_oracle_grads(sd, rays_o, rays_d, z, cot, flag):
    """float64 referee: ``raw`` of the oracle model on every sample and the parameter gradients of ``sum(raw * cot * flag)``
    (tests/test_gpu_train.py::_oracle_mlp_grads with the mask in the loss) -> ``(raw [N,S,4+C] f64, {name: grad f64})``."""
    from oracle import ref_cpu as O
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    rays_o, rays_d, z = rays_o.double(), rays_d.double(), z.double()
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
    vd = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    x = torch.cat([O.embed(pts.reshape(-1, 3), 10), O.embed(vd[:, None].expand(pts.shape).reshape(-1, 3), 4)], -1)
    raw = O.mlp_forward(sdg, x).reshape(z.shape[0], z.shape[1], -1)
    mask = torch.as_tensor(np.asarray(flag), dtype=torch.float64).reshape(z.shape[0], z.shape[1], 1)
    (raw * cot.double() * mask).sum().backward()
    return raw.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sdg.items()}


# ---- the hand-written scene: 37 rays along +x through the box [-1, 1)^3 with an 8^3 grid ------------------------------------
LO, HI, DIMS = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (8, 8, 8)
N_RAYS = 37


def hand_grid():
    """occ [8,8,8] bool, written by hand: a block in the middle, one slab on the x = lo face, one far corner cell."""
    occ = np.zeros(DIMS, dtype=bool)
    occ[1:7, 0:7, 1:7] = True               # the block: x in [-0.75, 0.75), y in [-1, 0.75), z in [-0.75, 0.75)
    occ[0, :, 4] = True                     # a slab on the entry face: x in [-1, -0.75), z in [0, 0.25)
    occ[7, 7, 7] = True
    return occ


def hand_rays(S):
    """37 rays from x = -2 along +x (slightly tilted) on a 7 x 5 lattice of (y, z) whose y = -1.15 column misses the box, two more
    through the middle; depths: every fourth ray samples x in [-0.4, 0.4] only (inside the block when its lattice point is), the others
    x in [-1.25, 1.25] (first and last samples outside the box).  -> rays_o [37,3], rays_d [37,3], z [37,S] float32."""
    o, d, z = np.zeros((N_RAYS, 3), F), np.zeros((N_RAYS, 3), F), np.zeros((N_RAYS, S), F)
    for i in range(N_RAYS):
        if i < 35:
            y, zc = -1.15 + 2.1 * (i % 7) / 6.0, -0.95 + 1.8 * (i // 7) / 4.0
        else:
            y, zc = (0.1, -0.2) if i == 35 else (-0.3, 0.3)
        o[i] = (-2.0, y, zc)
        d[i] = (1.0, 0.02 * ((i % 3) - 1), 0.015 * ((i % 5) - 2))
        near, far = (1.6, 2.4) if i % 4 == 0 else (0.75, 3.25)
        z[i] = np.linspace(near, far, S, dtype=np.float64).astype(F)
    return o, d, z


def hand_scene(S, outside):
    """The scene and its selection -> dict(o, d, z, words, flag [37,S], sel, count); asserts that the selection is not degenerate."""
    o, d, z = hand_rays(S)
    words = SR.pack_bits(hand_grid())
    flag, sel, count = SR.select(o, d, z, words, LO, HI, DIMS, outside=outside)
    in_set, _, _ = SR.select(o, d, z, words, LO, HI, DIMS, outside="empty")       # samples in a SET cell
    full = SR.pack_bits(np.ones(DIMS, dtype=bool))
    in_box, _, _ = SR.select(o, d, z, full, LO, HI, DIMS, outside="empty")
    inside_any = in_set.any(1)
    assert (~inside_any).any(), "some rays must have no set cell"
    assert in_set.all(1).any(), "some rays must have every sample in a set cell"
    assert (~in_box.all(1)).any() and (~in_box.any(1)).any(), "some rays must leave the box, some must miss it"
    assert count % 32 != 0, count
    assert 0.2 <= count / flag.size <= 0.8, count / flag.size
    return dict(o=o, d=d, z=z, words=words, flag=flag, sel=sel, count=count)


def exact_scene(K, S=5):
    """37 rays through the middle of the block whose depths are chosen per sample so that EXACTLY ``K`` samples are selected with
    ``outside="empty"``: a chosen sample sits at x in [-0.4, 0.4] (a set cell), the others at x < -1.5 (outside the box)."""
    o, d, z = np.zeros((N_RAYS, 3), F), np.zeros((N_RAYS, 3), F), np.zeros((N_RAYS, S), F)
    order = np.random.RandomState(11).permutation(N_RAYS * S)
    chosen = np.zeros(N_RAYS * S, dtype=bool)
    chosen[order[:K]] = True
    chosen = chosen.reshape(N_RAYS, S)
    for i in range(N_RAYS):
        o[i] = (-2.0, -0.4 + 0.8 * (i % 6) / 5.0, -0.6 + 1.2 * (i // 6) / 6.0)
        d[i] = (1.0, 0.0, 0.0)
        for s in range(S):
            z[i, s] = (1.6 + 0.8 * s / (S - 1)) if chosen[i, s] else (0.1 + 0.05 * s)
    words = SR.pack_bits(hand_grid())
    flag, sel, count = SR.select(o, d, z, words, LO, HI, DIMS, outside="empty")
    assert count == K and np.array_equal(flag != 0, chosen), (count, K)
    return dict(o=o, d=d, z=z, words=words, flag=flag, sel=sel, count=count)
