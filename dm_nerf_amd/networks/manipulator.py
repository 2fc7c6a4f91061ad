"""Drop-in for the render core of the reference's ``networks/manipulator.py``: ``exchanger``,
``manipulator_render``, ``manipulator_nerf``, ``manipulator``.  The two drivers of that file call exactly these four functions;
their pose loops live elsewhere in this package: one pose is ``dm_nerf_amd.distributed.manipulate_frame`` (rows sharded over
the ranks), ``manipulator_eval`` (:208-364) is ``dm_nerf_amd.editing.manipulate_eval_path`` (frames, PSNR / SSIM / AP, the 8-bit
and coloured images) and ``manipulator_demo`` (:367-491) is ``dm_nerf_amd.editing.manipulate_demo_path`` (several objects per
view, rigid or deformed).  File output and the pose JSON stay with the caller (LPIPS: ``manipulate_eval_path(..., lpips=evaluator.LPIPSVGG...)``)."""
import ctypes
from types import SimpleNamespace

import torch

from .. import _lib
from . import helpers
from .render import run_network, run_network_skip


def exchanger(ori_raw, tar_raws, ori_raw_pred, tar_raw_preds, move_labels):
    """``exchanger`` (networks/manipulator.py:18-83).  ``ori_raw`` is modified in place, as in the reference."""
    _lib.require_gpu(ori_raw, ori_raw_pred, *tar_raws, *tar_raw_preds)
    N, S, ch = ori_raw.shape
    C = ch - 4
    T = len(move_labels)
    tr = [_lib.f32(t) for t in tar_raws]
    ta = [_lib.f32(t) for t in tar_raw_preds]
    oa = _lib.f32(ori_raw_pred)
    P = ctypes.c_void_p * T
    raws, accs = P(*[t.data_ptr() for t in tr]), P(*[t.data_ptr() for t in ta])
    labels = (ctypes.c_int * T)(*[int(v) for v in move_labels])
    ori_label = torch.empty(N, S, dtype=torch.int64, device=ori_raw.device)
    tar_label = torch.empty(N, S, dtype=torch.int64, device=ori_raw.device)
    _lib.launch("dmnerf_exchanger", ori_raw, raws, oa, accs, labels, T, N, S, C, ori_label, tar_label)
    return ori_raw, tar_raws, ori_label, tar_label


MOVE, COPY, REMOVE = 0, 1, 2                    # the kinds of ``dmnerf_edit_exchange``


def keep_words(keep_labels, C):
    """The keep set as the two 64-bit words ``dmnerf_edit_exchange`` takes (bit ``l`` set: label ``l`` stays)."""
    words = [0, 0]
    for l in keep_labels:
        l = int(l)
        if not 0 <= l < C:
            raise ValueError(f"keep_labels: label {l} outside [0, {C})")
        words[l >> 6] |= 1 << (l & 63)
    return words


def edit_exchanger(ori_raw, tar_raws, ori_raw_pred, tar_raw_preds, move_labels, kinds, keep_labels=None, want_label=True):
    """``exchanger`` (networks/manipulator.py:18-83) generalised (``dmnerf_edit_exchange``): edit ``e`` of label
    ``move_labels[e]`` is a ``MOVE`` (the reference's loop body), a ``COPY`` (the target's rows where the target is the object and
    the original is not; nothing is given up) or a ``REMOVE`` (the original's rows of the object times 0; ``tar_raws[e]`` and
    ``tar_raw_preds[e]`` are ``None``).  ``keep_labels``: afterwards every row whose OWN label is not in the set is zeroed.
    ``ori_raw`` is modified in place -> ``(ori_raw, ori_label [N,S] int64 or None)``."""
    E = len(move_labels)
    if len(kinds) != E or len(tar_raws) != E or len(tar_raw_preds) != E:
        raise ValueError(f"edit_exchanger: {E} labels, {len(kinds)} kinds, {len(tar_raws)} / {len(tar_raw_preds)} targets")
    _lib.require_gpu(ori_raw, ori_raw_pred, *tar_raws, *tar_raw_preds)
    if ori_raw.dtype != torch.float32:
        raise ValueError("edit_exchanger: ori_raw is edited in place and must be float32")
    N, S, ch = ori_raw.shape
    C = ch - 4
    tr = [None if t is None else _lib.f32(t) for t in tar_raws]
    ta = [None if t is None else _lib.f32(t) for t in tar_raw_preds]
    oa = _lib.f32(ori_raw_pred)
    P = ctypes.c_void_p * max(E, 1)
    raws = P(*[None if t is None else t.data_ptr() for t in tr])
    accs = P(*[None if t is None else t.data_ptr() for t in ta])
    labels = (ctypes.c_int * max(E, 1))(*[int(v) for v in move_labels])
    kind = (ctypes.c_int * max(E, 1))(*[int(v) for v in kinds])
    keep = None if keep_labels is None else (ctypes.c_uint64 * 2)(*keep_words(keep_labels, C))
    ori_label = torch.empty(N, S, dtype=torch.int64, device=ori_raw.device) if want_label else None
    _lib.launch("dmnerf_edit_exchange", ori_raw, raws, oa, accs, labels, kind, E, keep, N, S, C, ori_label)
    return ori_raw, ori_label


def manipulator_render(raw, z_vals, rays_d):
    """``manipulator_render`` (networks/manipulator.py:86-105) -> (rgb_map, weights, depth_map, ins_map [N,C])."""
    raw, z, d = _lib.f32(raw), _lib.f32(z_vals), _lib.f32(rays_d)
    _lib.require_gpu(raw, z, d)
    N, S, ch = raw.shape
    C = ch - 4
    f = dict(dtype=torch.float32, device=raw.device)
    rgb, w, depth, ins = torch.empty(N, 3, **f), torch.empty(N, S, **f), torch.empty(N, **f), torch.empty(N, C, **f)
    _lib.launch("dmnerf_manipulator_render", raw, z, d, N, S, C, rgb, w, depth, ins)
    return rgb, w, depth, ins


def manipulator_z(N_rays, near, far, N_samples, device=None):
    """The depth grid of ``manipulator_nerf`` (:117-119): ``near (1 - t) + far t``."""
    dev = helpers._device(device)
    t = helpers.linspace01(N_samples, dev)
    z = torch.empty(int(N_rays), int(N_samples), dtype=torch.float32, device=dev)
    _lib.launch("dmnerf_z_val_lerp", t, float(near), float(far), int(N_rays), int(N_samples), z)
    return z


def manipulator_nerf(rays, position_embedder, view_embedder, model, N_samples=None, near=None, far=None, z_vals=None, split=None,
                     skip=None, counts=None):
    """``manipulator_nerf`` (networks/manipulator.py:108-134) -> (raw [N,S,4+C], z_vals).  ``split`` (extension): the opt-in
    split-operand network kernels, ``weights.split_mode(args)``.  ``skip`` (extension): a ``field.SkipGrid``; the network is then
    evaluated at the samples in set cells only and every other row of ``raw`` is the empty row (``render.run_network_skip``, which
    also explains ``counts``)."""
    rays_o, rays_d = rays
    if z_vals is None:
        z_vals = manipulator_z(rays_d.shape[0], near, far, N_samples, rays_d.device)
    with torch.no_grad():
        if skip is not None:
            raw = run_network_skip(model, rays_o, rays_d, z_vals, skip, split=split, counts=counts)
        else:
            raw = run_network(model, rays_o, rays_d, z_vals, split=split)
    return raw, z_vals


def _skip_plan(model_coarse, model_fine, args, skip, skip_levels, skip_counts):
    """-> the ``manipulator_nerf`` keywords of the coarse and of the fine model's calls: ``args.mfma_split``, the counts and, at the
    levels ``skip=`` names, the grid.  Everything ``skip=`` cannot serve is refused here, before the first launch."""
    from .. import weights
    split = weights.split_mode(args)
    kc = kf = {}
    if skip is not None:
        from .. import field
        from . import render
        if not isinstance(skip, field.SkipGrid):
            raise TypeError("manipulator: skip must be a field.SkipGrid")
        levels = render.check_skip_levels("manipulator", skip_levels)
        if split not in (None, "f16x2"):
            raise ValueError(f"manipulator: skip= has no sparse network kernel for args.mfma_split = {split!r} (f32 and 'f16x2' only)")
        for name, model in (("coarse", model_coarse), ("fine", model_fine)):
            if name in levels and not model._fused_ok():
                raise ValueError(f"manipulator: skip= needs the 8 x 256 network at the {name} level (the sparse kernels exist for it only)")
        kc, kf = ({"skip": skip} if name in levels else {} for name in ("coarse", "fine"))
    return dict(kc, split=split, counts=skip_counts), dict(kf, split=split, counts=skip_counts)


def sort_rows(x):
    """``torch.sort(x, -1).values`` (exact permutation)."""
    x = _lib.f32(x)
    _lib.require_gpu(x)
    out = torch.empty_like(x)
    _lib.launch("dmnerf_sort_rows", x, x.shape[0], x.shape[1], out)
    return out


def _first_pass(model_coarse, model_fine, ori_rays, f_tar_rays, args, us, kc, kf):
    """Step 1 of ``manipulator``, with or without edit kinds: the original rays, then every target ray set, through coarse ->
    resample -> fine -> accumulate.  One draw each, in that order (``us`` when given); ``draw`` makes the later ones."""
    N_samples, N_importance, near, far = args.N_samples, args.N_importance, args.near, args.far
    dev = ori_rays.device
    Nr = ori_rays.shape[1]
    us = list(us) if us is not None else None
    draw = lambda: _lib.f32(us.pop(0)) if us is not None else torch.rand([Nr, N_importance], device=dev)
    p = SimpleNamespace(draw=draw, tar_raws=[], f_tar_z=[], f_tar_zs=[], tar_ins_accums=[], tar_rgb=None, tar_ins_accum=None)
    p.ori_raw, p.ori_z = manipulator_nerf(ori_rays, None, None, model_coarse, N_samples, near, far, **kc)
    _, ori_w, _, _ = manipulator_render(p.ori_raw, p.ori_z, ori_rays[1])
    ori_z_full = helpers.importance_resample(p.ori_z, ori_w, N_importance, u=draw())
    ori_raw_full, _ = manipulator_nerf(ori_rays, None, None, model_fine, z_vals=ori_z_full, **kf)
    _, _, _, p.ori_ins_accum = manipulator_render(ori_raw_full, ori_z_full, ori_rays[1])
    for tar_rays in f_tar_rays:
        tar_raw, tar_z = manipulator_nerf(tar_rays, None, None, model_coarse, N_samples, near, far, **kc)
        p.tar_raws.append(tar_raw); p.f_tar_z.append(tar_z)
        p.tar_rgb, tar_w, _, _ = manipulator_render(tar_raw, tar_z, tar_rays[1])
        tar_z_full, tar_zs = helpers.importance_resample(tar_z, tar_w, N_importance, u=draw(), return_samples=True)
        tar_raw_full, _ = manipulator_nerf(tar_rays, None, None, model_fine, z_vals=tar_z_full, **kf)
        _, _, _, p.tar_ins_accum = manipulator_render(tar_raw_full, tar_z_full, tar_rays[1])
        p.f_tar_zs.append(tar_zs); p.tar_ins_accums.append(p.tar_ins_accum)
    return p


def _manipulator_edit(model_coarse, model_fine, ori_rays, f_tar_rays, args, us, kinds, keep_labels, kc, kf):
    """``manipulator`` with edit kinds: the chain below with ``edit_exchanger`` in place of ``exchanger``, the target side run for
    the ``T_r`` entries that have rays (MOVE and COPY) only, and the original's fine network on the merged depths evaluated once."""
    labels = [int(v) for v in args.target_labels]
    kinds = [MOVE] * len(labels) if kinds is None else [int(k) for k in kinds]
    if len(kinds) != len(labels):
        raise ValueError(f"manipulator: {len(kinds)} kinds for {len(labels)} target labels")
    if any(k not in (MOVE, COPY, REMOVE) for k in kinds):
        raise ValueError(f"manipulator: kinds must be MOVE (0), COPY (1) or REMOVE (2), got {kinds}")
    has_rays = [k != REMOVE for k in kinds]
    if len(f_tar_rays) != sum(has_rays):
        raise ValueError(f"manipulator: {len(f_tar_rays)} target ray sets for {sum(has_rays)} MOVE / COPY entries")
    if not labels and keep_labels is None:
        raise ValueError("manipulator: no edit and no keep_labels")
    p = _first_pass(model_coarse, model_fine, ori_rays, f_tar_rays, args, us, kc, kf)
    ori_z, tar_raws, f_tar_zs, N_importance = p.ori_z, p.tar_raws, p.f_tar_zs, args.N_importance

    def per_edit(with_rays):                    # one slot per edit: the next ray entry's tensor, None for a REMOVE
        it = iter(with_rays)
        return [next(it) if h else None for h in has_rays]
    accs = per_edit(p.tar_ins_accums)
    ori_raw, _ = edit_exchanger(p.ori_raw, per_edit(tar_raws), p.ori_ins_accum, accs, labels, kinds, keep_labels, want_label=False)
    _, ori_w, _, _ = manipulator_render(ori_raw, ori_z, ori_rays[1])
    _, ori_zs = helpers.importance_resample(ori_z, ori_w, N_importance, u=p.draw(), return_samples=True)
    ori_z = sort_rows(torch.cat([ori_z, ori_zs] + f_tar_zs, dim=-1))
    ori_raw, _ = manipulator_nerf(ori_rays, None, None, model_fine, z_vals=ori_z, **kf)
    for idx, tar_rays in enumerate(f_tar_rays):
        tar_z = sort_rows(torch.cat([p.f_tar_z[idx], ori_zs] + f_tar_zs, dim=-1))
        tar_raws[idx], _ = manipulator_nerf(tar_rays, None, None, model_fine, z_vals=tar_z, **kf)
    ori_raw, _ = edit_exchanger(ori_raw, per_edit(tar_raws), p.ori_ins_accum, accs, labels, kinds, keep_labels, want_label=False)
    final_rgb, _, _, final_ins = manipulator_render(ori_raw, ori_z, ori_rays[1])
    if not f_tar_rays:
        return final_rgb, final_ins, torch.zeros_like(final_rgb), torch.zeros_like(final_ins)
    return final_rgb, final_ins, p.tar_rgb, p.tar_ins_accum


def manipulator(position_embedder, view_embedder, model_coarse, model_fine, ori_rays, f_tar_rays, args, us=None, kinds=None,
                keep_labels=None, skip=None, skip_levels=("coarse", "fine"), skip_counts=None):
    """``manipulator`` (networks/manipulator.py:137-205) -> (final_rgb, final_ins, tar_rgb, tar_ins_accum).

    ``kinds`` / ``keep_labels`` (extension; both ``None``: the reference's chain below, unchanged): ``kinds[e]`` in ``MOVE``,
    ``COPY``, ``REMOVE`` for ``args.target_labels[e]``; ``f_tar_rays`` then holds rays only for the ``T_r`` MOVE and COPY entries, in
    order, the draws are ``2 + T_r`` (original, each target, original again) and the merged depth row has ``64 + 128 + 128 T_r``
    samples: a removal alone costs one coarse and two fine launches of the original rays.  ``keep_labels``: only samples whose own
    label is in the set survive (``edit_exchanger``).  With ``T_r == 0`` ``tar_rgb`` and ``tar_ins_accum`` are zeros.

    RNG: the reference calls ``sample_pdf(..., det=False)`` even at evaluation (:148,:170,:187): ``2 + T`` draws
    of ``torch.rand([N, N_importance])`` in the order original, each target, original again; the same draws are
    made here on the rays' device, or pass them as ``us`` (extension used by the tests).  ``args.mfma_split`` (extension, default
    off) evaluates the 2 + 4 T network launches on the opt-in split-operand kernels, as in ``dm_nerf``.

    ``skip`` (extension, default off: the chain is then untouched): a ``field.SkipGrid`` in the world frame of the trained scene.
    Target rays are the original rays carried back into that frame, so one grid serves both ray sets.  Every network call on
    ``model_coarse`` / ``model_fine`` named in ``skip_levels`` ("coarse", "fine") evaluates only the samples whose cell is set (or
    that lie outside the box with ``grid.outside == "evaluate"``); every other row of its output is the EMPTY ROW
    ``(0, 0, 0, 0 | 0, .., 0, 1)``: sigma 0, so its compositing weight is exactly 0, and per-sample label ``C - 1`` -- never a move
    label -- so the exchanger does not take a skipped sample for the moved object, as it would an all-zero row (label 0).  The result
    is the dense chain with exactly those rows of every network output replaced, bit for bit; with ``SkipGrid.full`` it is the dense
    result.  Draws, their order, shapes, ``kinds`` and ``keep_labels`` are unchanged.  ``args.mfma_split = "bf16x3"`` and a network
    shape other than 8 x 256 at a named level raise ``ValueError`` (no dense detour).  ``skip_counts``: optional int64 ``[2]`` device
    tensor, += (samples evaluated, samples) over the calls that went through the grid.
    """
    kc, kf = _skip_plan(model_coarse, model_fine, args, skip, skip_levels, skip_counts)
    if kinds is not None or keep_labels is not None:
        return _manipulator_edit(model_coarse, model_fine, ori_rays, list(f_tar_rays), args, us, kinds, keep_labels, kc, kf)
    p = _first_pass(model_coarse, model_fine, ori_rays, f_tar_rays, args, us, kc, kf)
    ori_z, tar_raws, N_importance = p.ori_z, p.tar_raws, args.N_importance
    ori_raw, _, _, _ = exchanger(p.ori_raw, tar_raws, p.ori_ins_accum, p.tar_ins_accums, args.target_labels)
    # step 2: re-render the edited coarse field, resample, and evaluate the fine model on the merged depths
    _, ori_w, _, _ = manipulator_render(ori_raw, ori_z, ori_rays[1])
    _, ori_zs = helpers.importance_resample(ori_z, ori_w, N_importance, u=p.draw(), return_samples=True)
    f_tar_zs = torch.cat(p.f_tar_zs, dim=-1)
    ori_z = sort_rows(torch.cat([ori_z, ori_zs, f_tar_zs], dim=-1))
    for idx, tar_rays in enumerate(f_tar_rays):
        ori_raw, ori_z = manipulator_nerf(ori_rays, None, None, model_fine, z_vals=ori_z, **kf)
        tar_z = sort_rows(torch.cat([p.f_tar_z[idx], ori_zs, f_tar_zs], dim=-1))
        tar_raws[idx], _ = manipulator_nerf(tar_rays, None, None, model_fine, z_vals=tar_z, **kf)
    ori_raw, _, _, _ = exchanger(ori_raw, tar_raws, p.ori_ins_accum, p.tar_ins_accums, args.target_labels)
    final_rgb, _, _, final_ins = manipulator_render(ori_raw, ori_z, ori_rays[1])
    return final_rgb, final_ins, p.tar_rgb, p.tar_ins_accum


def edited_field(model_coarse, model_fine, rays, args, edit, u=None, counts=None):
    """One chunk of the FIELD-EDIT render (extension; DESIGN.md 8a, "The field-edit route") -> ``(rgb [N,3], ins [N,C], depth [N])``:
    the trained field seen through the edited volume of ``edit`` (an ``editing.FieldEdit``), one network evaluation per sample.

    ``manipulator_z`` -> ``render.run_network_edited`` on ``model_coarse`` -> ``manipulator_render`` -> ``helpers.importance_resample``
    with the ONE draw ``u [N, N_importance]`` (drawn here with ``torch.rand`` if not given) -> ``run_network_edited`` on ``model_fine``
    over the merged depths -> ``manipulator_render``.  Two sparse network launches, whatever the number of edits.  Both compositing
    calls use the ORIGINAL ray's ``z`` and ``|d|``, as the exchanger route does: a carried-back ray only says where the network is asked.

    A render with its own contract, not ``manipulator()`` bit for bit: ownership is decided per cell by ``edit_volume`` (nearest cell, the
    cell centre's label) and the exchanger's accumulated-label conditions are not applied.  ``args.mfma_split``: None or ``"f16x2"``
    (``"bf16x3"`` and another network shape than 8 x 256 raise).  ``counts``: ``run_network_edited``'s.  Nothing reaches the host."""
    from .. import weights
    from .render import run_network_edited
    split = weights.split_mode(args)
    rays_o, rays_d = rays
    dev = rays_d.device
    N = rays_d.shape[0]
    n_imp = int(args.N_importance)
    u = torch.rand([N, n_imp], device=dev) if u is None else _lib.f32(u)
    with torch.no_grad():
        z = manipulator_z(N, args.near, args.far, args.N_samples, dev)
        raw = run_network_edited(model_coarse, rays_o, rays_d, z, edit, split=split, counts=counts)
        _, w, _, _ = manipulator_render(raw, z, rays_d)
        z_full = helpers.importance_resample(z, w, n_imp, u=u)
        raw = run_network_edited(model_fine, rays_o, rays_d, z_full, edit, split=split, counts=counts)
        rgb, _, depth, ins = manipulator_render(raw, z_full, rays_d)
    return rgb, ins, depth
