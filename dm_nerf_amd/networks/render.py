"""Drop-in for the reference's ``networks/render.py``: render_train, dm_nerf."""
from types import SimpleNamespace

import torch

from .. import _lib, weights
from . import helpers


def render_train(raw, z_vals, rays_d):
    """``render_train`` (networks/render.py:6-28) -> (rgb_map, weights, depth_map, ins_map)."""
    if torch.is_grad_enabled() and raw.requires_grad:
        from .. import autograd
        return autograd.render_train_train(raw, z_vals, rays_d)
    raw, z, d = _lib.f32(raw), _lib.f32(z_vals), _lib.f32(rays_d)
    _lib.require_gpu(raw, z, d)
    N, S, ch = raw.shape
    C = ch - 4
    dev = raw.device
    rgb = torch.empty(N, 3, dtype=torch.float32, device=dev)
    w = torch.empty(N, S, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    ins = torch.empty(N, C - 1, dtype=torch.float32, device=dev)
    _lib.launch("dmnerf_composite_fwd", raw, z, d, N, S, C, rgb, w, depth, ins)
    return rgb, w, depth, ins


def run_network(model, rays_o, rays_d, z_vals, split=None):
    """pts = o + d z -> embed(pts) | embed(d/|d|) -> ``model`` (networks/render.py:49-61 / :71-83)
    as one fused kernel: ``[N,3], [N,3], [N,S] -> raw [N,S,4+C]`` (inference only).  ``split``: None (the f32 kernels) or
    ``weights.split_mode(args)`` = "bf16x3" / "f16x2", the opt-in split-operand kernels (f32-class, not bitwise)."""
    if not model._fused_ok():                              # another network shape: layer by layer (dm_nerf_amd/generic.py)
        if split:
            raise ValueError("args.mfma_split: the split-operand kernels exist for the 8 x 256 network only")
        from .. import generic
        return generic.run_network(model, rays_o, rays_d, z_vals, train=False)
    rays_o, rays_d, z = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3)), _lib.f32(z_vals)
    _lib.require_gpu(rays_o, rays_d, z)
    N, S = z.shape
    raw = torch.empty(N, S, 4 + model.ins_num + 1, dtype=torch.float32, device=z.device)
    v = weights.VARIANTS[split or None]
    _lib.launch(v.fwd, getattr(model, v.blob)(), model.ins_num, rays_o, rays_d, z, N, S, raw)
    return raw


_fill_rows = {}


def fill_row(width, device, last=0.0):
    """The row ``(0, .., 0, last)`` that ``dmnerf_skip_select_fill`` writes where nothing is evaluated: ``empty_row`` for the renders,
    all zeros for training.  Built on the device (no host copy) and kept per width, device and ``last``; as with the weight blobs, make
    one call outside a graph capture first, so that the kept tensor does not come from the capture's memory pool."""
    key = (int(width), str(device), float(last))
    if key not in _fill_rows:
        row = torch.zeros(int(width), dtype=torch.float32, device=device)
        if last:
            row[-1:].fill_(last)
        _fill_rows[key] = row
    return _fill_rows[key]


def empty_row(C, device):
    """The EMPTY ROW ``E = (0, 0, 0, 0 | 0, .., 0, 1)`` of width ``4 + C`` on ``device``: sigma, rgb and the object logits 0, the last
    ("empty") logit 1.  Its weight in ``manipulator_render`` is exactly 0 and the argmax over its C logits is ``C - 1``.
    Kept per width and device: ``fill_row``, whose warning about graph capture holds here."""
    return fill_row(4 + int(C), device, last=1.0)


def check_skip_levels(who, levels):
    """``levels`` as a tuple of ``SKIP_LEVELS`` names, validated as ``dm_nerf_fine_skip`` validates it."""
    levels = (levels,) if isinstance(levels, str) else tuple(levels)
    if not levels or any(l not in SKIP_LEVELS for l in levels):
        raise ValueError(f"{who}: levels must name 'coarse' and / or 'fine', got {levels}")
    return levels


def _require_grid(who, grid):
    from .. import field
    if not isinstance(grid, field.SkipGrid):
        raise TypeError(f"{who}: grid must be a field.SkipGrid")


SPARSE_WORDS = ("no sparse network kernel", "the sparse network kernels exist", "render in smaller chunks")


def check_skip_network(who, words, model, grid, split):
    """The refusals of a sparse network call that need no tensor, for the entry ``who`` in its own ``words`` (what it has none of,
    what exists for one network only, the advice: ``SPARSE_WORDS``) -> ``split`` or None."""
    _require_grid(who, grid)
    split = split or None
    if split not in (None, "f16x2"):
        raise ValueError(f"{who}: {words[0]} for args.mfma_split = {split!r} (f32 and 'f16x2' only)")
    if not model._fused_ok():
        raise ValueError(f"{who}: {words[1]} for the 8 x 256 network only")
    return split


def select_buffers(n, dev, n_min=0):
    """``sel`` int32, ``flag`` uint8 (``max(n, n_min)`` entries each) and the scan workspace of a selection among ``n`` samples."""
    sel = torch.empty(max(n, n_min), dtype=torch.int32, device=dev)
    flag = torch.empty(max(n, n_min), dtype=torch.uint8, device=dev)
    work = torch.empty(int(_lib.load().dmnerf_skip_select_work_ints(n)), dtype=torch.int32, device=dev)
    return sel, flag, work


def skip_select(who, words, grid, rays_o, rays_d, z_vals, width, last, counts):
    """The selection of one sparse network call (after ``check_skip_network``; an entry's own checks answer between the two): the
    size, device and ``counts`` checks in ``who``'s name, ``raw [N,S,width]``, the buffers, and ONE ``dmnerf_skip_select_fill`` (the
    ascending selection, its device-side length, ``fill_row(width, dev, last)`` into the clear rows) -> ``(rays_o, rays_d, z, raw,
    sel, count)``, the rays as the f32 tensors the launch read.  No sample: no launch, and ``sel`` and ``count`` are None."""
    N, S = z_vals.shape
    if N * S >= 2 ** 31:
        raise ValueError(f"{who}: {N * S} samples do not fit the int32 selection; {words[2]}")
    rays_o, rays_d, z = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3)), _lib.f32(z_vals)
    _lib.require_gpu(rays_o, rays_d, z)
    dev = z.device
    if grid.bits.device != dev:
        raise RuntimeError(f"{who}: the grid lives on another device than the rays")
    if counts is not None:
        _lib.require_gpu(counts)
        if counts.dtype != torch.int64 or tuple(counts.shape) != (2,) or counts.device != dev or not counts.is_contiguous():
            raise ValueError(f"{who}: counts must be a contiguous int64 [2] tensor on the rays' device")
    raw = torch.empty(N, S, width, dtype=torch.float32, device=dev)
    if N * S == 0:
        return rays_o, rays_d, z, raw, None, None
    sel, flag, work = select_buffers(N * S, dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    g = grid.c_struct()
    _lib.launch("dmnerf_skip_select_fill", g, rays_o, rays_d, z, N, S, flag, sel, count, work, raw, fill_row(width, dev, last), width, counts)
    return rays_o, rays_d, z, raw, sel, count


def run_network_skip(model, rays_o, rays_d, z_vals, grid, split=None, counts=None):
    """``run_network`` that does not evaluate empty space: ``raw [N,S,4+C]`` whose rows are the dense call's, bit for bit, where the
    sample's cell of ``grid`` (a ``field.SkipGrid``) is set -- or the sample lies outside its box and ``grid.outside == "evaluate"`` --
    and the empty row ``E = (0, 0, 0, 0 | 0, .., 0, 1)`` everywhere else (``empty_row``).  One ``dmnerf_skip_select_fill`` (flags, the
    ascending selection, its device-side length, and E into the clear rows: there is no separate fill of the buffer), then
    ``dmnerf_mlp_fwd_rays_sel`` (``split`` None) or ``dmnerf_mlp_fwd_rays_f16_sel`` (``"f16x2"``) over the selection.

    There is no dense detour: ``split == "bf16x3"`` (no sparse kernel) and a network shape other than the 8 x 256 one raise
    ``ValueError``, a grid on another device raises ``RuntimeError``, ``N S >= 2^31`` raises ``ValueError``.  ``counts``: optional
    int64 ``[2]`` device tensor; the number of samples evaluated and the number of samples are ADDED to it on the device (nothing
    reaches the host, so the call can be captured after one warm-up call: ``empty_row``).  Calls that share one ``counts`` must be on
    one stream (the sums are a plain read-modify-write on the device)."""
    who = "run_network_skip"
    split = check_skip_network(who, SPARSE_WORDS, model, grid, split)
    rays_o, rays_d, z, raw, sel, count = skip_select(who, SPARSE_WORDS, grid, rays_o, rays_d, z_vals, 4 + model.ins_num + 1, 1.0, counts)
    if sel is None:
        return raw
    N, S = z.shape
    if split == "f16x2":
        _lib.launch("dmnerf_mlp_fwd_rays_f16_sel", model.blob_f16(), model.ins_num, rays_o, rays_d, z, N, S, sel, count, raw)
    else:
        _lib.launch("dmnerf_mlp_fwd_rays_sel", model.blob(), model.ins_num, 0, rays_o, rays_d, z, N, S, sel, count, raw)
    return raw


EDITED_WORDS = ("no sparse network kernel", "the sparse network kernels exist", "render in smaller chunks")


def run_network_edited(model, rays_o, rays_d, z_vals, edit, split=None, counts=None, _stages=None):
    """The trained field seen through an edited volume: ``raw [N,S,4+C]`` with ONE network evaluation per sample, wherever ``edit`` (an
    ``editing.FieldEdit``) says the sample's content comes from.

    ``dmnerf_field_edit_select``: the owner of every sample's cell of ``edit.source`` -- 0: its own point, ``1 + e``: the point carried
    back by entry ``e``'s matrix, 255: nobody, the row becomes the empty row ``E = (0, 0, 0, 0 | 0, .., 0, 1)`` -- with the ray of every
    evaluated sample and the ascending selection; then ``dmnerf_mlp_fwd_rays_sel`` (``split`` None) or ``dmnerf_mlp_fwd_rays_f16_sel``
    (``"f16x2"``) over the selection as ``N S`` one-sample rays; then ``dmnerf_field_edit_filter``: a row whose own label (first maximum
    of its C logits) is not in its owner's accept set becomes the empty row too -- the exchanger's per-sample rule.  The rows keep the
    ORIGINAL ray's place, so the compositing runs on the original ``z`` and ``|d|``.

    There is no dense detour: ``split == "bf16x3"`` and a network shape other than 8 x 256 raise ``ValueError``, a volume on another
    device ``RuntimeError``, ``N S >= 2^31`` ``ValueError``.  ``counts``: optional int64 ``[2]`` device tensor, += (samples evaluated,
    samples), as in ``run_network_skip``.  Nothing reaches the host: after one warm-up call (``empty_row``) it can be captured in a
    graph and follows ``edit.source`` on replay.  ``_stages`` (tests): a dict that receives ``owner``, ``o_w``, ``d_w``, ``sel``,
    ``count``, ``kept`` and ``raw_net``, a copy of ``raw`` before the filter."""
    from .. import editing
    who = "run_network_edited"
    if not isinstance(edit, editing.FieldEdit):
        raise TypeError(f"{who}: edit must be an editing.FieldEdit")
    split = split or None
    if split not in (None, "f16x2"):
        raise ValueError(f"{who}: {EDITED_WORDS[0]} for args.mfma_split = {split!r} (f32 and 'f16x2' only)")
    if not model._fused_ok():
        raise ValueError(f"{who}: {EDITED_WORDS[1]} for the 8 x 256 network only")
    N, S = z_vals.shape
    M, C = N * S, model.ins_num + 1
    if M >= 2 ** 31:
        raise ValueError(f"{who}: {M} samples do not fit the int32 selection; {EDITED_WORDS[2]}")
    if edit.C != C:
        raise ValueError(f"{who}: the FieldEdit was made for C = {edit.C} labels, the model has ins_num + 1 = {C} (FieldEdit.from_source(..., C=))")
    rays_o, rays_d, z = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3)), _lib.f32(z_vals)
    _lib.require_gpu(rays_o, rays_d, z)
    dev = z.device
    if edit.source.device != dev:
        raise RuntimeError(f"{who}: the source volume lives on another device than the rays")
    if counts is not None:
        _lib.require_gpu(counts)
        if counts.dtype != torch.int64 or tuple(counts.shape) != (2,) or counts.device != dev or not counts.is_contiguous():
            raise ValueError(f"{who}: counts must be a contiguous int64 [2] tensor on the rays' device")
    raw = torch.empty(N, S, 4 + C, dtype=torch.float32, device=dev)
    if M == 0:
        return raw
    sel, owner, work = select_buffers(M, dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    o_w, d_w = torch.empty(M, 3, dtype=torch.float32, device=dev), torch.empty(M, 3, dtype=torch.float32, device=dev)
    fill = empty_row(C, dev)
    lo, _, inv_cell, dims = _lib.box_args(edit)
    _lib.launch("dmnerf_field_edit_select", edit.source, lo, inv_cell, dims,
                editing.FIELD_POLICIES[edit.outside], editing.FIELD_POLICIES[edit.unowned], edit.entries, edit.E, C, rays_o, rays_d, z, N, S,
                owner, o_w, d_w, sel, count, work, raw, fill, counts)
    if split == "f16x2":
        _lib.launch("dmnerf_mlp_fwd_rays_f16_sel", model.blob_f16(), model.ins_num, o_w, d_w, z, M, 1, sel, count, raw)
    else:
        _lib.launch("dmnerf_mlp_fwd_rays_sel", model.blob(), model.ins_num, 0, o_w, d_w, z, M, 1, sel, count, raw)
    kept = None
    if _stages is not None:
        kept = torch.empty(1 + edit.E, dtype=torch.int64, device=dev)
        _stages.update(owner=owner, o_w=o_w, d_w=d_w, sel=sel, count=count, kept=kept, raw_net=raw.clone())
    _lib.launch("dmnerf_field_edit_filter", raw, owner, M, C, edit.masks, edit.E, fill, kept)
    return raw


def check_draws(t_rand, u, N, S, n_imp, perturb, dev):
    """The two random tensors of one ``dm_nerf`` call, validated before raw pointers reach the kernels.
    ``perturb > 0``: ``t_rand [N,S]`` (render.py:46) then ``u [N,n_imp]`` (helpers.py:135), drawn here in the reference's
    order unless passed in.  Otherwise no jitter and ``u`` = the deterministic grid ``linspace(0,1,n_imp)`` shared by all
    rays (``det = (perturb == 0.)``, render.py:67) -- or a caller-supplied ``[n_imp]`` / ``[N,n_imp]`` tensor.
    Returns ``(t_rand or None, u, u_row_stride)``; a wrong shape raises instead of reading out of bounds."""
    if perturb > 0.:
        if t_rand is None:
            t_rand = torch.rand([N, S], device=dev)
        if u is None:
            u = torch.rand([N, n_imp], device=dev)
    else:
        t_rand = None
        if u is None:
            u = helpers.linspace01(n_imp, dev)
    if t_rand is not None:
        if tuple(t_rand.shape) != (N, S):
            raise ValueError(f"dm_nerf: t_rand must be [{N}, {S}] (one draw per coarse sample), got {tuple(t_rand.shape)}")
        t_rand = _lib.f32(t_rand)
        _lib.require_gpu(t_rand)
    if tuple(u.shape) not in ((n_imp,), (N, n_imp)):
        raise ValueError(f"dm_nerf: u must be [{n_imp}] or [{N}, {n_imp}], got {tuple(u.shape)}")
    u = _lib.f32(u)
    _lib.require_gpu(u)
    return t_rand, u, (0 if u.dim() == 1 else n_imp)


def _training(model_coarse, model_fine):
    # training = gradients are wanted for EITHER model (a frozen fine model with a trainable coarse one still trains)
    return torch.is_grad_enabled() and any(p.requires_grad for m in (model_coarse, model_fine) for p in m.parameters())


def _ray_inputs(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u):
    """The prologue of the inference entries: embedder widths, the rays and depths as f32 device tensors, sizes, and the validated
    draws (``check_draws``) -> the call's state, read by name."""
    for emb, want in ((position_embedder, model_fine.input_ch_pts), (view_embedder, model_fine.input_ch_views)):
        if getattr(emb, "out_dim", want) != want:
            raise ValueError("dm_nerf: the embedders' out_dim does not match the models' input channels")
    rays_o, rays_d = rays
    rays_o, rays_d = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3))
    z_in = _lib.f32(z_vals_coarse)
    _lib.require_gpu(rays_o, rays_d, z_in)
    p = SimpleNamespace(model_coarse=model_coarse, model_fine=model_fine, args=args, rays_o=rays_o, rays_d=rays_d, z_in=z_in,
                        dev=rays_o.device, N=z_in.shape[0], S=z_in.shape[1], n_imp=int(args.N_importance), f16=False)
    if p.n_imp < 0:                  # (dm_nerf only: the fine entries refuse N_importance < 1 before they get here)
        raise ValueError("dm_nerf: N_importance must be >= 0")
    p.t_rand, p.u, p.u_stride = check_draws(t_rand, u, p.N, p.S, p.n_imp, float(args.perturb), p.dev)
    return p


# args.fuse_heads (extension, default off): inference with the activation-free feature linears folded into the
# hidden layers (-19 % MACs; results equal up to f32 re-association)
# args.mfma_split (extension, default off): split-operand 16-bit MFMA inference (f32-class accuracy, not bitwise the f32
# chain): True / "bf16x3" = three bf16 planes, six products; "f16x2" = two f16 planes, three products
# What each of them runs on (``fused_heads``, blob, entries): ``weights.VARIANTS``.


def _fill_args(a, p, split, out, ws, _events, coarse_blob=None):
    """What ``RenderArgs`` and ``RenderFineArgs`` share: blobs / ``fused_heads`` by ``split`` or ``args.fuse_heads`` (``coarse_blob``:
    another one for the coarse model), rays, draws, sizes, the fine outputs, the weight workspace and the event pair."""
    v = weights.VARIANTS[split or ("fused" if bool(getattr(p.args, "fuse_heads", False)) else None)]
    a.fused_heads = v.fused_heads
    a.d_blob_coarse = getattr(p.model_coarse, coarse_blob or v.blob)().data_ptr()
    a.d_blob_fine = getattr(p.model_fine, v.blob)().data_ptr()
    a.ins_num = p.model_fine.ins_num
    a.d_rays_o, a.d_rays_d, a.d_z_in = p.rays_o.data_ptr(), p.rays_d.data_ptr(), p.z_in.data_ptr()
    a.d_t_rand = p.t_rand.data_ptr() if p.t_rand is not None else None
    a.d_u, a.u_row_stride = p.u.data_ptr(), p.u_stride
    a.N, a.S, a.n_imp = p.N, p.S, p.n_imp
    a.d_z_fine, a.d_raw_fine = out['z_vals_fine'].data_ptr(), out['raw_fine'].data_ptr()
    a.d_rgb_fine, a.d_depth_fine = out['rgb_fine'].data_ptr(), out['depth_fine'].data_ptr()
    a.d_ins_fine = out['ins_fine'].data_ptr()
    a.d_weights_ws = ws.data_ptr()
    if _events is not None:          # (begin, end) torch.cuda.Event pair around the fine-network MLP kernel
        for e in _events:
            e.record()               # torch creates the hipEvent_t lazily; the library re-records it in place
        a.ev_fine_mlp_begin, a.ev_fine_mlp_end = _events[0].cuda_event, _events[1].cuda_event


def ins_slice(out, args):
    """``ins_*`` of a training batch keep their last ``N_ins`` rays only (render.py:88-90) -> ``out``."""
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out.update({key: out[key][-args.N_ins:] for key in ('ins_fine', 'ins_coarse') if key in out})
    return out


def _epilogue(p, out):
    """After the launches: the opt-in f16 range probe (DMNERF_CHECK_F16=1 / args.check_f16: did a conversion saturate?) on the depths
    of a call that ran the f16x2 kernels, then the ``N_ins`` slice."""
    if p.f16:
        from .. import autograd
        if autograd.f16_check_enabled(p.args):
            model_coarse, model_fine, rays_o, rays_d = p.model_coarse, p.model_fine, p.rays_o, p.rays_d
            autograd.f16x2_probe(model_coarse, rays_o, rays_d, p.z_c)
            autograd.f16x2_probe(model_fine, rays_o, rays_d, out['z_vals_fine'])
            autograd.check_f16x2(p.dev)
    return ins_slice(out, p.args)


def dm_nerf(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
            t_rand=None, u=None, _events=None):
    """``dm_nerf`` (networks/render.py:31-96) -> the reference's 10-key dict.

    ``position_embedder`` / ``view_embedder`` are accepted for signature compatibility; the
    encoding (multires 10 / 4, the only values create_nerf's configs use) is computed inside the
    fused kernel.  RNG parity: with ``args.perturb > 0`` the reference draws ``torch.rand([N,S])``
    (render.py:46) and then ``torch.rand([N,N_importance])`` (helpers.py:135); the same two draws
    are made here, in that order, on the rays' device -- or pass ``t_rand`` / ``u`` (extension).
    ``_events``: optional (begin, end) ``torch.cuda.Event`` pair recorded around the fine MLP kernel.
    """
    if _training(model_coarse, model_fine):
        from .. import autograd
        # args.train_skip (extension, default None): a field.SkipGrid / field.TrainSkip -- the levels in args.train_skip_levels are
        # trained through the grid (autograd.run_network_train_skip); the reference's train loops opt in as with args.mfma_split
        return autograd.dm_nerf_train(rays, model_coarse, model_fine, z_vals_coarse, args, t_rand=t_rand, u=u,
                                      skip=getattr(args, "train_skip", None),             # (None: the levels are not looked at)
                                      skip_levels=getattr(args, "train_skip_levels", ("coarse", "fine")))
    p = _ray_inputs(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u)
    rays_o, rays_d, z_in, N, S, n_imp = p.rays_o, p.rays_d, p.z_in, p.N, p.S, p.n_imp
    if n_imp == 0 or not (model_coarse._fused_ok() and model_fine._fused_ok()):
        # composed from the stage kernels instead of the one fused call.  N_importance = 0 (config.py:43 allows it; no
        # shipped config uses it): sample_pdf returns [N, 0], the merged depths are the coarse ones (render.py:66-70) and the
        # fine network is evaluated on them.  A network shape other than the shipped one: run_network goes layer by layer.
        z_c = helpers.stratify(z_in, p.t_rand) if p.t_rand is not None else z_in
        raw_c = run_network(model_coarse, rays_o, rays_d, z_c)
        rgb_c, w_c, dep_c, ins_c = render_train(raw_c, z_c, rays_d)
        z_f = z_c.clone() if n_imp == 0 else helpers.importance_resample(z_c, w_c, n_imp, u=p.u)
        raw_f = run_network(model_fine, rays_o, rays_d, z_f)
        rgb_f, _, dep_f, ins_f = render_train(raw_f, z_f, rays_d)
        return _epilogue(p, {'rgb_fine': rgb_f, 'ins_fine': ins_f, 'z_vals_fine': z_f, 'raw_fine': raw_f, 'raw_coarse': raw_c,
                             'rgb_coarse': rgb_c, 'ins_coarse': ins_c, 'z_vals_coarse': z_c, 'depth_fine': dep_f, 'depth_coarse': dep_c})
    C = model_fine.ins_num + 1
    SF = S + n_imp
    f = dict(dtype=torch.float32, device=p.dev)
    out = {
        'rgb_fine': torch.empty(N, 3, **f), 'ins_fine': torch.empty(N, C - 1, **f),
        'z_vals_fine': torch.empty(N, SF, **f), 'raw_fine': torch.empty(N, SF, 4 + C, **f),
        'raw_coarse': torch.empty(N, S, 4 + C, **f), 'rgb_coarse': torch.empty(N, 3, **f),
        'ins_coarse': torch.empty(N, C - 1, **f),
        # without jitter the reference hands its input grid back (render.py:40-47 is skipped): alias, no copy
        'z_vals_coarse': torch.empty(N, S, **f) if p.t_rand is not None else z_in,
        'depth_fine': torch.empty(N, **f), 'depth_coarse': torch.empty(N, **f),
    }
    ws = torch.empty(N, SF, **f)
    a = _lib.RenderArgs()
    split = weights.split_mode(args)
    _fill_args(a, p, split, out, ws, _events)
    a.d_z_coarse, a.d_raw_coarse = out['z_vals_coarse'].data_ptr(), out['raw_coarse'].data_ptr()
    a.d_rgb_coarse, a.d_depth_coarse = out['rgb_coarse'].data_ptr(), out['depth_coarse'].data_ptr()
    a.d_ins_coarse = out['ins_coarse'].data_ptr()
    _lib.launch("dmnerf_render_rays_fwd", a)
    p.f16, p.z_c = split == "f16x2", out['z_vals_coarse']
    return _epilogue(p, out)


def _fine_mode(model_coarse, model_fine, args):
    """Which fine-only path serves this call: ``"f32"`` (``dm_nerf_fine``), ``"f16x2"`` (``dm_nerf_fine_f16``) or None -- training,
    another network than the shipped 8 x 256 one in either model, no hierarchical sampling, or bf16x3 (no density-only variant)."""
    if _training(model_coarse, model_fine) or not (model_coarse._fused_ok() and model_fine._fused_ok()) or int(args.N_importance) < 1:
        return None
    return {None: "f32", "f16x2": "f16x2"}.get(weights.split_mode(args))


def fine_eligible(model_coarse, model_fine, args):
    """Can ``dm_nerf_fine`` serve this call?  Inference, the shipped 8 x 256 network in both models, hierarchical sampling on,
    and the f32 kernels (f16x2 has a density-only variant of its own: ``fine_f16_eligible`` / ``dm_nerf_fine_f16``; bf16x3 has none)."""
    return _fine_mode(model_coarse, model_fine, args) == "f32"


def fine_f16_eligible(model_coarse, model_fine, args):
    """Can ``dm_nerf_fine_f16`` serve this call?  ``fine_eligible``'s conditions, with ``args.mfma_split = "f16x2"`` instead of f32."""
    return _fine_mode(model_coarse, model_fine, args) == "f16x2"


def fine_renderer(model_coarse, model_fine, args):
    """The chunk renderer of a caller that keeps the fine level only: ``dm_nerf_fine`` / ``dm_nerf_fine_f16`` where eligible, else
    ``dm_nerf``."""
    return {"f32": dm_nerf_fine, "f16x2": dm_nerf_fine_f16, None: dm_nerf}[_fine_mode(model_coarse, model_fine, args)]


def _fine_prepare(who, modes, rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u, _events):
    """Validation, draws, outputs and the filled ``RenderFineArgs`` of one fine-only render that serves ``modes`` of ``_fine_mode`` ->
    the call's state (``_ray_inputs``) with ``out``, the struct ``a`` and the tensors it points into: ``z_c``, ``sigma``, ``ws``."""
    mode = _fine_mode(model_coarse, model_fine, args)
    if mode not in modes:
        want = {("f32",): "no args.mfma_split", ("f16x2",): 'args.mfma_split = "f16x2"'}.get(tuple(modes), 'no args.mfma_split or "f16x2"')
        raise ValueError(f"{who}: inference with the 8 x 256 network, N_importance >= 1 and {want} only -- use dm_nerf")
    p = _ray_inputs(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u)
    N, S, SF, C = p.N, p.S, p.S + p.n_imp, model_fine.ins_num + 1
    f = dict(dtype=torch.float32, device=p.dev)
    p.out = {'rgb_fine': torch.empty(N, 3, **f), 'ins_fine': torch.empty(N, C - 1, **f), 'depth_fine': torch.empty(N, **f),
             'z_vals_fine': torch.empty(N, SF, **f), 'raw_fine': torch.empty(N, SF, 4 + C, **f)}
    p.z_c = torch.empty(N, S, **f) if p.t_rand is not None else p.z_in     # without jitter the coarse grid is read in place
    p.sigma, p.ws = torch.empty(N, S, **f), torch.empty(N, SF, **f)
    p.f16 = mode == "f16x2"
    p.a = _lib.RenderFineArgs()
    # f16x2: the linear weight stream wants a density blob of its own (f32: the trunk and its table entries are the same in both blobs)
    _fill_args(p.a, p, "f16x2" if p.f16 else None, p.out, p.ws, _events, coarse_blob="blob_f16_density" if p.f16 else None)
    p.a.d_z_coarse, p.a.d_sigma_ws = p.z_c.data_ptr(), p.sigma.data_ptr()
    return p


def _fine(who, modes, rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u, _events):
    p = _fine_prepare(who, modes, rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u, _events)
    _lib.launch("dmnerf_render_rays_fwd_fine", p.a)
    return _epilogue(p, p.out)


def dm_nerf_fine(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                 t_rand=None, u=None, _events=None):
    """``dm_nerf`` for a caller that keeps the fine level only, as ``render_test`` does (networks/tester.py:71-77 reads
    ``rgb_fine``, ``ins_fine``, ``depth_fine``): returns ``{'rgb_fine', 'ins_fine', 'depth_fine', 'z_vals_fine', 'raw_fine'}``,
    each ``torch.equal`` to the same key of ``dm_nerf`` called with the same arguments and draws.

    Of the coarse level only the compositing weights reach the fine one (render.py:66-70) and they depend on the density alone
    (:6-20), so the coarse network is evaluated up to ``density_linear`` (``dmnerf_mlp_fwd_rays_density``): no heads, no
    ``raw_coarse``, no coarse maps -- 29 % fewer MFMAs in that launch.  Arguments, validation and the order of the RNG draws are
    ``dm_nerf``'s.  Only for calls that are ``fine_eligible``; anything else raises (there is no silent detour)."""
    return _fine("dm_nerf_fine", ("f32",), rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                 t_rand, u, _events)


def dm_nerf_fine_f16(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                     t_rand=None, u=None, _events=None):
    """``dm_nerf_fine`` on the split-f16 kernels (``args.mfma_split = "f16x2"``): the coarse network runs as far as ``density_linear``
    (``dmnerf_mlp_fwd_rays_density_f16``, 122 instead of 140 + OBX weight groups), the fine one is ``dmnerf_mlp_fwd_rays_f16``.  Each
    returned key is ``torch.equal`` to the same key of ``dm_nerf`` called with the same f16x2 args and draws.  Signature, validation,
    draw order and keys are ``dm_nerf_fine``'s; only for calls that are ``fine_f16_eligible``, anything else raises."""
    return _fine("dm_nerf_fine_f16", ("f16x2",), rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                 t_rand, u, _events)


SKIP_LEVELS = {"coarse": 1, "fine": 2}          # DMNERF_SKIP_LEVEL_* (include/dmnerf_hip.h)


def dm_nerf_fine_skip(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, grid,
                      levels=("coarse", "fine"), t_rand=None, u=None, _events=None):
    """``dm_nerf_fine`` that does not march through empty space: at the levels named in ``levels`` the network is evaluated only
    at the samples whose cell of ``grid`` (a ``field.SkipGrid``) is set -- or that lie outside its box, with ``grid.outside ==
    "evaluate"`` -- and the other rows of the density / of ``raw_fine`` are zero.  A zero row is exactly neutral to the compositing
    ("Skipping empty space"), so every key equals the dense render with those rows masked; with ``SkipGrid.full`` it equals
    ``dm_nerf_fine`` bit for bit.  Returns ``dm_nerf_fine``'s keys plus ``n_eval``: int32 ``[2]`` on the device, the samples evaluated
    at the coarse and at the fine level.  The counts never reach the host, so the call can be captured in a graph and replayed after
    the grid's bits were overwritten in place.

    ``levels=("fine",)`` leaves the coarse pass dense: the grid comes from the FINE network's density, and masking the coarse
    network by it is an approximation the caller opts into.  Serves a call that is ``fine_eligible`` (the f32 kernels) or
    ``fine_f16_eligible`` (``args.mfma_split = "f16x2"``: ``dmnerf_mlp_fwd_rays_density_f16_sel`` / ``.._f16_sel``, equal to
    ``dm_nerf_fine_f16`` with ``SkipGrid.full``); validation and the order of the RNG draws are ``dm_nerf_fine``'s; anything else raises."""
    _require_grid("dm_nerf_fine_skip", grid)
    levels = check_skip_levels("dm_nerf_fine_skip", levels)
    p = _fine_prepare("dm_nerf_fine_skip", ("f32", "f16x2"), rays, position_embedder, view_embedder, model_coarse, model_fine,
                      z_vals_coarse, args, t_rand, u, _events)
    out, dev = p.out, p.dev
    if grid.bits.device != dev:
        raise RuntimeError("dm_nerf_fine_skip: the grid lives on another device than the rays")
    N, SF = out['z_vals_fine'].shape
    if N * SF >= 2 ** 31:
        raise ValueError(f"dm_nerf_fine_skip: {N * SF} samples do not fit the int32 selection; render in smaller chunks")
    sel, flag, work = select_buffers(N * SF, dev, n_min=1)
    out['n_eval'] = torch.empty(2, dtype=torch.int32, device=dev)
    k = _lib.RenderFineSkipArgs()
    k.fine = p.a
    k.grid = grid.c_struct()
    k.d_sel, k.d_flag, k.d_select_ws, k.d_n_eval = sel.data_ptr(), flag.data_ptr(), work.data_ptr(), out['n_eval'].data_ptr()
    k.levels = sum(SKIP_LEVELS[l] for l in set(levels))
    _lib.launch("dmnerf_render_rays_fwd_fine_skip", k)
    return _epilogue(p, out)


def dm_nerf_fine_mark(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, grid, threshold=0.0,
                      levels=("coarse", "fine"), t_rand=None, u=None, _events=None):
    """``dm_nerf_fine`` (or, with ``args.mfma_split = "f16x2"``, ``dm_nerf_fine_f16``) that also records in ``grid`` (a
    ``field.SkipGrid``, marked in place) which cells the render used: the cell of every sample whose compositing weight is
    ``> threshold``.  The render is the dense one, unchanged -- the same ``dmnerf_render_rays_fwd_fine`` call -- so the returned keys
    are ``torch.equal`` to ``dm_nerf_fine``'s.

    ``"fine"`` in ``levels``: marked with ``z_vals_fine`` and the fine weights the compositing left in its workspace.  ``"coarse"``:
    the coarse weights are recomputed from the coarse density the render left behind (``dmnerf_weights_from_sigma``, the kernel the
    render itself ran, on the same inputs: these are the weights the resampler saw) into a scratch of this call, and marked with the
    coarse depths the networks saw -- the jittered ones when ``args.perturb > 0``.  Nothing reaches the host and nothing is allocated
    between the launches, so the call can be captured in a graph.  Serves the calls ``dm_nerf_fine_skip`` serves; anything else raises."""
    _require_grid("dm_nerf_fine_mark", grid)
    levels = check_skip_levels("dm_nerf_fine_mark", levels)
    p = _fine_prepare("dm_nerf_fine_mark", ("f32", "f16x2"), rays, position_embedder, view_embedder, model_coarse, model_fine,
                      z_vals_coarse, args, t_rand, u, _events)
    rays_o, rays_d, z_c = p.rays_o, p.rays_d, p.z_c
    if grid.bits.device != p.dev:
        raise RuntimeError("dm_nerf_fine_mark: the grid lives on another device than the rays")
    N, S = z_c.shape
    w_c = torch.empty(N, S, dtype=torch.float32, device=p.dev) if "coarse" in levels else None
    _lib.launch("dmnerf_render_rays_fwd_fine", p.a)
    if "fine" in levels:
        grid.mark(rays_o, rays_d, p.out['z_vals_fine'], p.ws, threshold)
    if w_c is not None and N:
        _lib.launch("dmnerf_weights_from_sigma", p.sigma, z_c, rays_d, N, S, w_c)
        grid.mark(rays_o, rays_d, z_c, w_c, threshold)
    return _epilogue(p, p.out)
