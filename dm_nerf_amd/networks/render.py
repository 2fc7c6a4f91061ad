"""Drop-in for the reference's ``networks/render.py``: render_train, dm_nerf."""
import ctypes

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
    _lib.check(_lib.load().dmnerf_composite_fwd(_lib.ptr(raw), _lib.ptr(z), _lib.ptr(d), N, S, C, _lib.ptr(rgb), _lib.ptr(w),
                                                _lib.ptr(depth), _lib.ptr(ins), _lib.stream()), "dmnerf_composite_fwd")
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
    lib = _lib.load()
    fn, blob, name = {None: (lib.dmnerf_mlp_fwd_rays, model.blob, "dmnerf_mlp_fwd_rays"),
                      "bf16x3": (lib.dmnerf_mlp_fwd_rays_split, model.blob_split, "dmnerf_mlp_fwd_rays_split"),
                      "f16x2": (lib.dmnerf_mlp_fwd_rays_f16, model.blob_f16, "dmnerf_mlp_fwd_rays_f16")}[split or None]
    _lib.check(fn(_lib.ptr(blob()), model.ins_num, _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z), N, S, _lib.ptr(raw), _lib.stream()), name)
    return raw


_empty_rows = {}


def empty_row(C, device):
    """The EMPTY ROW ``E = (0, 0, 0, 0 | 0, .., 0, 1)`` of width ``4 + C`` on ``device``: sigma, rgb and the object logits 0, the last
    ("empty") logit 1.  Its weight in ``manipulator_render`` is exactly 0 and the argmax over its C logits is ``C - 1``.
    Built on the device (no host copy) and kept per width and device; as with the weight blobs, make one call outside a graph capture
    first, so that the kept tensor does not come from the capture's memory pool."""
    key = (int(C), str(device))
    if key not in _empty_rows:
        row = torch.zeros(4 + int(C), dtype=torch.float32, device=device)
        row[-1:].fill_(1.0)
        _empty_rows[key] = row
    return _empty_rows[key]


def check_skip_levels(who, levels):
    """``levels`` as a tuple of ``SKIP_LEVELS`` names, validated as ``dm_nerf_fine_skip`` validates it."""
    levels = (levels,) if isinstance(levels, str) else tuple(levels)
    if not levels or any(l not in SKIP_LEVELS for l in levels):
        raise ValueError(f"{who}: levels must name 'coarse' and / or 'fine', got {levels}")
    return levels


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
    from .. import field
    if not isinstance(grid, field.SkipGrid):
        raise TypeError("run_network_skip: grid must be a field.SkipGrid")
    split = split or None
    if split not in (None, "f16x2"):
        raise ValueError(f"run_network_skip: no sparse network kernel for args.mfma_split = {split!r} (f32 and 'f16x2' only)")
    if not model._fused_ok():
        raise ValueError("run_network_skip: the sparse network kernels exist for the 8 x 256 network only")
    N, S = z_vals.shape
    if N * S >= 2 ** 31:
        raise ValueError(f"run_network_skip: {N * S} samples do not fit the int32 selection; render in smaller chunks")
    rays_o, rays_d, z = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3)), _lib.f32(z_vals)
    _lib.require_gpu(rays_o, rays_d, z)
    dev = z.device
    if grid.bits.device != dev:
        raise RuntimeError("run_network_skip: the grid lives on another device than the rays")
    if counts is not None:
        _lib.require_gpu(counts)
        if counts.dtype != torch.int64 or tuple(counts.shape) != (2,) or counts.device != dev or not counts.is_contiguous():
            raise ValueError("run_network_skip: counts must be a contiguous int64 [2] tensor on the rays' device")
    C = model.ins_num + 1
    raw = torch.empty(N, S, 4 + C, dtype=torch.float32, device=dev)
    if N * S == 0:
        return raw
    lib = _lib.load()
    sel = torch.empty(N * S, dtype=torch.int32, device=dev)
    flag = torch.empty(N * S, dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(N * S)), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    g = grid.c_struct()
    st = _lib.stream()
    _lib.check(lib.dmnerf_skip_select_fill(ctypes.byref(g), _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z), N, S, _lib.ptr(flag),
                                           _lib.ptr(sel), _lib.ptr(count), _lib.ptr(work), _lib.ptr(raw), _lib.ptr(empty_row(C, dev)),
                                           4 + C, _lib.ptr(counts), st), "dmnerf_skip_select_fill")
    if split == "f16x2":
        _lib.check(lib.dmnerf_mlp_fwd_rays_f16_sel(_lib.ptr(model.blob_f16()), model.ins_num, _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z),
                                                   N, S, _lib.ptr(sel), _lib.ptr(count), _lib.ptr(raw), st), "dmnerf_mlp_fwd_rays_f16_sel")
    else:
        _lib.check(lib.dmnerf_mlp_fwd_rays_sel(_lib.ptr(model.blob()), model.ins_num, 0, _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z),
                                               N, S, _lib.ptr(sel), _lib.ptr(count), _lib.ptr(raw), st), "dmnerf_mlp_fwd_rays_sel")
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
    # training = gradients are wanted for EITHER model (a frozen fine model with a trainable coarse one still trains)
    training = torch.is_grad_enabled() and any(p.requires_grad for m in (model_coarse, model_fine) for p in m.parameters())
    if training:
        from .. import autograd
        # args.train_skip (extension, default None): a field.SkipGrid / field.TrainSkip -- the levels in args.train_skip_levels are
        # trained through the grid (autograd.run_network_train_skip); the reference's train loops opt in as with args.mfma_split
        grid = getattr(args, "train_skip", None)
        if grid is None:
            return autograd.dm_nerf_train(rays, model_coarse, model_fine, z_vals_coarse, args, t_rand=t_rand, u=u)
        return autograd.dm_nerf_train(rays, model_coarse, model_fine, z_vals_coarse, args, t_rand=t_rand, u=u, skip=grid,
                                      skip_levels=getattr(args, "train_skip_levels", ("coarse", "fine")))
    for emb, want in ((position_embedder, model_fine.input_ch_pts), (view_embedder, model_fine.input_ch_views)):
        if getattr(emb, "out_dim", want) != want:
            raise ValueError("dm_nerf: the embedders' out_dim does not match the models' input channels")
    rays_o, rays_d = rays
    rays_o, rays_d = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3))
    z_in = _lib.f32(z_vals_coarse)
    _lib.require_gpu(rays_o, rays_d, z_in)
    dev = rays_o.device
    N, S = z_in.shape
    n_imp = int(args.N_importance)
    if n_imp < 0:
        raise ValueError("dm_nerf: N_importance must be >= 0")
    ins_num = model_fine.ins_num
    C = ins_num + 1
    perturb = float(args.perturb)
    t_rand, u, u_stride = check_draws(t_rand, u, N, S, n_imp, perturb, dev)
    if n_imp == 0 or not (model_coarse._fused_ok() and model_fine._fused_ok()):
        # composed from the stage kernels instead of the one fused call.  N_importance = 0 (config.py:43 allows it; no
        # shipped config uses it): sample_pdf returns [N, 0], the merged depths are the coarse ones (render.py:66-70) and the
        # fine network is evaluated on them.  A network shape other than the shipped one: run_network goes layer by layer.
        z_c = helpers.stratify(z_in, t_rand) if t_rand is not None else z_in
        raw_c = run_network(model_coarse, rays_o, rays_d, z_c)
        rgb_c, w_c, dep_c, ins_c = render_train(raw_c, z_c, rays_d)
        z_f = z_c.clone() if n_imp == 0 else helpers.importance_resample(z_c, w_c, n_imp, u=u)
        raw_f = run_network(model_fine, rays_o, rays_d, z_f)
        rgb_f, _, dep_f, ins_f = render_train(raw_f, z_f, rays_d)
        if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
            ins_f, ins_c = ins_f[-args.N_ins:], ins_c[-args.N_ins:]
        return {'rgb_fine': rgb_f, 'ins_fine': ins_f, 'z_vals_fine': z_f, 'raw_fine': raw_f, 'raw_coarse': raw_c, 'rgb_coarse': rgb_c,
                'ins_coarse': ins_c, 'z_vals_coarse': z_c, 'depth_fine': dep_f, 'depth_coarse': dep_c}
    SF = S + n_imp
    f = dict(dtype=torch.float32, device=dev)
    out = {
        'rgb_fine': torch.empty(N, 3, **f), 'ins_fine': torch.empty(N, C - 1, **f),
        'z_vals_fine': torch.empty(N, SF, **f), 'raw_fine': torch.empty(N, SF, 4 + C, **f),
        'raw_coarse': torch.empty(N, S, 4 + C, **f), 'rgb_coarse': torch.empty(N, 3, **f),
        'ins_coarse': torch.empty(N, C - 1, **f),
        # without jitter the reference hands its input grid back (render.py:40-47 is skipped): alias, no copy
        'z_vals_coarse': torch.empty(N, S, **f) if t_rand is not None else z_in,
        'depth_fine': torch.empty(N, **f), 'depth_coarse': torch.empty(N, **f),
    }
    ws = torch.empty(N, SF, **f)
    a = _lib.RenderArgs()
    # args.fuse_heads (extension, default off): inference with the activation-free feature linears folded into the
    # hidden layers (-19 % MACs; results equal up to f32 re-association)
    # args.mfma_split (extension, default off): split-operand 16-bit MFMA inference (f32-class accuracy, not bitwise the f32
    # chain): True / "bf16x3" = three bf16 planes, six products; "f16x2" = two f16 planes, three products
    fused = bool(getattr(args, "fuse_heads", False))
    split = weights.split_mode(args)
    a.fused_heads = {"bf16x3": 2, "f16x2": 3}[split] if split else (1 if fused else 0)
    pick = {"bf16x3": (lambda mdl: mdl.blob_split()), "f16x2": (lambda mdl: mdl.blob_f16())}[split] if split else \
        ((lambda mdl: mdl.blob_fused()) if fused else (lambda mdl: mdl.blob()))
    a.d_blob_coarse = pick(model_coarse).data_ptr()
    a.d_blob_fine = pick(model_fine).data_ptr()
    a.ins_num = ins_num
    a.d_rays_o, a.d_rays_d, a.d_z_in = rays_o.data_ptr(), rays_d.data_ptr(), z_in.data_ptr()
    a.d_t_rand = t_rand.data_ptr() if t_rand is not None else None
    a.d_u, a.u_row_stride = u.data_ptr(), u_stride
    a.N, a.S, a.n_imp = N, S, n_imp
    a.d_z_coarse, a.d_raw_coarse = out['z_vals_coarse'].data_ptr(), out['raw_coarse'].data_ptr()
    a.d_rgb_coarse, a.d_depth_coarse = out['rgb_coarse'].data_ptr(), out['depth_coarse'].data_ptr()
    a.d_ins_coarse = out['ins_coarse'].data_ptr()
    a.d_z_fine, a.d_raw_fine = out['z_vals_fine'].data_ptr(), out['raw_fine'].data_ptr()
    a.d_rgb_fine, a.d_depth_fine = out['rgb_fine'].data_ptr(), out['depth_fine'].data_ptr()
    a.d_ins_fine = out['ins_fine'].data_ptr()
    a.d_weights_ws = ws.data_ptr()
    if _events is not None:          # (begin, end) torch.cuda.Event pair around the fine-network MLP kernel
        for e in _events:
            e.record()               # torch creates the hipEvent_t lazily; the library re-records it in place
        a.ev_fine_mlp_begin, a.ev_fine_mlp_end = _events[0].cuda_event, _events[1].cuda_event
    _lib.check(_lib.load().dmnerf_render_rays_fwd(ctypes.byref(a), _lib.stream()), "dmnerf_render_rays_fwd")
    if split == "f16x2":
        from .. import autograd
        if autograd.f16_check_enabled(args):             # opt-in diagnostic (DMNERF_CHECK_F16=1 / args.check_f16): did a conversion saturate?
            autograd.f16x2_probe(model_coarse, rays_o, rays_d, out['z_vals_coarse'])
            autograd.f16x2_probe(model_fine, rays_o, rays_d, out['z_vals_fine'])
            autograd.check_f16x2(dev)
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out['ins_fine'] = out['ins_fine'][-args.N_ins:]          # render.py:88-90
        out['ins_coarse'] = out['ins_coarse'][-args.N_ins:]
    return out


def _training(model_coarse, model_fine):
    return torch.is_grad_enabled() and any(p.requires_grad for m in (model_coarse, model_fine) for p in m.parameters())


def fine_eligible(model_coarse, model_fine, args):
    """Can ``dm_nerf_fine`` serve this call?  Inference, the shipped 8 x 256 network in both models, hierarchical sampling on,
    and the f32 kernels (f16x2 has a density-only variant of its own: ``fine_f16_eligible`` / ``dm_nerf_fine_f16``; bf16x3 has none)."""
    return (not _training(model_coarse, model_fine) and model_coarse._fused_ok() and model_fine._fused_ok()
            and int(args.N_importance) >= 1 and not weights.split_mode(args))


def fine_f16_eligible(model_coarse, model_fine, args):
    """Can ``dm_nerf_fine_f16`` serve this call?  ``fine_eligible``'s conditions with ``args.mfma_split = "f16x2"`` instead of the f32
    kernels (bf16x3 has no density-only variant)."""
    return (not _training(model_coarse, model_fine) and model_coarse._fused_ok() and model_fine._fused_ok()
            and int(args.N_importance) >= 1 and weights.split_mode(args) == "f16x2")


def _fine_prepare(who, rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args, t_rand, u, _events,
                  modes=("f32",)):
    """Validation, draws, outputs and the filled ``RenderFineArgs`` of one fine-only render -> ``(out, a, keep)``; ``keep`` holds the
    tensors the struct points into.  ``modes``: which of the f32 kernels (``fine_eligible``) and the f16x2 kernels
    (``fine_f16_eligible``) the caller serves."""
    f16 = "f16x2" in modes and fine_f16_eligible(model_coarse, model_fine, args)
    if not f16 and not ("f32" in modes and fine_eligible(model_coarse, model_fine, args)):
        want = {("f32",): "no args.mfma_split", ("f16x2",): 'args.mfma_split = "f16x2"'}.get(tuple(modes), 'no args.mfma_split or "f16x2"')
        raise ValueError(f"{who}: inference with the 8 x 256 network, N_importance >= 1 and {want} only -- use dm_nerf")
    for emb, want in ((position_embedder, model_fine.input_ch_pts), (view_embedder, model_fine.input_ch_views)):
        if getattr(emb, "out_dim", want) != want:
            raise ValueError("dm_nerf: the embedders' out_dim does not match the models' input channels")
    rays_o, rays_d = rays
    rays_o, rays_d = _lib.f32(rays_o.reshape(-1, 3)), _lib.f32(rays_d.reshape(-1, 3))
    z_in = _lib.f32(z_vals_coarse)
    _lib.require_gpu(rays_o, rays_d, z_in)
    dev = rays_o.device
    N, S = z_in.shape
    n_imp = int(args.N_importance)
    ins_num = model_fine.ins_num
    C = ins_num + 1
    t_rand, u, u_stride = check_draws(t_rand, u, N, S, n_imp, float(args.perturb), dev)
    SF = S + n_imp
    f = dict(dtype=torch.float32, device=dev)
    out = {'rgb_fine': torch.empty(N, 3, **f), 'ins_fine': torch.empty(N, C - 1, **f), 'depth_fine': torch.empty(N, **f),
           'z_vals_fine': torch.empty(N, SF, **f), 'raw_fine': torch.empty(N, SF, 4 + C, **f)}
    z_c = torch.empty(N, S, **f) if t_rand is not None else z_in     # without jitter the coarse grid is read in place
    sigma, ws = torch.empty(N, S, **f), torch.empty(N, SF, **f)
    fused = bool(getattr(args, "fuse_heads", False))
    pick = (lambda mdl: mdl.blob_fused()) if fused else (lambda mdl: mdl.blob())
    a = _lib.RenderFineArgs()
    if f16:                                                          # the linear weight stream wants a density blob of its own
        a.fused_heads = 3
        a.d_blob_coarse = model_coarse.blob_f16_density().data_ptr()
        a.d_blob_fine = model_fine.blob_f16().data_ptr()
    else:
        a.fused_heads = 1 if fused else 0
        a.d_blob_coarse = pick(model_coarse).data_ptr()              # (the trunk and its table entries are the same in both blobs)
        a.d_blob_fine = pick(model_fine).data_ptr()
    a.ins_num = ins_num
    a.d_rays_o, a.d_rays_d, a.d_z_in = rays_o.data_ptr(), rays_d.data_ptr(), z_in.data_ptr()
    a.d_t_rand = t_rand.data_ptr() if t_rand is not None else None
    a.d_u, a.u_row_stride = u.data_ptr(), u_stride
    a.N, a.S, a.n_imp = N, S, n_imp
    a.d_z_coarse, a.d_sigma_ws, a.d_weights_ws = z_c.data_ptr(), sigma.data_ptr(), ws.data_ptr()
    a.d_z_fine, a.d_raw_fine = out['z_vals_fine'].data_ptr(), out['raw_fine'].data_ptr()
    a.d_rgb_fine, a.d_depth_fine = out['rgb_fine'].data_ptr(), out['depth_fine'].data_ptr()
    a.d_ins_fine = out['ins_fine'].data_ptr()
    if _events is not None:          # (begin, end) torch.cuda.Event pair around the fine-network MLP kernel
        for e in _events:
            e.record()               # torch creates the hipEvent_t lazily; the library re-records it in place
        a.ev_fine_mlp_begin, a.ev_fine_mlp_end = _events[0].cuda_event, _events[1].cuda_event
    return out, a, (rays_o, rays_d, z_in, t_rand, u, z_c, sigma, ws)


def dm_nerf_fine(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                 t_rand=None, u=None, _events=None):
    """``dm_nerf`` for a caller that keeps the fine level only, as ``render_test`` does (networks/tester.py:71-77 reads
    ``rgb_fine``, ``ins_fine``, ``depth_fine``): returns ``{'rgb_fine', 'ins_fine', 'depth_fine', 'z_vals_fine', 'raw_fine'}``,
    each ``torch.equal`` to the same key of ``dm_nerf`` called with the same arguments and draws.

    Of the coarse level only the compositing weights reach the fine one (render.py:66-70) and they depend on the density alone
    (:6-20), so the coarse network is evaluated up to ``density_linear`` (``dmnerf_mlp_fwd_rays_density``): no heads, no
    ``raw_coarse``, no coarse maps -- 29 % fewer MFMAs in that launch.  Arguments, validation and the order of the RNG draws are
    ``dm_nerf``'s.  Only for calls that are ``fine_eligible``; anything else raises (there is no silent detour)."""
    out, a, _keep = _fine_prepare("dm_nerf_fine", rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                                  t_rand, u, _events)
    _lib.check(_lib.load().dmnerf_render_rays_fwd_fine(ctypes.byref(a), _lib.stream()), "dmnerf_render_rays_fwd_fine")
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out['ins_fine'] = out['ins_fine'][-args.N_ins:]          # render.py:88-90
    return out


def _f16_probe(model_coarse, model_fine, args, keep, out):
    """The opt-in f16 range probe of ``dm_nerf`` (DMNERF_CHECK_F16=1 / args.check_f16), on the same depths."""
    from .. import autograd
    if autograd.f16_check_enabled(args):
        rays_o, rays_d, z_c = keep[0], keep[1], keep[5]
        autograd.f16x2_probe(model_coarse, rays_o, rays_d, z_c)
        autograd.f16x2_probe(model_fine, rays_o, rays_d, out['z_vals_fine'])
        autograd.check_f16x2(rays_o.device)


def dm_nerf_fine_f16(rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse, args,
                     t_rand=None, u=None, _events=None):
    """``dm_nerf_fine`` on the split-f16 kernels (``args.mfma_split = "f16x2"``): the coarse network runs as far as ``density_linear``
    (``dmnerf_mlp_fwd_rays_density_f16``, 122 instead of 140 + OBX weight groups), the fine one is ``dmnerf_mlp_fwd_rays_f16``.  Each
    returned key is ``torch.equal`` to the same key of ``dm_nerf`` called with the same f16x2 args and draws.  Signature, validation,
    draw order and keys are ``dm_nerf_fine``'s; only for calls that are ``fine_f16_eligible``, anything else raises."""
    out, a, keep = _fine_prepare("dm_nerf_fine_f16", rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse,
                                 args, t_rand, u, _events, modes=("f16x2",))
    _lib.check(_lib.load().dmnerf_render_rays_fwd_fine(ctypes.byref(a), _lib.stream()), "dmnerf_render_rays_fwd_fine")
    _f16_probe(model_coarse, model_fine, args, keep, out)
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out['ins_fine'] = out['ins_fine'][-args.N_ins:]          # render.py:88-90
    return out


def fine_renderer(model_coarse, model_fine, args):
    """The chunk renderer of a caller that keeps the fine level only: ``dm_nerf_fine`` / ``dm_nerf_fine_f16`` where eligible, else
    ``dm_nerf``."""
    if fine_eligible(model_coarse, model_fine, args):
        return dm_nerf_fine
    if fine_f16_eligible(model_coarse, model_fine, args):
        return dm_nerf_fine_f16
    return dm_nerf


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
    from .. import field
    if not isinstance(grid, field.SkipGrid):
        raise TypeError("dm_nerf_fine_skip: grid must be a field.SkipGrid")
    levels = check_skip_levels("dm_nerf_fine_skip", levels)
    out, a, _keep = _fine_prepare("dm_nerf_fine_skip", rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse,
                                  args, t_rand, u, _events, modes=("f32", "f16x2"))
    dev = out['raw_fine'].device
    if grid.bits.device != dev:
        raise RuntimeError("dm_nerf_fine_skip: the grid lives on another device than the rays")
    N, SF = out['z_vals_fine'].shape
    if N * SF >= 2 ** 31:
        raise ValueError(f"dm_nerf_fine_skip: {N * SF} samples do not fit the int32 selection; render in smaller chunks")
    lib = _lib.load()
    sel = torch.empty(max(N * SF, 1), dtype=torch.int32, device=dev)
    flag = torch.empty(max(N * SF, 1), dtype=torch.uint8, device=dev)
    work = torch.empty(int(lib.dmnerf_skip_select_work_ints(N * SF)), dtype=torch.int32, device=dev)
    out['n_eval'] = torch.empty(2, dtype=torch.int32, device=dev)
    k = _lib.RenderFineSkipArgs()
    k.fine = a
    k.grid = grid.c_struct()
    k.d_sel, k.d_flag, k.d_select_ws, k.d_n_eval = sel.data_ptr(), flag.data_ptr(), work.data_ptr(), out['n_eval'].data_ptr()
    k.levels = sum(SKIP_LEVELS[l] for l in set(levels))
    _lib.check(lib.dmnerf_render_rays_fwd_fine_skip(ctypes.byref(k), _lib.stream()), "dmnerf_render_rays_fwd_fine_skip")
    if a.fused_heads == 3:
        _f16_probe(model_coarse, model_fine, args, _keep, out)
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out['ins_fine'] = out['ins_fine'][-args.N_ins:]          # render.py:88-90
    return out


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
    from .. import field
    if not isinstance(grid, field.SkipGrid):
        raise TypeError("dm_nerf_fine_mark: grid must be a field.SkipGrid")
    levels = check_skip_levels("dm_nerf_fine_mark", levels)
    out, a, keep = _fine_prepare("dm_nerf_fine_mark", rays, position_embedder, view_embedder, model_coarse, model_fine, z_vals_coarse,
                                 args, t_rand, u, _events, modes=("f32", "f16x2"))
    rays_o, rays_d, z_c, sigma, ws = keep[0], keep[1], keep[5], keep[6], keep[7]
    if grid.bits.device != rays_o.device:
        raise RuntimeError("dm_nerf_fine_mark: the grid lives on another device than the rays")
    N, S = z_c.shape
    w_c = torch.empty(N, S, dtype=torch.float32, device=rays_o.device) if "coarse" in levels else None
    lib = _lib.load()
    _lib.check(lib.dmnerf_render_rays_fwd_fine(ctypes.byref(a), _lib.stream()), "dmnerf_render_rays_fwd_fine")
    if "fine" in levels:
        grid.mark(rays_o, rays_d, out['z_vals_fine'], ws, threshold)
    if w_c is not None and N:
        _lib.check(lib.dmnerf_weights_from_sigma(_lib.ptr(sigma), _lib.ptr(z_c), _lib.ptr(rays_d), N, S, _lib.ptr(w_c), _lib.stream()),
                   "dmnerf_weights_from_sigma")
        grid.mark(rays_o, rays_d, z_c, w_c, threshold)
    if a.fused_heads == 3:
        _f16_probe(model_coarse, model_fine, args, keep, out)
    if getattr(args, "is_train", False) and getattr(args, "N_ins", None) is not None:
        out['ins_fine'] = out['ins_fine'][-args.N_ins:]          # render.py:88-90
    return out
