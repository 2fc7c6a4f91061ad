"""One process per GPU (torchrun), RCCL over xGMI via ``torch.distributed`` (backend "nccl" on ROCm).

Rays are independent units, so the path shards with no data-path collective:

* render (reference: the serial chunk loop of ``render_test``, networks/tester.py:55-85): rank r owns
  a contiguous band of image rows, generates its own rays (no scatter), renders them in chunks,
  and ONE all-gather per frame of one packed band buffer assembles ``rgb [H,W,3]``, ``ins [H,W,ins_num]``,
  ``depth [H,W]`` (``FrameRenderer``; replaces the O(chunks^2) ``torch.cat`` accumulation, tester.py:73-77).
* training: every rank renders a slice of the same ray batch; ``allreduce_grads`` sums the gradients
  of both models in one flat 5.57 MB bucket per step (after ``total_loss.backward()``,
  train_dmsr.py:63); ``all_gather_cat`` exchanges the small per-ray outputs that batch-global
  losses (Hungarian matching, soft-IoU; networks/evaluator.py:19-74) need.

Nothing here touches kernels: the collectives move finished tiles / gradients only.  The chunk
renderer and ray generator are injectable so the sharding logic is tested on CPU with gloo.
"""
import os

import torch
import torch.distributed as dist


def init_from_env(backend=None):
    """Initialise the default process group from torchrun's environment (idempotent).
    Returns (rank, world, device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda", local) if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(local)
    if (world > 1 or force_collectives()) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        kw = {"device_id": device} if use_cuda else {}
        dist.init_process_group(backend or ("nccl" if use_cuda else "gloo"), rank=rank, world_size=world, **kw)
    return rank, world, device


def world_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


_force = [False]


def force_collectives(on=None):
    """``DMNERF_FORCE_COLLECTIVES=1`` (or ``force_collectives(True)``): issue every collective of this module even in a world of
    ONE rank, where they are otherwise skipped as no-ops.  A one-GPU box can then drive the exact RCCL calls of the 8-GPU run --
    the packed all-gather, the 64-B all-reduce, the in-place arena all-reduce, the frame gather -- through the product code with
    ``init_process_group("nccl", world_size=1, device_id=...)`` and compare against the skipped path bit for bit
    (tests/test_gpu_rccl.py).  Needs an initialised process group; returns the current setting."""
    if on is not None:
        _force[0] = bool(on)
    return _force[0] or os.environ.get("DMNERF_FORCE_COLLECTIVES") == "1"


def _active(world):
    """Whether collectives are issued: more than one rank, or forced in an initialised world of one."""
    return world > 1 or (force_collectives() and dist.is_available() and dist.is_initialized())


# Tally of the collectives this module issued (host-side counters, no synchronisation): what a bench line reports as
# ``collectives_per_step`` / bytes so that a multi-rank record says what crossed the links, not only how long it took.
_tally = {"count": 0, "bytes": 0, "kinds": {}}


def _count(kind, t):
    _tally["count"] += 1
    _tally["bytes"] += t.numel() * t.element_size()
    _tally["kinds"][kind] = _tally["kinds"].get(kind, 0) + 1


def collective_tally(reset=False):
    """``{"count", "bytes", "kinds"}`` of the collectives issued through this module since the last reset (``bytes`` = the size of
    each call's local send buffer; an all-gather delivers ``world`` times that to every rank)."""
    out = {"count": _tally["count"], "bytes": _tally["bytes"], "kinds": dict(_tally["kinds"])}
    if reset:
        _tally.update(count=0, bytes=0, kinds={})
    return out


def row_band(H, rank, world):
    """Contiguous band of image rows of rank ``rank``: (row0, nrows); bands differ by at most one row."""
    base, rem = divmod(int(H), int(world))
    row0 = rank * base + min(rank, rem)
    return row0, base + (1 if rank < rem else 0)


def ray_slice(N, rank, world):
    """Contiguous slice of a ray batch (training): (start, count)."""
    return row_band(N, rank, world)


def all_gather_cat(t, sizes=None):
    """Concatenate ``t`` (dim 0) over ranks.  ``sizes``: per-rank dim-0 lengths when they differ."""
    rank, world = world_info()
    if not _active(world):
        return t
    t = t.contiguous()

    # The collective is chosen UP FRONT from the backend, identically on every rank -- never by catching an exception
    # (a failure on some ranks only would make the ranks issue different collectives and hang; a real RCCL error must
    # surface): RCCL ("nccl") has the single-buffer form, gloo gathers into a list.
    tensor_form = dist.get_backend() == "nccl"

    def gather(x):                                       # [n, ...] -> [world * n, ...]
        if tensor_form:
            out = torch.empty((world * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            dist.all_gather_into_tensor(out, x)          # one RCCL all-gather
            _count("all_gather", x)
            return out
        parts = [torch.empty_like(x) for _ in range(world)]
        dist.all_gather(parts, x)
        _count("all_gather", x)
        return torch.cat(parts, 0)

    if sizes is None or len(set(sizes)) == 1:
        return gather(t)
    mx = max(sizes)
    pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[:t.shape[0]] = t
    out = gather(pad)
    return torch.cat([out[r * mx:r * mx + sizes[r]] for r in range(world)], 0)


def allreduce_grads(models, average=False, arena=None):
    """Sum (or average) the gradients of ``models`` across ranks in ONE flat message (5.57 MB at ins_num 13).

    With a ``GradArena`` (dm_nerf_amd.autograd) whose slots the backward kernels filled, the parameters' ``.grad`` ARE
    views of one buffer and that buffer is all-reduced in place: no ``cat``, no copies.  Otherwise the bucket is built
    over all parameters that require a gradient, zero-filling those this rank has none for, so that every rank contributes
    the same number of elements whatever it rendered (a rank whose slice produced no gradient for some tensor must not shrink
    its bucket); one flag per parameter rides in the same message, and a tensor no rank had a gradient for keeps ``grad = None``
    (single-process semantics: the optimizer skips it).  The result is copied back."""
    rank, world = world_info()
    if not _active(world):
        return 0
    if arena is not None:
        from . import autograd
        autograd.join_side()                             # the gradients must be complete on this stream before they are reduced
    if arena is not None and arena.resident():
        dist.all_reduce(arena.flat, op=dist.ReduceOp.SUM)
        _count("all_reduce_grads", arena.flat)
        if average:
            arena.flat /= world
        return arena.flat.numel() * arena.flat.element_size()
    # parameters that do not require a gradient take no part (identically on every rank: requires_grad is model structure)
    params = [p for m in models for p in m.parameters() if p.requires_grad]
    if not params:
        return 0
    # one flat message: the gradients (zeros where this rank has none, so that every rank contributes the same count whatever
    # it rendered) followed by one flag per parameter -- after the sum a flag of zero means NO rank had a gradient for that
    # tensor, and it stays None as in a single process (an optimizer skips it; zero-filling would let Adam's moments or weight
    # decay move a parameter nobody differentiated)
    # The message is formed in the widest floating type among the parameters (f32 for the shipped models; f64 parameters -- the
    # CPU / gloo path, oracle-style double models -- are summed in f64 as a single process would); the flags are small integers,
    # exact in any of them.  (Reading the flags back is a host synchronisation: this path is the CPU / injected-renderer one;
    # the HIP path reduces the arena above, in place and graph-capturably.)
    wide = params[0].dtype
    for p in params[1:]:
        wide = torch.promote_types(wide, p.dtype)
    if not wide.is_floating_point:
        wide = torch.float32
    has = torch.tensor([0.0 if p.grad is None else 1.0 for p in params], dtype=wide, device=params[0].device)
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).to(wide) for p in params] + [has])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    _count("all_reduce_grads", flat)
    n_grad = flat.numel() - len(params)
    any_rank = flat[n_grad:].tolist()
    if average:
        flat[:n_grad] /= world
    o = 0
    for p, flag in zip(params, any_rank):
        n = p.numel()
        if flag > 0:
            if p.grad is None:
                p.grad = flat[o:o + n].view_as(p).to(p.dtype).clone()
            else:
                p.grad.copy_(flat[o:o + n].view_as(p.grad))
        o += n
    return n_grad * flat.element_size()


def data_parallel_backward(loss_local, models, n_local, n_global):
    """Ray-sharded training step: every rank rendered ``n_local`` of the ``n_global`` rays of the SAME
    batch and formed ``loss_local`` as a SUM over its rays of per-ray terms (e.g. ``((rgb - target)**2).sum()``).
    Scales it so that the all-reduced gradients equal those of the mean over the global batch, runs backward and
    sums the gradients over ranks in one bucket.  Batch-global losses (Hungarian cost, penalizer normalisers) need
    ``all_gather_cat`` of the small per-ray outputs first -- they are not a sum of per-ray terms."""
    del n_local
    (loss_local / float(n_global)).backward()
    return allreduce_grads(models)


class _GatherBatch(torch.autograd.Function):
    """Forward: the full batch tensor on every rank (one all-gather of the detached local slices).
    Backward: the gradient w.r.t. the full tensor is identical on every rank (the losses that consume it are
    evaluated redundantly); each rank keeps the rows of its own slice."""

    @staticmethod
    def forward(ctx, local, sizes):
        rank, world = world_info()
        ctx.s0, ctx.cnt = sum(sizes[:rank]), sizes[rank]
        return all_gather_cat(local.detach(), sizes)

    @staticmethod
    def backward(ctx, g):
        return g[ctx.s0:ctx.s0 + ctx.cnt].contiguous(), None


def gather_batch(local, sizes):
    """``[n_local, ...] -> [N, ...]`` on every rank, differentiable w.r.t. the local rows (the small
    per-ray outputs -- rgb ``[N,3]``, ins ``[N,ins_num]`` -- that batch-global losses need: ≈0.2 MB per step)."""
    rank, world = world_info()
    if not _active(world):
        return local
    return _GatherBatch.apply(local, list(sizes))


def allreduce_sums(t):
    """In-place sum over ranks of a small tensor of batch-global partial sums (the emptiness penalizer's mask
    normalisers, networks/penalizer.py:43,52).  No-op in a single process."""
    rank, world = world_info()
    if _active(world):
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        _count("all_reduce_sums", t)
    return t


def overlap_enabled(n_local, n_coarse, n_fine, device, cus=None):
    """Whether the step runs the two levels' network backwards on two streams (autograd.overlapped_backward).

    Worth it exactly when it removes a partial round: the data-gradient kernel runs one 128-sample workgroup per CU at a time, so
    the fine launch takes ceil(wg_fine / CUs) rounds and the coarse one ceil(wg_coarse / CUs) after it; side by side they take
    ceil((wg_fine + wg_coarse) / CUs).  At the 384-ray shard of an 8-way split: 576 + 192 workgroups on 256 CUs, 3 + 1 rounds
    against 3 (measured, profiles/r04: 3.88 -> 3.72 ms per step); at 512 / 3072 / 4096 rays both launches are whole rounds and two
    streams only add contention (+1 .. 2 %, same measurement), so they stay on one.  ``DMNERF_OVERLAP_BWD`` = 0 / 1 forces it."""
    env = os.environ.get("DMNERF_OVERLAP_BWD")
    if env is not None:
        return env != "0"
    if cus is None:
        if device.type != "cuda":
            return False
        cus = torch.cuda.get_device_properties(device).multi_processor_count
    wg_f, wg_c = -(-n_local * n_fine // 128), -(-n_local * n_coarse // 128)
    rounds = lambda w: -(-w // cus)
    return rounds(wg_f) + rounds(wg_c) > rounds(wg_f + wg_c)


def sharded_train_step(rays, z_vals, target, labels, models, args, optimizer, ins_num,
                       render=None, mse=None, criterion=None, penalizer=None, t_rand=None, u=None):
    """One optimisation step of train_dmsr.py:26-64 with the ray batch sharded over the ranks, producing the SAME
    update as a single process on the whole batch (BASELINE config 5):

    * every rank holds the same ``rays [2,N,3]``, ``z_vals [N,S]``, ``target [N,3]``, ``labels`` (the loaders draw the
      batch from a numpy stream that is seeded identically on every rank) and renders rows ``ray_slice(N)``;
      with ``args.perturb > 0`` the two jitter tensors are drawn FULL-size from the (identically seeded) device
      generator, in the reference's order (render.py:46, helpers.py:135), and sliced, so the jitter of ray i does not
      depend on the world size;
    * the per-ray outputs the batch-global losses need are all-gathered in ONE packed ``gather_batch`` (rgb and ins of both
      levels side by side, ≈0.2 MB):
      img2mse's mean and the Hungarian cost matrices / soft-IoU sums of ins_criterion (evaluator.py:19-74) are then
      evaluated identically on every rank, and autograd hands each rank the gradient rows of its own slice;
      ``args.N_ins`` (ScanNet: only the LAST N_ins rays carry labels, render.py:88-90) is applied to the gathered tensor;
    * with ``args.penalize`` (train_dmsr.py:51-58; off by default in config.py:86, on in every shipped train config) the
      emptiness penalizer is added: a ratio of batch sums, numerators and mask counts summed over ranks
      (``allreduce_sums``) before the division, inside the penalizer (``sharded=True``);
    * ``loss.backward()`` then yields on each rank the gradient contribution of its rays to the GLOBAL loss, one flat
      all-reduce (sum) of both models' gradients completes them, and every rank takes the same optimizer step.

    ``render / mse / criterion / penalizer`` default to the HIP path (networks.render.dm_nerf, evaluator.img2mse,
    evaluator.ins_criterion, penalizer.ins_penalizer); they are injectable so that the sharding logic itself is
    covered on CPU with gloo.  Returns the (global) loss and the number of bytes all-reduced.

    ``args.train_skip`` (a ``field.SkipGrid`` / ``field.TrainSkip``) needs nothing here: the default render reaches
    ``autograd.dm_nerf_train`` through ``args``, every rank selects within its own ray slice (one host read per skipped level
    and rank), a rank whose slice selects nothing contributes exact zeros, and the collectives are unchanged."""
    from .networks import evaluator as E, penalizer as P, render as R
    rank, world = world_info()
    multi = _active(world)                               # (a forced world of one takes every multi-rank branch below)
    arena = None
    render_is_hip = render is None
    if render is None and (multi or getattr(optimizer, "wants_arena", False)):                     # HIP path: backward writes both models' gradients into one buffer
        from . import autograd
        arena = autograd.grad_arena(models)
    N = rays.shape[1]
    sizes = [ray_slice(N, r, world)[1] for r in range(world)]
    s0, cnt = ray_slice(N, rank, world)
    sl = slice(s0, s0 + cnt)
    n_imp = int(args.N_importance)
    if float(args.perturb) > 0.:
        if t_rand is None:
            t_rand = torch.rand(z_vals.shape, device=z_vals.device)
        if u is None:
            u = torch.rand([N, n_imp], device=z_vals.device)
    import copy
    largs = copy.copy(args)
    n_ins = getattr(args, "N_ins", None)
    largs.N_ins = None                                   # the label slice is taken on the gathered batch
    render = render or (lambda r, z, a, tr, uu: R.dm_nerf(r, None, None, models[0], models[1], z, a, t_rand=tr, u=uu))
    local_rays = rays[:, sl].contiguous()                # (kept: the loss tail recognises the tensors the render was called with)
    out = render(local_rays, z_vals[sl].contiguous(), largs,
                 None if t_rand is None else t_rand[sl].contiguous(),
                 None if u is None else (u if u.dim() == 1 else u[sl].contiguous()))      # a 1-D u is the grid shared by all rays
    penalize = bool(getattr(args, "penalize", False))    # train_dmsr.py:51: the emptiness term is optional (--penalize)
    # ONE exchange for everything the batch-global losses need: rgb_fine | rgb_coarse | ins_fine | ins_coarse packed side by side
    # into [n_local, 6 + 2 * ins_num] and all-gathered once (160 B per ray at ins_num 13; at the 384-ray shard of an 8-rank step
    # four latency-bound collectives would cost more than the 61 KB they carry).  Packing and un-packing move values, not
    # arithmetic: the gathered columns are the same floats, and autograd routes each rank the rows of its own slice.
    levels = ("fine", "coarse")
    widths = [out['rgb_' + l].shape[-1] for l in levels] + [out['ins_' + l].shape[-1] for l in levels]
    if multi:
        packed = gather_batch(torch.cat([out['rgb_' + l] for l in levels] + [out['ins_' + l] for l in levels], -1), sizes)
        rgb_f, rgb_c, ins_f, ins_c = torch.split(packed, widths, -1)
    else:
        rgb_f, rgb_c, ins_f, ins_c = (out['rgb_fine'], out['rgb_coarse'], out['ins_fine'], out['ins_coarse'])
    if render_is_hip and mse is None and criterion is None and penalizer is None and os.environ.get("DMNERF_FUSED_TAIL", "1") != "0":
        # the HIP path's own loss tail: the same sum as the loop below as ONE autograd node (dm_nerf_amd/losses.py) -- the
        # object-code loss of both levels per launch, the scalar arithmetic in two kernels instead of some forty
        from . import losses
        if n_ins is not None:
            ins_f, ins_c = ins_f[-n_ins:], ins_c[-n_ins:]
        loss, _ = losses.train_losses(out, local_rays[1], target, labels, ins_num, largs, rgb_ins=(rgb_f, rgb_c, ins_f, ins_c),
                                      sharded=multi)
    else:
        mse = mse or E.img2mse
        criterion = criterion or (lambda pred, gt: E.ins_criterion(pred, gt, ins_num)[0])
        penalizer = penalizer or (lambda o, lvl, rays_d: P.ins_penalizer(o['raw_' + lvl], o['z_vals_' + lvl], o['depth_' + lvl],
                                                                         rays_d, largs, sharded=True))
        loss = 0.
        for lvl, rgb, ins in (("fine", rgb_f, ins_f), ("coarse", rgb_c, ins_c)):
            if n_ins is not None:
                ins = ins[-n_ins:]
            loss = loss + mse(rgb, target) + criterion(ins, labels)
            if penalize:
                loss = loss + penalizer(out, lvl, rays[1, sl]).sum()
    optimizer.zero_grad(set_to_none=True)
    if arena is not None:
        arena.begin_step()
    if render_is_hip:
        from . import autograd
        with autograd.overlapped_backward(overlap_enabled(cnt, z_vals.shape[1], z_vals.shape[1] + n_imp, rays.device)):   # coarse and fine network backwards side by side (two streams)
            loss.backward()
    else:
        loss.backward()
    nbytes = allreduce_grads(models, arena=arena)
    optimizer.step()
    return loss.detach(), nbytes


def _default_raygen(H, W, K, c2w, row0, nrows):
    from .networks import helpers
    return helpers.get_rays_k(H, W, K, c2w, row0=row0, nrows=nrows)


def _render_chunk(rays_o, rays_d, z, models, args, events=None, entry=None, **kw):
    """One chunk through the render entry ``entry`` with its keywords ``kw`` -> the three maps a frame keeps.  No entry: the frame
    keeps the fine level only (tester.py:71-77), so where the density-only coarse pass exists, the coarse heads are skipped."""
    from .networks import render
    fn = entry or render.fine_renderer(models[0], models[1], args)
    out = fn(torch.stack([rays_o, rays_d]), None, None, models[0], models[1], z, args, _events=events, **kw)
    return out['rgb_fine'], out['ins_fine'], out['depth_fine']


_compact_index_cache = {}


def _compact_index(sizes, mx, device):
    """Row index that drops the padding of a gathered ``[world * mx, ...]`` tensor whose rank r contributed ``sizes[r]`` rows."""
    key = (tuple(sizes), mx, str(device))
    if key not in _compact_index_cache:
        _compact_index_cache[key] = torch.cat([torch.arange(r * mx, r * mx + n) for r, n in enumerate(sizes)]).to(device)
    return _compact_index_cache[key]


def _gather_band(band, sizes, world, dev):
    """The frame from the ranks' packed bands: ONE all-gather of ``band [max(sizes), cols]`` (every rank allocates the largest
    band's size, so uneven bands gather without a padding copy), then one indexed row copy that drops the padding rows."""
    if not _active(world):
        return band
    full = all_gather_cat(band)
    if len(set(sizes)) != 1:
        full = full.index_select(0, _compact_index(sizes, max(sizes), dev))
    return full


class FrameRenderer:
    """One pose, rows sharded over the ranks: the per-pose body of ``render_test`` (networks/tester.py:58-85) as a resumable
    object -- ``step(i)`` renders chunk i of this rank's band into ONE packed band buffer
    ``[band rays, 3 + ins_num + 1]`` (rgb | ins | depth; ``labels_only``: ``[band rays, 6]`` = rgb | label | conf | depth, the
    label stored as an exactly representable float), ``gather()`` assembles the frame with ONE all-gather of that buffer.
    The buffer is allocated at the largest band's size, so ranks whose band is one row shorter (H not divisible by the world
    size) gather without a padding copy and the padding rows are dropped by one indexed row copy after the collective.
    ``render_frame`` is ``step`` over all chunks + ``gather``; bench.py drives the same object chunk by chunk."""

    def __init__(self, H, W, K, c2w, models, near, far, args, chunk=4096, n_samples=64,
                 raygen=None, render_chunk=None, z_fn=None, labels_only=False, label_conf=None, ins_num=None, dtype=None,
                 skip=None, skip_levels=("coarse", "fine"), mark=None, mark_threshold=0.0, mark_levels=("coarse", "fine")):
        self.rank, self.world = world_info()
        self.dtype = dtype                                         # band dtype (default f32, what every kernel writes)
        self.H, self.W, self.models, self.args, self.chunk = int(H), int(W), models, args, int(chunk)
        self.labels_only = bool(labels_only)
        self._pass_events = render_chunk is None
        if skip is not None:
            # skip = a field.SkipGrid: the chunks go through render.dm_nerf_fine_skip (samples in empty cells are not evaluated)
            if render_chunk is not None:
                raise ValueError("FrameRenderer: skip= routes the chunks through dm_nerf_fine_skip; it cannot be combined with render_chunk=")
            import functools

            from .networks import render
            render_chunk = functools.partial(_render_chunk, entry=render.dm_nerf_fine_skip, grid=skip, levels=skip_levels)
        if mark is not None:
            # mark = a field.SkipGrid: the chunks go through render.dm_nerf_fine_mark -- the dense render, which also sets in the grid
            # the cells of the samples it gave a weight > mark_threshold.  This rank marks the rows of its own band.
            if skip is not None:
                raise ValueError("FrameRenderer: mark= records what a DENSE render uses; it cannot be combined with skip=")
            if render_chunk is not None:
                raise ValueError("FrameRenderer: mark= routes the chunks through dm_nerf_fine_mark; it cannot be combined with render_chunk=")
            import functools

            from .networks import render
            render_chunk = functools.partial(_render_chunk, entry=render.dm_nerf_fine_mark, grid=mark, threshold=mark_threshold,
                                             levels=mark_levels)
        self.render_chunk = render_chunk or _render_chunk
        if z_fn is None:
            from .networks import helpers
            z_fn = lambda n, dev: helpers.z_val_sample(n, near, far, n_samples, device=dev)
        self.z_fn = z_fn
        if self.labels_only and label_conf is None:
            from .networks import evaluator
            label_conf = evaluator.ins_label_conf
        self.label_conf = label_conf
        row0, nrows = row_band(H, self.rank, self.world)
        ro, rd = (raygen or _default_raygen)(H, W, K, c2w, row0, nrows)
        self.rays_o, self.rays_d = ro.reshape(-1, 3), rd.reshape(-1, 3)
        self.n_local = self.rays_o.shape[0]
        self.sizes = [row_band(H, r, self.world)[1] * self.W for r in range(self.world)]
        self.dev = self.rays_o.device
        self.n_chunks = -(-self.n_local // self.chunk)
        self.z_full = self.z_fn(min(self.chunk, max(self.n_local, 1)), self.dev) if self.n_local else None
        # The packed band is sized HERE (object-code width from the model, f32 like every kernel output), not by the first rendered
        # chunk: a rank whose band has no rays (H < world size) never renders one, and must still enter the frame's all-gather with
        # a buffer of the common size -- raising on that rank alone would leave the others waiting in the collective.
        self.band = None
        if ins_num is None and models is not None:
            ins_num = getattr(models[-1], "ins_num", None)
        if ins_num is not None:
            self._alloc_band(int(ins_num), self.dtype or torch.float32)

    def _alloc_band(self, n_ins, dtype):
        self.n_ins = n_ins
        cols = 6 if self.labels_only else 3 + n_ins + 1
        self.band = torch.empty(max(max(self.sizes), 1), cols, dtype=dtype, device=self.dev)

    def step(self, i, events=None):
        """Render chunk ``i`` (0 .. n_chunks - 1; the last one may be ragged, tester.py:65-67) into the band."""
        s = i * self.chunk
        e = min(s + self.chunk, self.n_local)
        z = self.z_full if e - s == self.z_full.shape[0] else self.z_fn(e - s, self.dev)
        if self._pass_events:
            c_rgb, c_ins, c_depth = self.render_chunk(self.rays_o[s:e], self.rays_d[s:e], z, self.models, self.args, events=events)
        else:
            c_rgb, c_ins, c_depth = self.render_chunk(self.rays_o[s:e], self.rays_d[s:e], z, self.models, self.args)
        if self.band is None:
            self._alloc_band(c_ins.shape[-1], self.dtype or c_rgb.dtype)
        elif self.n_ins != c_ins.shape[-1]:
            # (a WIDTH the band was not sized for cannot be stored; every rank that renders sees the same renderer and raises the
            # same error.  A different DTYPE is converted by the assignments below instead -- ranks never disagree on the buffer.)
            if self.world > 1:
                raise RuntimeError(f"FrameRenderer: the chunk renderer returned object-code width {c_ins.shape[-1]}, the band was sized "
                                   f"for {self.n_ins} (pass ins_num= / a model with .ins_num matching the renderer)")
            self._alloc_band(c_ins.shape[-1], self.dtype or c_rgb.dtype)
        t = self.band[s:e]
        t[:, :3] = c_rgb
        if self.labels_only:
            label, conf = self.label_conf(c_ins)
            t[:, 3] = label.to(t.dtype)                            # (< 2^24: exact)
            t[:, 4] = conf
        else:
            t[:, 3:3 + self.n_ins] = c_ins
        t[:, -1] = c_depth
        return c_rgb, c_ins, c_depth

    def gather(self):
        """ONE all-gather of the packed band -> the frame's tensors on every rank."""
        H, W = self.H, self.W
        if self.band is None:                                      # no model width, no ins_num=, and no chunk rendered yet
            raise RuntimeError("FrameRenderer.gather(): the band was never sized -- render a chunk first or pass ins_num= "
                               "(required when a rank's band can be empty)")
        full = _gather_band(self.band, self.sizes, self.world, self.dev)
        rgb, depth = full[:, :3].reshape(H, W, 3), full[:, -1].reshape(H, W)
        if self.labels_only:
            return rgb, full[:, 3].to(torch.int64).reshape(H, W), full[:, 4].reshape(H, W), depth
        return rgb, full[:, 3:3 + self.n_ins].reshape(H, W, -1), depth


def render_frame(H, W, K, c2w, models, near, far, args, chunk=4096, n_samples=64,
                 raygen=None, render_chunk=None, z_fn=None, labels_only=False, label_conf=None, ins_num=None,
                 skip=None, skip_levels=("coarse", "fine"), mark=None, mark_threshold=0.0, mark_levels=("coarse", "fine")):
    """Full-frame render, rows sharded over ranks, ONE all-gather per frame (``FrameRenderer``).

    Mirrors the per-pose body of ``render_test`` (networks/tester.py:58-85): same chunking
    (``chunk`` = N_test rays, ragged last chunk), ``args.perturb`` is the caller's business
    (test scripts set it False, test_dmsr.py:86).  Returns ``rgb [H,W,3]``, ``ins [H,W,ins_num]``,
    ``depth [H,W]`` on every rank (views of the one gathered buffer).  ``labels_only=True``: the object map is reduced on the
    device to what ``ins_eval`` consumes (evaluator.py:127-137) -- ``label [H,W]`` int64 = argmax, ``conf [H,W]`` = max --
    before the gather, and ``(rgb, label, conf, depth)`` is returned: 24 instead of 16 + 4*ins_num bytes per pixel cross the links.
    ``skip=`` a ``field.SkipGrid``: every chunk is rendered by ``render.dm_nerf_fine_skip`` at ``skip_levels`` (opt-in; samples in
    empty cells are not evaluated).  ``render_path(..., skip=grid)`` hands it through.
    ``mark=`` a ``field.SkipGrid``: every chunk is rendered by ``render.dm_nerf_fine_mark`` -- the frame is the dense one, bit for bit
    -- and the cells of the samples whose weight is ``> mark_threshold`` at ``mark_levels`` are set in the grid, in place; each rank
    marks the rows of its own band (``field.SkipGrid.from_views`` combines the ranks).  Not with ``skip=`` or ``render_chunk=``
    (``ValueError``).  ``render_path(..., mark=grid)`` hands it through.
    """
    fr = FrameRenderer(H, W, K, c2w, models, near, far, args, chunk=chunk, n_samples=n_samples, raygen=raygen,
                       render_chunk=render_chunk, z_fn=z_fn, labels_only=labels_only, label_conf=label_conf, ins_num=ins_num,
                       skip=skip, skip_levels=skip_levels, mark=mark, mark_threshold=mark_threshold, mark_levels=mark_levels)
    for i in range(fr.n_chunks):
        fr.step(i)
    return fr.gather()


def render_path(render_poses, hwk, models, args, gt_imgs=None, crop_mask=None, labels_only=False, gt_labels=None,
                image_metrics=False, lpips=None, **frame_kw):
    """The pose loop of ``render_test`` (networks/tester.py:55-90) without its file output and CPU metrics: every pose of
    ``render_poses [P,3or4,4]`` through ``render_frame`` (rows sharded over the ranks, chunks of ``args.N_test`` rays),
    the ScanNet ``crop_mask`` applied as the reference applies it (:78-82: the pixels with mask 1, reshaped to
    ``args.crop_height x args.crop_width``), and, given ``gt_imgs [P,h,w,3]``, the per-pose PSNR on the device
    (data_range 1, what ``skimage.metrics.peak_signal_noise_ratio`` computes at :89).

    Returns a dict of stacked device tensors: ``rgb [P,h,w,3]``, ``depth [P,h,w]``, and either ``ins [P,h,w,ins_num]`` or,
    with ``labels_only=True``, ``label [P,h,w]`` (int64) and ``conf [P,h,w]``; ``psnr [P]`` when ``gt_imgs`` is given.

    Given ``gt_labels [P,h,w]`` (the per-pixel instance labels of the test set, in the frame's shape), also the instance AP of every
    pose as ``render_test`` scores it (tester.py:97-118 -> ``ins_eval``), on the device (``evaluator.ins_eval_device``): ``ap
    [P,6]`` (AP50, AP75, AP80, AP85, AP90, AP95), ``matched [P,ins_num]`` (the predicted label matched to each gt row; -1 unmatched
    and beyond the pose's row count: the data of ``matching_log.json``) and ``gt_num [P]``.  The rows are ``unique(gt_label)``, with
    ``crop_mask`` ``unique(gt_label)[:-1]`` and the mask ``gt_label < ins_num``, as in the two branches of the reference.  A pose
    without rows gets six APs of 1.0 (the reference appends ``tensor([1.0])`` there and fails later at tester.py:150).
    ``labels_only=True`` is the cheap way to it: the AP needs only the label and the confidence of each pixel.

    With ``image_metrics=True`` and ``gt_imgs``, also ``ssim [P]`` and ``psnr_f64 [P]`` (float64, on the device): the frame's
    ``structural_similarity(..., multichannel=True, data_range=1)`` and ``peak_signal_noise_ratio(..., data_range=1)`` as
    tester.py:89-90 computes them on a host copy (``evaluator.img_metrics_device``: one call for all poses after the loop, no
    synchronisation; the scored frame is the cropped one in the ``crop_mask`` branch and must be at least 7 x 7).  ``psnr`` keeps
    its float32 value.  The frames are complete on every rank, so every rank computes the same numbers; no collective is added.

    With ``lpips=`` an ``evaluator.LPIPSVGG`` and ``gt_imgs``, also ``lpips [P]`` (float64, on the device): tester.py:91's
    ``lpips.LPIPS(net="vgg")(rgb, gt)`` of the frame ``ssim`` scores (the cropped one in the ``crop_mask`` branch; at least
    16 x 16), one call for all poses after the loop, no synchronisation."""
    H, W, K = hwk
    chunk = int(getattr(args, "N_test", 4096))
    n_samples = int(getattr(args, "N_samples", 64))
    keep = None
    if crop_mask is not None:
        keep = torch.as_tensor(crop_mask).reshape(-1) == 1
        h, w = int(args.crop_height), int(args.crop_width)
    else:
        h, w = H, W
    cols = {}
    for i, c2w in enumerate(render_poses):
        frame = render_frame(H, W, K, c2w, models, args.near, args.far, args, chunk=chunk, n_samples=n_samples,
                             labels_only=labels_only, **frame_kw)
        names = ("rgb", "label", "conf", "depth") if labels_only else ("rgb", "ins", "depth")
        for name, t in zip(names, frame):
            flat = t.reshape(H * W, *t.shape[2:])
            if keep is not None:
                flat = flat[keep.to(flat.device)]
            cols.setdefault(name, []).append(flat.reshape(h, w, *t.shape[2:]))
        if gt_imgs is not None:
            gt = torch.as_tensor(gt_imgs[i]).to(cols["rgb"][-1])
            mse = torch.mean((cols["rgb"][-1] - gt) ** 2)
            cols.setdefault("psnr", []).append(-10.0 * torch.log10(mse))
        if gt_labels is not None:
            for name, t in zip(("ap", "matched", "gt_num"), _frame_ap(cols, gt_labels[i], crop_mask is not None, labels_only, args,
                                                                       frame_kw)):
                cols.setdefault(name, []).append(t)
    out = {k: torch.stack(v, 0) for k, v in cols.items()}
    if image_metrics and gt_imgs is not None and "rgb" in out:
        from .networks import evaluator
        gt = torch.stack([torch.as_tensor(gt_imgs[i]).to(out["rgb"]) for i in range(out["rgb"].shape[0])], 0)
        out["ssim"], out["psnr_f64"] = evaluator.img_metrics_device(out["rgb"], gt)
    if lpips is not None and gt_imgs is not None and "rgb" in out:
        gt = torch.stack([torch.as_tensor(gt_imgs[i]).to(out["rgb"]) for i in range(out["rgb"].shape[0])], 0)
        out["lpips"] = lpips(out["rgb"], gt)
    return out


def results_table(out, lpips=None):
    """The array ``render_test`` hands to ``np.savetxt`` as ``test_results.txt`` (networks/tester.py:149-157) from a
    ``render_path(..., gt_imgs=, gt_labels=, image_metrics=True)`` result: numpy float64 ``[P + 1, 9]`` with the columns PSNR, SSIM,
    LPIPS, AP50, AP75, AP80, AP85, AP90, AP95, one row per pose and the column means as the last row.  The LPIPS column is the
    caller's ``lpips [P]`` if given, else the result's own ``out["lpips"]`` (``render_path(..., lpips=model)``: an
    ``evaluator.LPIPSVGG`` with the weights the caller holds), else ``nan``.  The one host synchronisation of a whole test set."""
    import numpy as np
    for key in ("psnr_f64", "ssim", "ap"):
        if key not in out:
            raise ValueError(f"results_table: the result has no '{key}' (render_path(..., gt_imgs=, gt_labels=, image_metrics=True))")
    dev = torch.cat([out["psnr_f64"].double().reshape(-1, 1), out["ssim"].double().reshape(-1, 1), out["ap"].double()], 1)
    if dev.shape[1] != 8:
        raise ValueError(f"results_table: ap must be [P, 6], got {tuple(out['ap'].shape)}")
    own = lpips is None and "lpips" in out
    if own:                                             # (rides along in the one copy)
        dev = torch.cat([dev, out["lpips"].double().reshape(-1, 1).to(dev.device)], 1)
    host = dev.cpu().numpy()                            # the one sync
    P = host.shape[0]
    if own:
        lp, host = host[:, 8], host[:, :8]
    elif lpips is None:
        lp = np.full(P, np.nan)
    else:
        lp = np.asarray(lpips.detach().cpu() if isinstance(lpips, torch.Tensor) else lpips, dtype=np.float64).reshape(-1)
    if lp.shape[0] != P:
        raise ValueError(f"results_table: {lp.shape[0]} LPIPS values for {P} poses")
    rows = np.concatenate([host[:, :2], lp[:, None], host[:, 2:]], 1)
    return np.concatenate([rows, rows.mean(0, keepdims=True)], 0)


def _frame_ap(cols, gt_label, crop, labels_only, args, frame_kw):
    """One pose's ``(ap [6], matched [ins_num], gt_num)`` for render_path: the rows and the mask of tester.py:97-118, then
    ``ins_eval_device``."""
    from .networks import evaluator
    if labels_only:
        label, conf = cols["label"][-1].contiguous(), cols["conf"][-1].contiguous()   # (views of the frame's packed output without a crop)
        ins_num = frame_kw.get("ins_num") or getattr(args, "ins_num", None)
        if ins_num is None:
            raise ValueError("render_path(gt_labels=...): pass ins_num= or set args.ins_num")
    else:
        label, conf = evaluator.ins_label_conf(cols["ins"][-1])
        ins_num = cols["ins"][-1].shape[-1]
    ins_num = int(ins_num)
    gl = torch.as_tensor(gt_label).to(device=label.device, dtype=torch.int64).reshape(label.shape)
    rows = torch.unique(gl)
    mask = None
    if crop:
        rows = rows[:-1]
        mask = (gl < ins_num).to(torch.float32)
    n = int(rows.numel())
    if n == 0:
        return (torch.ones(6, dtype=torch.float32, device=label.device), torch.full((ins_num,), -1, dtype=torch.int64, device=label.device),
                torch.tensor(0, dtype=torch.int64, device=label.device))
    _, ap, matched = evaluator.ins_eval_device(label, conf, gl, rows, ins_num, mask)
    return ap, matched, torch.tensor(n, dtype=torch.int64, device=label.device)


def _matmul4_f32(a, b):
    """``a @ b`` for two 4 x 4 f32 matrices with a FIXED evaluation order: products and sums rounded to f32 one at a time,
    k = 0..3 in sequence.  The reference forms ``trans @ ori_pose`` with ``torch.matmul`` on the host (manipulator.py:235), whose
    BLAS kernel -- and with it the last bit of the result -- depends on the CPU model; this one gives the same target pose on
    every host (within 1 ulp per entry of whatever the reference's host computes)."""
    import numpy as np
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    out = np.zeros((4, 4), dtype=np.float32)
    for k in range(4):
        out = (out + (a[:, k:k + 1] * b[k:k + 1, :]).astype(np.float32)).astype(np.float32)
    return torch.from_numpy(out)


def _default_manipulate_chunk(ori_rays, tar_rays, models, args, us):
    from .networks import manipulator as Mn
    return Mn.manipulator(None, None, models[0], models[1], ori_rays, tar_rays, args, us=us, kinds=getattr(args, "edit_kinds", None),
                          keep_labels=getattr(args, "keep_labels", None))


def _skip_manipulate_chunk(ori_rays, tar_rays, models, args, us, grid=None, levels=("coarse", "fine"), counts=None):
    from .networks import manipulator as Mn
    return Mn.manipulator(None, None, models[0], models[1], ori_rays, tar_rays, args, us=us, kinds=getattr(args, "edit_kinds", None),
                          keep_labels=getattr(args, "keep_labels", None), skip=grid, skip_levels=levels, skip_counts=counts)


def _field_edit_chunk(ori_rays, tar_rays, models, args, us, edit=None, counts=None):
    """The chunk of a ``field_edit=`` frame: ``manipulator.edited_field`` with the FIRST of the chunk's draws; no target side (zeros)."""
    from .networks import manipulator as Mn
    rgb, ins, _ = Mn.edited_field(models[0], models[1], ori_rays, args, edit, u=us[0], counts=counts)
    return rgb, ins, torch.zeros_like(rgb), torch.zeros_like(ins)


def _default_draws(n, n_imp, count, device):
    return [torch.rand([n, n_imp], device=device) for _ in range(count)]


def _default_target_rays(H, W, K, poses, kinds, offsets, row0, nrows):
    from . import editing
    return editing.edit_rays(H, W, K, poses, kinds, offsets, row0=row0, nrows=nrows)


def _target_rays_from(raygen):
    """``target_rays`` built on an injected ``raygen`` (CPU / gloo tests): the rays of each pose, a deformed object's origin x
    plus its row's offset as the reference forms it (manipulator.py:428: f32 column + f64 tensor, rounded once).  The rows are
    the band's ABSOLUTE image rows."""
    def target_rays(H, W, K, poses, kinds, offsets, row0, nrows):
        tars = []
        for t, (pose, kind) in enumerate(zip(poses, kinds)):
            to, td = raygen(H, W, K, pose, row0, nrows)
            to, td = to.reshape(-1, 3).clone(), td.reshape(-1, 3)
            if kind:
                off = torch.from_numpy(offsets[t, row0:row0 + nrows].copy()).to(to.device).repeat_interleave(int(W))
                to[:, 0] = to[:, 0] + off
            tars.append(torch.stack([to, td]))
        return torch.stack(tars)
    return target_rays


class ManipulationFrameRenderer:
    """One pose of the manipulation render, rows sharded over the ranks: the per-pose body of ``manipulator_eval``
    (networks/manipulator.py:232-270) -- original rays of ``ori_pose``, target rays of ``trans @ ori_pose``, the chunk loop around
    ``manipulator()`` (:137-205) and its four O(chunks^2) ``torch.cat`` accumulations -- as a resumable object (BASELINE config 5).

    * rank r owns a contiguous band of image rows and generates the original AND the ``T = len(trans_list)`` target rays of that
      band itself (raygen kernel, no scatter; the reference evaluates one transformation per call, ``trans_list`` generalises it
      the way ``manipulator()``'s ``f_tar_rays`` list does).  An entry of ``trans_list`` may also be an ``editing.Deform``
      (``manipulator_demo``'s deformations, :397-429): that object's target rays are the ORIGINAL pose's with the origin's x shifted
      by a per-image-row offset.  With any ``Deform`` present all target rays come from ONE launch of ``dmnerf_edit_rays``, the
      offset table indexed by the absolute image row; with matrices only nothing changes;
    * the chunks are those of the WHOLE frame -- ``[c N_test, (c + 1) N_test)``, ragged last chunk (:241-244) -- and a rank renders
      the part of each chunk that falls into its band.  ``step(c)`` makes, on EVERY rank, the ``2 + T`` draws
      ``torch.rand([chunk rays, N_importance])`` that ``manipulator()`` makes for chunk c in a single process (it resamples with
      ``det=False`` even at evaluation, :148,:170,:187), in the reference's order, and uses the rows of its own part: the device
      generator advances identically on all ranks, and **the assembled frame is bit-identical whatever the world size**
      (tests/test_gpu_manipulator_frame.py) -- which a per-rank chunking of the band could not be;
    * each part's four outputs go into ONE packed band ``[band rays, 2 (3 + C)]`` = ``final_rgb | final_ins | tar_rgb | tar_ins``
      (C = ins_num + 1: the manipulation render keeps the last object channel, :101-102), and ``gather()`` is ONE all-gather per
      frame.

    * an entry may also be an ``editing.Remove()`` or an ``editing.Copy(matrix)``, and ``keep_labels`` isolates a set of objects
      (``networks.manipulator.edit_exchanger``).  A removal has no target rays and no draws: ``T`` counts the entries WITH rays,
      ``step`` draws ``2 + T``, and the kinds and the keep set travel to ``manipulate_chunk`` as ``args.edit_kinds`` (one per entry of
      ``trans_list``) and ``args.keep_labels``.  Without target rays the ``tar_rgb | tar_ins`` columns of the band are zero.  With
      ``keep_labels`` ``trans_list`` may be empty.

    ``manipulate_chunk(ori_rays [2,n,3], tar_rays [T,2,n,3], models, args, us)``, ``raygen`` / ``draws`` and
    ``target_rays(H, W, K, poses, kinds, offsets [T,H] float64, row0, nrows) -> [T,2,n,3]`` are injectable
    (CPU / gloo tests of the sharding logic); ``rank=`` / ``world=`` override the process group's view for the band arithmetic
    (a single process can then render band r of N, without collectives).

    ``skip=`` a ``field.SkipGrid`` (opt-in): the default chunk function hands it to ``manipulator(skip=, skip_levels=)``, which does
    not evaluate samples in empty cells and writes the empty row there.  The draws do not depend on the grid, so the assembled frame
    stays bit-identical whatever the world size.  ``self.n_eval``: int64 ``[2]`` on the device, the samples evaluated and the samples
    in all over the steps this rank rendered (zeros without ``skip=``); it never reaches the host.  ``skip=`` cannot be combined with
    an injected ``manipulate_chunk=``.

    ``field_edit=`` an ``editing.FieldEdit`` (opt-in): the frame is the FIELD-EDIT render -- every chunk goes through
    ``manipulator.edited_field``, the trained field seen through the edited volume with one network evaluation per sample (two sparse
    launches per chunk for any number of edits; a render with its own contract).  The edits live in the ``FieldEdit``:
    ``trans_list`` must be empty, ``T = 0``, and it cannot be combined with ``skip=``, ``keep_labels=`` or ``manipulate_chunk=``
    (``ValueError``).  ``step`` still makes its usual two draws per chunk on every rank and the route uses the first, so the frame stays
    bit-identical whatever the world size; the ``tar_rgb | tar_ins`` columns of the band are zero; ``n_eval`` counts the samples
    evaluated and the samples in all."""

    def __init__(self, H, W, K, ori_pose, trans_list, models, args, chunk=None, raygen=None, manipulate_chunk=None, draws=None,
                 ins_num=None, rank=None, world=None, dtype=torch.float32, target_rays=None, keep_labels=None, skip=None,
                 skip_levels=("coarse", "fine"), field_edit=None):
        r_, w_ = world_info()
        self.rank, self.world = (r_ if rank is None else int(rank)), (w_ if world is None else int(world))
        self._collective = rank is None and world is None
        self.H, self.W, self.models = int(H), int(W), models
        self.chunk = int(chunk if chunk is not None else getattr(args, "N_test", 4096))
        import copy
        self.args = copy.copy(args)
        if not hasattr(self.args, "target_labels"):                 # manipulator.py:229
            self.args.target_labels = [self.args.target_label] if len(trans_list) else []
        self.n_imp = int(self.args.N_importance)
        if skip is not None and manipulate_chunk is not None:
            raise ValueError("ManipulationFrameRenderer: skip= routes the chunks through manipulator(skip=); it cannot be combined "
                             "with manipulate_chunk=")
        if field_edit is not None:
            from .editing import FieldEdit
            who = "ManipulationFrameRenderer: field_edit="
            if not isinstance(field_edit, FieldEdit):
                raise TypeError(f"{who} must be an editing.FieldEdit")
            if len(trans_list):
                raise ValueError(f"{who} carries the edits itself (FieldEdit.from_volume(grid, trans_list, ...)); trans_list must be empty")
            if skip is not None or manipulate_chunk is not None or keep_labels is not None:
                raise ValueError(f"{who} routes the chunks through manipulator.edited_field; it cannot be combined with skip=, "
                                 "manipulate_chunk= or keep_labels= (the keep set is the FieldEdit's)")
            self.args.target_labels = []
        self._skip = None
        if skip is not None:
            from .networks import render
            self._skip = (skip, render.check_skip_levels("ManipulationFrameRenderer", skip_levels))
        self.manipulate_chunk = manipulate_chunk or _default_manipulate_chunk
        self.draws = draws or _default_draws
        from .editing import Copy, Deform, check_edit_lengths, edit_kind
        kinds = [edit_kind(trans) for trans in trans_list]
        if len(kinds) == 0 and keep_labels is None and field_edit is None:
            raise ValueError("ManipulationFrameRenderer: at least one transformation")
        if any(kinds) or keep_labels is not None:                   # removals, copies, a keep set: manipulator()'s edit path
            check_edit_lengths("ManipulationFrameRenderer", len(kinds), len(self.args.target_labels))
            self.args.edit_kinds = kinds
            self.args.keep_labels = None if keep_labels is None else [int(l) for l in keep_labels]
        # only MOVE and COPY entries have target rays (and draws): a removal reads no target
        trans_list = [trans.matrix if isinstance(trans, Copy) else trans for trans, k in zip(trans_list, kinds) if k != 2]
        deform = [isinstance(trans, Deform) for trans in trans_list]
        self.T = len(deform)
        if target_rays is None and any(deform):
            target_rays = _target_rays_from(raygen) if raygen is not None else _default_target_rays
        raygen = raygen or _default_raygen
        row0, nrows = row_band(H, self.rank, self.world)
        pose = torch.as_tensor(ori_pose, dtype=torch.float32)
        dev_pose = pose.device
        pose_h = pose.detach().cpu()
        if pose_h.shape[0] == 3:                                    # [3,4] pose: the homogeneous row the 4 x 4 product needs
            pose_h = torch.cat([pose_h, torch.tensor([[0., 0., 0., 1.]])], 0)
        ro, rd = raygen(H, W, K, pose.to(dev_pose), row0, nrows)
        self.ori = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)])                      # [2, band, 3]
        # a rigid object's pose is trans @ ori_pose (manipulator.py:235, :432), a deformed object's the original pose (:427-429)
        tar_poses = [pose_h if d else _matmul4_f32(torch.as_tensor(trans, dtype=torch.float32).cpu(), pose_h)
                     for d, trans in zip(deform, trans_list)]
        if self.T == 0:
            self.tar = torch.zeros(0, 2, self.ori.shape[1], 3, dtype=self.ori.dtype, device=self.ori.device)
        elif target_rays is not None:
            import numpy as np
            offsets = np.zeros((self.T, self.H), dtype=np.float64)
            for t, trans in enumerate(trans_list):
                if deform[t]:
                    offsets[t] = trans.offsets(self.H)
            self.tar = target_rays(self.H, self.W, K, [p.to(dev_pose) for p in tar_poses], [int(d) for d in deform], offsets, row0, nrows)
        else:
            tars = []
            for tar_pose in tar_poses:
                to, td = raygen(H, W, K, tar_pose.to(dev_pose), row0, nrows)
                tars.append(torch.stack([to.reshape(-1, 3), td.reshape(-1, 3)]))
            self.tar = torch.stack(tars)                                                    # [T, 2, band, 3]
        self.dev = self.ori.device
        self.start = row0 * self.W                                                          # first frame ray of this band
        self.n_local = self.ori.shape[1]
        self.sizes = [row_band(H, r, self.world)[1] * self.W for r in range(self.world)]
        self.n_chunks = -(-(self.H * self.W) // self.chunk)
        if ins_num is None and models is not None:
            ins_num = getattr(models[-1], "ins_num", None)
        if ins_num is None:
            raise ValueError("ManipulationFrameRenderer: pass ins_num= (no model with .ins_num given)")
        self.C = int(ins_num) + 1
        self.band = torch.empty(max(max(self.sizes), 1), 2 * (3 + self.C), dtype=dtype, device=self.dev)
        self.n_eval = torch.zeros(2, dtype=torch.int64, device=self.dev)
        if self._skip is not None:
            import functools
            self.manipulate_chunk = functools.partial(_skip_manipulate_chunk, grid=self._skip[0], levels=self._skip[1], counts=self.n_eval)
        if field_edit is not None:
            import functools
            self.manipulate_chunk = functools.partial(_field_edit_chunk, edit=field_edit, counts=self.n_eval)

    def owned(self, c):
        """Rows of the band that chunk ``c`` of the frame covers: (first, last + 1) in band coordinates; empty if first >= last."""
        a = max(c * self.chunk, self.start) - self.start
        b = min(min((c + 1) * self.chunk, self.H * self.W), self.start + self.n_local) - self.start
        return a, b

    def step(self, c):
        """Chunk ``c`` of the frame: the ``2 + T`` draws on every rank, the render of this rank's part of it (if any)."""
        s = c * self.chunk
        n = min(self.chunk, self.H * self.W - s)
        us = self.draws(n, self.n_imp, 2 + self.T, self.dev)
        a, b = self.owned(c)
        if b <= a:
            return None
        off = self.start + a - s                                    # this part's first row inside the chunk's draws
        us = [u[off:off + (b - a)].contiguous() for u in us]
        out = self.manipulate_chunk(self.ori[:, a:b].contiguous(), self.tar[:, :, a:b].contiguous(), self.models, self.args, us)
        t, C = self.band[a:b], self.C
        t[:, 0:3], t[:, 3:3 + C], t[:, 3 + C:6 + C], t[:, 6 + C:6 + 2 * C] = out
        return out

    def gather(self):
        """ONE all-gather of the packed band -> ``final_rgb [H,W,3], final_ins [H,W,C], tar_rgb [H,W,3], tar_ins [H,W,C]``."""
        full = _gather_band(self.band, self.sizes, self.world, self.dev) if self._collective else self.band[:self.n_local]
        rows = self.H if self._collective else self.n_local // self.W
        C = self.C
        return (full[:, 0:3].reshape(rows, self.W, 3), full[:, 3:3 + C].reshape(rows, self.W, C),
                full[:, 3 + C:6 + C].reshape(rows, self.W, 3), full[:, 6 + C:6 + 2 * C].reshape(rows, self.W, C))


def manipulate_frame(H, W, K, ori_pose, trans_list, models, args, **kw):
    """One manipulated pose, rows sharded over the ranks, ONE all-gather (``ManipulationFrameRenderer``): what the chunk loop of
    ``manipulator_eval`` (networks/manipulator.py:232-270) leaves in ``full_rgb, full_ins, full_tar_rgb, full_tar_ins``, reshaped
    ``[H, W, .]`` as :273-274 does.  ``args``: N_samples, N_importance, near, far, N_test, target_labels (or target_label)."""
    fr = ManipulationFrameRenderer(H, W, K, ori_pose, trans_list, models, args, **kw)
    for c in range(fr.n_chunks):
        fr.step(c)
    return fr.gather()
