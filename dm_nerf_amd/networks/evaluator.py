"""Mirror of the loss side of ``networks/evaluator.py`` that sits in the training step of the reference
(train_dmsr.py:33-47): ``img2mse``, ``mse2psnr`` and the Hungarian-matched object-code loss ``ins_criterion``.

``ins_criterion`` runs entirely on the GPU stream (csrc/criterion.hip): the reference moves the cost matrix to the
host for ``scipy.optimize.linear_sum_assignment`` and syncs twice per step.  The metrics half of
the file runs on the device too: the per-pixel label / confidence every rendered frame needs (``ins_label_conf``) and the
instance AP of a frame (``ins_eval``, ``ins_eval_device``: csrc/ins_eval.hip).  ``calculate_ap`` on its own has no device
version: the AP integral is the last step of the ``ins_eval`` kernel, which works on counts, not on an IoU vector.
The two image scores of ``render_test`` that the reference takes from ``skimage.metrics`` on a host copy of the frame
(tester.py:89-90) are ``img_metrics_device`` / ``ssim`` / ``psnr`` (csrc/img_metrics.hip), and the third, ``lpips.LPIPS(net="vgg")``
(tester.py:43,91), is ``LPIPSVGG`` / ``lpips`` (csrc/conv3x3.hip, csrc/lpips.hip) with weights the caller hands over.
"""
import torch

from .. import _lib

img2mse = lambda x, y: torch.mean((x - y) ** 2)                                             # evaluator.py:11
mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.tensor([10.], device=x.device))  # evaluator.py:15


class _InsCriterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, labels, ins_num):
        lib = _lib.load()
        N = pred.shape[0]
        nbytes = lib.dmnerf_ins_criterion_work_bytes(N, ins_num)
        if nbytes < 0:
            raise ValueError(f"ins_criterion: unsupported N={N} ins_num={ins_num} (ins_num <= 128)")
        work = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        out = torch.empty(4, dtype=torch.float32, device=pred.device)
        _lib.launch("dmnerf_ins_criterion_fwd", pred, labels, N, ins_num, work, nbytes, out)
        ctx.save_for_backward(pred, labels, work)
        ctx.ins_num = ins_num
        ctx.mark_non_differentiable(work)
        ctx.set_materialize_grads(False)                 # (no zero-filled "gradient" for the work buffer)
        return out, work

    @staticmethod
    def backward(ctx, g_out, _g_work=None):
        if g_out is None:
            return None, None, None
        pred, labels, work = ctx.saved_tensors
        grad = torch.empty_like(pred)
        g = _lib.f32(g_out)
        _lib.launch("dmnerf_ins_criterion_bwd", pred, labels, pred.shape[0], ctx.ins_num, work, g, grad)
        return grad, None, None


CRIT_TOO_MANY_LABELS, CRIT_LABEL_RANGE = 1, 2          # DMNERF_CRIT_* (include/dmnerf_hip.h)


def ins_criterion(pred_ins, gt_labels, ins_num, check=None):
    """``ins_criterion`` (networks/evaluator.py:19-37): ``pred_ins [N, ins_num]``, ``gt_labels [N]`` ->
    ``(ins_loss_sum, valid_ce, invalid_ce, valid_siou)`` as 0-dim tensors, differentiable w.r.t. ``pred_ins``.

    Same definition as the reference: rows of the cost matrices are the labels that occur (ascending), matched to
    channels by a minimum-cost assignment of ``cost_ce + cost_siou``; ``invalid_ce`` is the mean prediction of the
    unmatched channels (0 when every channel is matched, where the reference returns ``tensor([0])``).
    No host synchronisation -- which is also why two conditions on which the reference RAISES cannot raise here by
    default: more distinct labels than ``ins_num`` channels (the first ``ins_num`` are kept) and labels outside
    ``[0, ins_num]`` (they join no row).  The kernels record both in a flags word; ``check=True`` (or the environment
    variable ``DMNERF_CHECK_LABELS=1``; default off) reads it back -- one sync -- and raises ``ValueError`` like the reference.
    """
    pred = _lib.f32(pred_ins)
    _lib.require_gpu(pred)
    if pred.dim() != 2 or pred.shape[1] != int(ins_num):
        raise ValueError("ins_criterion: pred_ins must be [N, ins_num]")
    labels = gt_labels.reshape(-1).to(device=pred.device, dtype=torch.int32).contiguous()
    if labels.shape[0] != pred.shape[0]:
        raise ValueError("ins_criterion: one label per ray")
    out, work = _InsCriterion.apply(pred, labels, int(ins_num))
    if check is None:
        import os
        check = os.environ.get("DMNERF_CHECK_LABELS", "0") == "1"
    if check:
        off = _lib.load().dmnerf_ins_criterion_flags_offset(pred.shape[0], int(ins_num))
        flags = int(work[off:off + 4].view(torch.int32).item())
        if flags & CRIT_TOO_MANY_LABELS:
            raise ValueError(f"ins_criterion: more than ins_num={ins_num} distinct labels in the batch (evaluator.py:21-25 raises too)")
        if flags & CRIT_LABEL_RANGE:
            raise ValueError(f"ins_criterion: a label lies outside [0, {ins_num}]")
    return out[0], out[1], out[2], out[3]


def ins_label_conf(pred_ins):
    """The first two lines of ``ins_eval`` (networks/evaluator.py:127-137): ``pred_label = argmax(pred_ins, -1)`` (int64,
    first maximum) and ``pred_conf_mask = max(pred_ins, -1)`` for ``pred_ins [..., ins_num]``, on the device."""
    x = _lib.f32(pred_ins)
    _lib.require_gpu(x)
    C = x.shape[-1]
    flat = x.reshape(-1, C)
    label = torch.empty(flat.shape[0], dtype=torch.int64, device=x.device)
    conf = torch.empty(flat.shape[0], dtype=torch.float32, device=x.device)
    _lib.launch("dmnerf_ins_label_conf", flat, flat.shape[0], C, label, conf)
    return label.reshape(x.shape[:-1]), conf.reshape(x.shape[:-1])


IE_LABEL_RANGE, IE_GT_NOT_ONEHOT = 1, 2               # DMNERF_IE_* (include/dmnerf_hip.h)
THRESHOLDS = (0.5, 0.75, 0.8, 0.85, 0.9, 0.95)        # evaluator.py:10


def _rows_view(t):
    """``t [..., K]`` as (tensor, number of rows, row stride in elements) without a copy when its rows are evenly spaced with a
    unit inner stride (a channel slice such as ``ins[..., :-1]``); otherwise a contiguous f32 copy (plumbing)."""
    if t.dtype != torch.float32:
        t = t.float()
    lead = t.shape[:-1]
    n = 1
    for s in lead:
        n *= int(s)
    if t.dim() >= 2 and t.stride(-1) == 1:
        rs = t.stride(-2)
        expect, ok = rs, True
        for d in range(t.dim() - 2, -1, -1):           # every leading dim must step by (inner rows) x row stride
            if t.shape[d] != 1 and t.stride(d) != expect:
                ok = False
                break
            expect *= int(t.shape[d])
        if ok and rs >= t.shape[-1]:
            return t, n, rs
    t = t.contiguous()
    return t, n, t.shape[-1]


def _ins_eval_run(N, ins_num, gt_num, masked, device, prep_args):
    lib = _lib.load()
    nbytes = lib.dmnerf_ins_eval_work_bytes(N, ins_num)
    if nbytes < 0:
        raise ValueError(f"ins_eval: unsupported N={N} ins_num={ins_num} (ins_num <= 128)")
    if not 0 <= gt_num <= ins_num:
        raise ValueError(f"ins_eval: gt_num={gt_num} must lie in [0, ins_num={ins_num}]")
    work = torch.empty(nbytes, dtype=torch.uint8, device=device)
    label = torch.empty(N, dtype=torch.int64, device=device)
    ap = torch.empty(6, dtype=torch.float32, device=device)
    matched = torch.empty(ins_num, dtype=torch.int64, device=device)
    args = prep_args(label)
    _lib.launch("dmnerf_ins_eval_prep", *args, gt_num, N, ins_num, work, nbytes)
    _lib.launch("dmnerf_ins_eval", N, ins_num, gt_num, 1 if masked else 0, work, nbytes, ap, matched)
    return label, ap, matched, work


def ins_eval_device(pred_label, pred_conf, gt_label, gt_rows, ins_num, mask=None):
    """``ins_eval`` (networks/evaluator.py:125-175) of one frame from its per-pixel ``pred_label`` (int, argmax over the object
    channels, in ``[0, ins_num)``) and ``pred_conf`` (the max) -- e.g. ``render_frame(..., labels_only=True)``'s output -- and the
    ground truth as per-pixel labels ``gt_label`` with ``gt_rows`` (int64 ``[gt_num]``, ascending): the labels that form the rows,
    the reference's ``valid_gt_labels``.  No host synchronisation, no allocation outside the returned tensors; capturable.

    Returns device tensors ``(pred_label, ap [6], matched [ins_num])``: the labels with the mask rule applied (``ins_num`` where
    ``mask == 0``), the six APs (float32) and the matched predicted label of each gt row (``return_labels``; -1 for an unmatched
    row and beyond ``gt_num``).  Where the reference raises because no predicted label is valid, every row is unmatched and the
    APs are 0."""
    _lib.require_gpu(pred_label, pred_conf, gt_label, gt_rows, mask)
    ins_num = int(ins_num)
    shape = pred_label.shape
    lab = pred_label.reshape(-1).to(torch.int64).contiguous()
    conf = _lib.f32(pred_conf).reshape(-1)
    gl = gt_label.reshape(-1).to(torch.int64).contiguous()
    rows = gt_rows.reshape(-1).to(torch.int64).contiguous()
    m = None if mask is None else _lib.f32(mask).reshape(-1)
    N = lab.shape[0]
    if conf.shape[0] != N or gl.shape[0] != N or (m is not None and m.shape[0] != N):
        raise ValueError("ins_eval_device: pred_label, pred_conf, gt_label (and mask) must have one entry per pixel")
    label, ap, matched, _ = _ins_eval_run(
        N, ins_num, rows.shape[0], m is not None, lab.device,
        lambda out: (None, 0, lab, conf, out, m, None, 0, gl, rows))
    return label.reshape(shape), ap, matched


def ins_eval(pred_ins, gt_ins, gt_ins_num, ins_num, mask=None, check=None):
    """``ins_eval(pred_ins, gt_ins, gt_ins_num, ins_num, mask)`` (networks/evaluator.py:125-175) on the device: ``pred_ins
    [H, W, ins_num]`` (f32; rows may be strided, e.g. ``ins[..., :-1]``), the one-hot ``gt_ins [H, W, ins_num]`` (columns
    ``< gt_ins_num``), the optional ``mask [H, W]``.  Returns ``(pred_label [H, W] int64 device tensor, ap: six floats,
    return_labels: int64 numpy array [gt_ins_num], -1 for an unmatched row)`` -- one host synchronisation, for the returned values.

    The counts behind the reference's ``[ins_num, ins_num, H W]`` broadcasts are formed in one pass over the frame; the
    assignment is the criterion's solver (scipy's algorithm).  ``check=True`` raises ``ValueError`` when a pixel's
    ``gt_ins[:gt_ins_num]`` is not one-hot (0 / 1 with at most one 1).  Where the reference raises because no predicted label is
    valid, every row is unmatched and the APs are 0."""
    for t in (pred_ins, gt_ins):
        if not t.is_cuda:
            _lib.require_gpu(t)                         # raises: no CPU fallback
    _lib.require_gpu(mask)
    p, N, ps = _rows_view(pred_ins)
    g, Ng, gs = _rows_view(gt_ins)
    ins_num, gt_num = int(ins_num), int(gt_ins_num)
    if p.shape[-1] != ins_num or Ng != N:
        raise ValueError("ins_eval: pred_ins must be [..., ins_num] and gt_ins one row per pixel")
    if g.shape[-1] < gt_num:
        raise ValueError("ins_eval: gt_ins has fewer than gt_ins_num columns")
    m = None if mask is None else _lib.f32(mask).reshape(-1)
    if m is not None and m.shape[0] != N:
        raise ValueError("ins_eval: one mask entry per pixel")
    label, ap, matched, work = _ins_eval_run(
        N, ins_num, gt_num, m is not None, p.device,
        lambda out: (p, ps, None, None, out, m, g, gs, None, None))
    off = _lib.load().dmnerf_ins_eval_flags_offset(N, ins_num)
    host = torch.cat([ap.double(), matched[:gt_num].double(), work[off:off + 4].view(torch.int32).double()]).cpu()   # the one sync
    flags = int(host[-1])
    if check and flags & IE_GT_NOT_ONEHOT:
        raise ValueError(f"ins_eval: gt_ins[..., :{gt_num}] is not one-hot")
    return label.reshape(pred_ins.shape[:-1]), [float(v) for v in host[:6]], host[6:6 + gt_num].numpy().astype("int64")


def _img_metrics_run(pred, gt, with_channels=False):
    """``dmnerf_img_metrics`` on ``pred, gt [P,H,W,C]``: ``(ssim [P], psnr [P], mse [P], ssim_ch [P,C] or None)``, f64 on the device."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"img_metrics: {name} must be a device tensor (there is no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"img_metrics: {name} must be float32, got {t.dtype}")
    if pred.shape != gt.shape or pred.dim() != 4 or pred.device != gt.device:
        raise ValueError(f"img_metrics: pred and gt must share one [P,H,W,C] or [H,W,C] shape and device, got {tuple(pred.shape)} and "
                         f"{tuple(gt.shape)}")
    P, H, W, C = (int(s) for s in pred.shape)
    if H < 7 or W < 7:
        raise ValueError(f"img_metrics: win_size 7 exceeds the image extent {H} x {W}")
    lib = _lib.load()
    nbytes = lib.dmnerf_img_metrics_work_bytes(P, H, W, C)
    if nbytes < 0:
        raise ValueError(f"img_metrics: unsupported P={P} H={H} W={W} C={C} (C in 1..4, H, W <= 32768)")
    pred, gt = pred.contiguous(), gt.contiguous()       # (the crop of render_path is a view)
    dev = pred.device
    work = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    out = torch.empty(3, P, dtype=torch.float64, device=dev)
    ch = torch.empty(P, C, dtype=torch.float64, device=dev) if with_channels else None
    _lib.launch("dmnerf_img_metrics", pred, gt, P, H, W, C, work, nbytes, out[0], ch, out[1], out[2])
    return out[0], out[2], out[1], ch


def img_metrics_device(pred, gt):
    """SSIM and PSNR of rendered frames as ``render_test`` scores them (networks/tester.py:89-90: ``skimage.metrics``'
    ``structural_similarity(rgb, gt, multichannel=True, data_range=1)`` and ``peak_signal_noise_ratio(rgb, gt, data_range=1)``) on
    the device (csrc/img_metrics.hip; float64 throughout, 7x7 uniform windows wholly inside the image, sample covariance).

    ``pred, gt``: float32 device tensors ``[P,H,W,C]`` or ``[H,W,C]``, ``C`` in 1..4, ``H, W >= 7``; views are made contiguous.
    Returns ``(ssim, psnr)``: float64 device tensors ``[P]``, or 0-d for the 3-d form.  No host synchronisation; capturable;
    bit-identical from run to run and independent of ``P``.  What ``manipulate_frame`` returns goes in as it is."""
    single = isinstance(pred, torch.Tensor) and pred.dim() == 3
    if single and isinstance(gt, torch.Tensor) and gt.dim() == 3:
        pred, gt = pred[None], gt[None]
    ssim_, psnr_, _, _ = _img_metrics_run(pred, gt)
    return (ssim_[0], psnr_[0]) if single else (ssim_, psnr_)


def ssim(pred, gt):
    """``structural_similarity(pred, gt, multichannel=True, data_range=1)`` of one ``[H,W,C]`` frame (tester.py:90) as a Python
    float: ``img_metrics_device`` plus one synchronisation."""
    if pred.dim() != 3:
        raise ValueError("ssim: one [H,W,C] frame")
    return float(img_metrics_device(pred, gt)[0])


def psnr(pred, gt):
    """``peak_signal_noise_ratio(pred, gt, data_range=1)`` of one ``[H,W,C]`` frame (tester.py:89) as a Python float (``inf`` for
    identical frames): ``img_metrics_device`` plus one synchronisation."""
    if pred.dim() != 3:
        raise ValueError("psnr: one [H,W,C] frame")
    return float(img_metrics_device(pred, gt)[1])


# ---- LPIPS (VGG16): lpips.LPIPS(net="vgg") of tester.py:43,91 and manipulator.py:216,280 ------------------------------------------
# (index in torchvision's vgg16().features, slice of lpips' wrapper, Cin, Cout); a 2x2 max-pool precedes each slice but the first,
# and each slice's last ReLU is tapped.
LPIPS_VGG_CONVS = ((0, 1, 3, 64), (2, 1, 64, 64), (5, 2, 64, 128), (7, 2, 128, 128), (10, 3, 128, 256), (12, 3, 256, 256),
                   (14, 3, 256, 256), (17, 4, 256, 512), (19, 4, 512, 512), (21, 4, 512, 512), (24, 5, 512, 512), (26, 5, 512, 512),
                   (28, 5, 512, 512))
LPIPS_VGG_TAPS = (64, 128, 256, 512, 512)
LPIPS_MIN_SIZE = 16


def lpips_parse_state_dicts(vgg_sd, lin_sd, conv_key):
    """The 13 ``(weight [Cout,Cin,3,3], bias [Cout])`` pairs and the 5 ``lin`` weights (``[1,C,1,1]``) out of the mappings, shapes
    checked: ``ValueError`` naming the key that is missing or misshapen.  ``conv_key(idx, slice, 'weight' | 'bias')`` names a
    convolution's entry.  Needs no device and no library."""
    convs, lins = [], []
    for idx, sl, cin, cout in LPIPS_VGG_CONVS:
        pair = []
        for kind, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = conv_key(idx, sl, kind)
            if key not in vgg_sd:
                raise ValueError(f"LPIPSVGG: state dict has no '{key}'")
            t = vgg_sd[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f"LPIPSVGG: '{key}' must be a tensor of shape {shape}, got {tuple(getattr(t, 'shape', ()))}")
            pair.append((key, t))
        convs.append(tuple(pair))
    for k, c in enumerate(LPIPS_VGG_TAPS):
        key = f"lin{k}.model.1.weight"
        if key not in lin_sd:
            raise ValueError(f"LPIPSVGG: state dict has no '{key}'")
        t = lin_sd[key]
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (1, c, 1, 1):
            raise ValueError(f"LPIPSVGG: '{key}' must be a tensor of shape {(1, c, 1, 1)}, got {tuple(getattr(t, 'shape', ()))}")
        lins.append((key, t))
    return convs, lins


def lpips_parse_state_dict(sd):
    """``lpips.LPIPS(net='vgg').state_dict()``'s form: ``net.slice{1..5}.{idx}.{weight,bias}`` and ``lin{0..4}.model.1.weight``; the
    ``lins.{k}...`` duplicates and ``scaling_layer.*`` are ignored."""
    return lpips_parse_state_dicts(sd, sd, lambda idx, sl, kind: f"net.slice{sl}.{idx}.{kind}")


def lpips_parse_torchvision(vgg_sd, lin_sd):
    """torchvision's ``vgg16().state_dict()`` (``features.{idx}.{weight,bias}``; the classifier is ignored) plus the ``lin`` weights."""
    return lpips_parse_state_dicts(vgg_sd, lin_sd, lambda idx, sl, kind: f"features.{idx}.{kind}")


def _pf_rows(n, h, w):
    """Rows of a padded-flat buffer of ``n`` images ``h x w`` (include/dmnerf_hip.h): bordered images plus the two guards."""
    return n * (h + 2) * (w + 2) + 2 * (w + 3)


def conv3x3_pack(weight):
    """``dmnerf_conv3x3_pack``: a ``[Cout,Cin,3,3]`` float32 device tensor as the kernel's ``[Cout][9 Cin -> 32]`` matrix."""
    cout, cin = int(weight.shape[0]), int(weight.shape[1])
    ldb = (9 * cin + 31) // 32 * 32
    w = weight.detach().contiguous()
    out = torch.empty(cout, ldb, dtype=torch.float32, device=w.device)
    _lib.launch("dmnerf_conv3x3_pack", w, cout, cin, out, ldb)
    return out


def padded_flat(x):
    """``x [N,H,W,C]`` as a padded-flat buffer ``[rows, C]`` (a host-side helper for tests and timing: plain torch copies)."""
    n, h, w, c = x.shape
    buf = torch.zeros(_pf_rows(n, h, w), c, dtype=x.dtype, device=x.device)
    buf[w + 3:w + 3 + n * (h + 2) * (w + 2)].view(n, h + 2, w + 2, c)[:, 1:-1, 1:-1] = x
    return buf


def padded_flat_images(buf, n, h, w):
    """The ``[N,H+2,W+2,C]`` view (borders included) of a padded-flat buffer."""
    return buf[w + 3:w + 3 + n * (h + 2) * (w + 2)].view(n, h + 2, w + 2, buf.shape[1])


def conv3x3(x_pf, packed, bias, n, h, w, relu=True, out=None):
    """``dmnerf_conv3x3`` (taps = 9) on a padded-flat ``[rows, Cin]`` buffer of ``n`` images ``h x w``: the padded-flat
    ``[rows, Cout]`` output, borders and guards exactly zero."""
    cin, cout = int(x_pf.shape[1]), int(packed.shape[0])
    if out is None:
        out = torch.empty(_pf_rows(n, h, w), cout, dtype=torch.float32, device=x_pf.device)
    _lib.launch("dmnerf_conv3x3", x_pf, x_pf.numel(), packed, packed.numel(), bias, out, out.numel(), n, h, w, cin, cout, 9, 1 if relu else 0)
    return out


def maxpool2(x_pf, n, h, w):
    """``dmnerf_maxpool2``: padded-flat ``n`` images ``h x w`` -> padded-flat ``h // 2 x w // 2``."""
    c = int(x_pf.shape[1])
    out = torch.empty(_pf_rows(n, h // 2, w // 2), c, dtype=torch.float32, device=x_pf.device)
    _lib.launch("dmnerf_maxpool2", x_pf, x_pf.numel(), out, out.numel(), n, h, w, c)
    return out


class LPIPSVGG:
    """``lpips.LPIPS(net="vgg")`` (lpips 0.1.4, version 0.1, ``spatial=False``) on the device, with weights the caller already holds:

        model = LPIPSVGG.from_state_dict(their_lpips_module.state_dict())        # or from_state_dicts(vgg16_sd, lin_sd)
        d = model(pred, gt)                                                      # [P,H,W,3] or [H,W,3] float32 device tensors

    Nothing here constructs ``lpips.LPIPS`` or a torchvision model (those constructors fetch weights).  The thirteen convolutions are
    csrc/conv3x3.hip, the scaling layer, pooling and the tail csrc/lpips.hip.  Weights are packed once at construction; the
    workspace is cached per ``(P, H, W)``.  The result is float64 ``[P]`` (0-d for one frame), with no host synchronisation; the
    call is capturable once its workspace exists, bit-identical from run to run and independent of ``P``."""

    def __init__(self, convs, lins):
        dev = None
        for pair in list(convs) + [(l,) for l in lins]:
            for key, t in pair:
                if not t.is_cuda:
                    raise ValueError(f"LPIPSVGG: '{key}' must be a device tensor (there is no CPU path)")
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise ValueError(f"LPIPSVGG: '{key}' is on {t.device}, other weights on {dev}")
        self.device = dev
        with torch.cuda.device(dev):
            self.packed = [conv3x3_pack(w.detach().float()) for (_, w), _ in convs]
            self.bias = [b.detach().float().contiguous().clone() for _, (_, b) in convs]
            self.lin = [t.detach().float().reshape(-1).contiguous().clone() for _, t in lins]
        self._work = {}

    @classmethod
    def from_state_dict(cls, sd):
        return cls(*lpips_parse_state_dict(sd))

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd):
        return cls(*lpips_parse_torchvision(vgg_sd, lin_sd))

    def _workspace(self, P, H, W):
        key = (P, H, W)
        ws = self._work.get(key)
        if ws is None:
            lib = _lib.load()
            nbytes = lib.dmnerf_lpips_work_bytes(P, H, W)
            if nbytes < 0:
                raise ValueError(f"LPIPSVGG: unsupported P={P} H={H} W={W} (H, W in {LPIPS_MIN_SIZE} .. 4096)")
            al = lambda b: (b + 255) // 256 * 256
            m = 2 * P * (H + 2) * (W + 2)
            n_taps, n_act = m * 32, _pf_rows(2 * P, H, W) * 64
            n_part = P * ((H * W + 255) // 256)
            assert al(4 * n_taps) + 2 * al(4 * n_act) + al(8 * n_part) == nbytes, "workspace layout out of step with dmnerf_lpips_work_bytes"
            raw = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            o1 = al(4 * n_taps)
            o2 = o1 + al(4 * n_act)
            o3 = o2 + al(4 * n_act)
            ws = dict(raw=raw, taps=raw[:4 * n_taps].view(torch.float32), a=raw[o1:o1 + 4 * n_act].view(torch.float32),
                      b=raw[o2:o2 + 4 * n_act].view(torch.float32), part=raw[o3:o3 + 8 * n_part].view(torch.float64))
            self._work[key] = ws
        return ws

    def __call__(self, pred, gt, normalize=False, features=None):
        """``pred, gt``: ``[P,H,W,3]`` or ``[H,W,3]`` float32 device tensors, ``H, W >= 16`` -- what ``render_path`` and
        ``manipulate_frame`` return.  ``normalize``: the library's flag (``2 x - 1`` first; the reference passes ``[0,1]`` frames
        without it).  ``features``: a list that receives the five tapped feature maps ``[2P,h,w,C]`` (pred then gt) as copies -- a
        debug output for the tests."""
        for name, t in (("pred", pred), ("gt", gt)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"LPIPSVGG: {name} must be a device tensor (there is no CPU path)")
            if t.dtype != torch.float32:
                raise ValueError(f"LPIPSVGG: {name} must be float32, got {t.dtype}")
        single = pred.dim() == 3 and gt.dim() == 3
        if single:
            pred, gt = pred[None], gt[None]
        if pred.shape != gt.shape or pred.dim() != 4 or pred.device != gt.device or pred.shape[-1] != 3:
            raise ValueError(f"LPIPSVGG: pred and gt must share one [P,H,W,3] or [H,W,3] shape and device, got {tuple(pred.shape)} and "
                             f"{tuple(gt.shape)}")
        if pred.device != self.device:
            raise ValueError(f"LPIPSVGG: frames on {pred.device}, weights on {self.device}")
        P, H, W, _ = (int(s) for s in pred.shape)
        if H < LPIPS_MIN_SIZE or W < LPIPS_MIN_SIZE:
            raise ValueError(f"LPIPSVGG: frames of {H} x {W} are below the {LPIPS_MIN_SIZE} x {LPIPS_MIN_SIZE} the five levels need")
        out = torch.empty(P, dtype=torch.float64, device=self.device)
        if P == 0:
            return out
        ws = self._workspace(P, H, W)
        pred, gt = pred.contiguous(), gt.contiguous()       # (the crop of render_path is a view)
        N = 2 * P
        _lib.launch("dmnerf_lpips_prologue", pred, gt, P, H, W, 1 if normalize else 0, ws["taps"], ws["taps"].numel())
        src, dst = ws["taps"], ws["a"]
        other = ws["b"]
        h, w, level = H, W, 0
        for i, (idx, sl, cin, cout) in enumerate(LPIPS_VGG_CONVS):
            if i > 0 and sl != LPIPS_VGG_CONVS[i - 1][1]:     # the pool in front of slices 2 .. 5
                _lib.launch("dmnerf_maxpool2", src, src.numel(), dst, dst.numel(), N, h, w, cin)
                h, w = h // 2, w // 2
                src, dst = dst, src
            first = i == 0
            _lib.launch("dmnerf_conv3x3", src, src.numel(), self.packed[i], self.packed[i].numel(), self.bias[i], dst, dst.numel(), N, h, w,
                        32 if first else cin, cout, 1 if first else 9, 1)
            if first:
                src, dst = dst, other
            else:
                src, dst = dst, src
            if i + 1 == len(LPIPS_VGG_CONVS) or LPIPS_VGG_CONVS[i + 1][1] != sl:      # the slice's last ReLU: a tap
                _lib.launch("dmnerf_lpips_tail", src, src.numel(), self.lin[level], P, h, w, cout, 1 if level == 0 else 0, ws["part"],
                            ws["part"].numel(), out)
                if features is not None:
                    features.append(padded_flat_images(src[:_pf_rows(N, h, w) * cout].view(-1, cout), N, h, w)[:, 1:-1, 1:-1].clone())
                level += 1
        return out[0] if single else out


def lpips(model, pred, gt):
    """``float(lpips.LPIPS(net="vgg")(pred, gt))`` of one ``[H,W,3]`` frame (tester.py:91) as a Python float: ``model(pred, gt)``
    plus one synchronisation."""
    if pred.dim() != 3:
        raise ValueError("lpips: one [H,W,3] frame")
    return float(model(pred, gt))
