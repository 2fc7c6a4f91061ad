"""Scene editing on the device: the two manipulation drivers of the reference's ``networks/manipulator.py`` around
``manipulator()`` -- ``manipulator_demo`` (:367-491) and ``manipulator_eval`` (:208-364) -- without their file output.

    :381-382, :397-429   the per-image-row deformation of an object's target rays    ->  ``deform_offsets``, ``Deform``, ``edit_rays``
    :384-488             the demo's pose loop: one edit per object per view           ->  ``manipulate_demo_path``
    :233-339             the evaluation's pose loop with PSNR / SSIM / AP             ->  ``manipulate_eval_path``
    :472-488, :310-323   8-bit frame, label, label mask, coloured object image        ->  ``frame_products``, ``label_lut``
    (extension)          remove, duplicate, isolate: entries next to matrices / ``Deform``  ->  ``Remove``, ``Copy``, ``keep_labels=``
    (extension)          the edit applied to a label / baked volume itself, with collision counts  ->  ``edit_volume``
    tools/pose_generator.py:67-77   a matrix about a centre; the centre from a ``field.LabelGrid``  ->  ``about``, ``object_centre``

The frames are rendered by ``distributed.ManipulationFrameRenderer`` (rows sharded over the ranks, one all-gather per frame); the
products are computed from the gathered frame's packed buffer in place (csrc/edit_frame.hip), so 7 bytes per pixel leave the
device instead of the ``4 (3 + C)`` of the float maps the reference copies to the host.  Writing PNG files stays with the caller.
"""
import copy
import ctypes

import numpy as np
import torch

from . import _lib
from . import distributed as D

DEFORM_FUNCS = ("sin", "ex", "linear", "abs_linear", "ln")
# manipulator.py:381-382
DEFORM_V = np.concatenate((np.linspace(0, 0.18, 2), np.linspace(0.18, 0, 2), np.linspace(0, -0.18, 2), np.linspace(-0.18, 0, 2)))


def deform_offsets(H, func, view_index):
    """The x offset of every image row for a deformed object, numpy float64 ``[H]``: ``v_1`` of manipulator.py:398-426 before
    its ``np.repeat`` over the columns, computed on the host with numpy exactly as there (the constants of the reference's
    400-pixel frames are kept literally), so the values are the reference's bit for bit.  ``sin`` scales by
    ``deform_v[view_index]`` (:381-382, eight views; a larger index raises ``IndexError`` as in the reference)."""
    v = np.linspace(1, int(H), int(H))
    if func == "sin":
        v = ((8 * np.pi) / 400) * v
        return np.sin(v) * DEFORM_V[view_index]
    if func == "ex":
        return np.exp(-1 * v / 50)
    if func == "linear":
        return (v - 200) / 215
    if func == "abs_linear":
        return np.abs(v - 200) / 200
    if func == "ln":
        return np.log(v / 200)
    raise ValueError(f"deform_offsets: unknown deformation '{func}' (one of {', '.join(DEFORM_FUNCS)})")


class Deform:
    """A deformation as an entry of ``ManipulationFrameRenderer``'s ``trans_list``, next to 4 x 4 matrices: the object's target
    rays are the ORIGINAL pose's rays with the origin's x shifted by ``deform_offsets(H, func, view_index)[row]``."""
    __slots__ = ("func", "view_index")

    def __init__(self, func, view_index=0):
        if func not in DEFORM_FUNCS:
            raise ValueError(f"Deform: unknown deformation '{func}' (one of {', '.join(DEFORM_FUNCS)})")
        self.func, self.view_index = func, int(view_index)

    def offsets(self, H):
        return deform_offsets(H, self.func, self.view_index)

    def __repr__(self):
        return f"Deform({self.func!r}, {self.view_index})"

    def __eq__(self, other):
        return isinstance(other, Deform) and (self.func, self.view_index) == (other.func, other.view_index)

    def __hash__(self):
        return hash((self.func, self.view_index))


class Remove:
    """Removal of an object as an entry of ``trans_list``: its samples are zeroed in the original rays' field
    (``networks.manipulator.REMOVE``).  It has no target rays, makes no draws and adds no samples to the merged depths."""
    __slots__ = ()

    def __repr__(self):
        return "Remove()"

    def __eq__(self, other):
        return isinstance(other, Remove)

    def __hash__(self):
        return hash(Remove)


class Copy:
    """Duplication of an object as an entry of ``trans_list``: the object also appears where ``matrix`` (4 x 4, as for a move)
    puts it, and stays where it is (``networks.manipulator.COPY``).  ``matrix`` may be a ``Deform``: the duplicate's target rays
    are then the deformed ones -- the rays of an entry and what the exchange does with them are independent."""
    __slots__ = ("matrix",)

    def __init__(self, matrix):
        if isinstance(matrix, (Remove, Copy)):
            raise ValueError(f"Copy: cannot wrap {matrix!r} (a 4 x 4 matrix or a Deform)")
        if not isinstance(matrix, Deform) and tuple(np.shape(matrix)) != (4, 4):
            raise ValueError(f"Copy: the transformation must be 4 x 4 or a Deform, got shape {tuple(np.shape(matrix))}")
        self.matrix = matrix

    def __repr__(self):
        return f"Copy({self.matrix!r})"


def edit_kind(trans):
    """The exchange kind of a ``trans_list`` entry: ``networks.manipulator.MOVE`` / ``COPY`` / ``REMOVE``."""
    return 2 if isinstance(trans, Remove) else 1 if isinstance(trans, Copy) else 0


def about(matrix, centre):
    """``matrix`` (4 x 4: a rotation, a scale, any product of them) applied about ``centre [3]`` instead of the origin -> the float64
    4 x 4 ``T(centre) @ matrix @ T(-centre)``, a ``trans_list`` entry.  The arithmetic of tools/pose_generator.py:67-77: the two
    translations are float32 ``np.eye`` matrices (the centre is rounded to f32 once), the product is float64."""
    matrix = np.asarray(matrix, dtype=np.float64)
    centre = np.asarray(centre, dtype=np.float64).reshape(-1)
    if matrix.shape != (4, 4) or centre.shape != (3,):
        raise ValueError(f"about: expected a 4 x 4 matrix and a centre [3], got {matrix.shape} and {centre.shape}")
    translation = np.eye(4, 4, dtype=np.float32)
    translation[:3, -1] = -1 * centre
    translation_inverse = np.eye(4, 4, dtype=np.float32)
    translation_inverse[:3, -1] = -1 * translation[:3, -1]
    return translation_inverse @ matrix @ translation


def object_centre(label_grid_or_stats, label):
    """The centre of object ``label`` -> numpy float64 ``[3]``: row ``label`` of ``stats()["centre"]`` of a ``field.LabelGrid`` (or of
    the dict ``stats()`` returned), the mean of the centres of the cells the object owns.  This is the one host read of the label
    grid: one copy of four numbers.  ``ValueError`` if the object owns no cell or ``label`` is not a row of the stats.  The mean is
    over ALL cells of the label, so stray cells pull it: ``object_centre(grid.cleaned(keep="largest")[0], label)`` is the robust
    pivot, the centre of the object's largest connected component (``field.LabelGrid.cleaned``)."""
    stats = label_grid_or_stats if isinstance(label_grid_or_stats, dict) else label_grid_or_stats.stats()
    label = int(label)
    if not 0 <= label < stats["count"].shape[0]:
        raise ValueError(f"object_centre: label {label} outside [0, {stats['count'].shape[0]})")
    row = torch.cat([stats["count"][label].double().reshape(1), stats["centre"][label]]).cpu().numpy()
    if row[0] == 0:
        raise ValueError(f"object_centre: object {label} owns no cell of the label grid")
    return row[1:].astype(np.float64)


def edit_rays(H, W, K, poses, kinds, offsets=None, row0=0, nrows=None, device=None):
    """Target rays of ``T`` edited objects for image rows ``[row0, row0 + nrows)`` in one launch (``dmnerf_edit_rays``) ->
    ``[T, 2, nrows W, 3]``, what ``manipulator()`` takes as ``f_tar_rays``.  ``poses``: T c2w ``[3or4, 4]`` (read on the host),
    ``kinds [T]``: 0 rigid (``get_rays_k`` of the pose, bit for bit) or 1 deform (origin x + ``offsets[t][absolute row]``, summed
    in float64 and rounded once); ``offsets``: numpy float64 ``[T, H]`` or a device tensor of that shape (needed with a deform)."""
    H, W, row0 = int(H), int(W), int(row0)
    nrows = H - row0 if nrows is None else int(nrows)
    T = len(poses)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    K = np.asarray(K)
    intr = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[2, 2]], dtype=np.float64).astype(np.float32)
    c = np.ascontiguousarray(np.stack([(p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)).astype(np.float32)[:3, :4]
                                       for p in poses])) if T else np.zeros((0, 3, 4), np.float32)
    kind = (ctypes.c_int * max(T, 1))(*[int(k) for k in kinds])
    off = None
    if offsets is not None:
        off = offsets if torch.is_tensor(offsets) else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.float64))
        off = off.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(off.shape) != (T, H):
            raise ValueError(f"edit_rays: offsets must be [T={T}, H={H}], got {tuple(off.shape)}")
    rays = torch.empty(T, 2, nrows * W, 3, dtype=torch.float32, device=dev)
    _lib.launch("dmnerf_edit_rays", H, W, intr, c, kind, T, off, row0, nrows, rays)
    return rays


def label_lut(C, rgbs, color_dict, ins_map, device=None):
    """The table of ``render_label2img`` (tools/visualizer.py:73-86) for labels ``0 .. C - 1`` -> uint8 ``[C, 3]`` on the device:
    ``rgbs[color_dict[str(ins_map[str(l)])]]``, 0 where ``ins_map`` has no ``l`` (``field.color_table``, the rule of
    ``field.label_colors``)."""
    from . import field
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(field.color_table(int(C), rgbs, color_dict, ins_map)).to(dev)


def frame_products(rgb, ins=None, lut=None):
    """What the drivers write out for a frame (manipulator.py:472-488), on the device (``dmnerf_edit_products``):

    ``rgb [..., 3]`` -> ``rgb8`` uint8 ``[..., 3]`` = ``to8b`` (evaluator.py:13); ``ins [..., C]`` -> ``label`` int64 ``[...]`` =
    ``torch.argmax(ins, -1)`` over ALL channels (first maximum) and ``mask`` uint8 = that label; ``lut`` uint8 ``[C, 3]``
    (``label_lut``) -> ``ins_img`` uint8 ``[..., 3]`` = ``lut[label]``.  Returns ``(rgb8, label, mask, ins_img)``; what has no
    input is ``None``.  Channel-slice views of a packed frame -- what ``manipulate_frame`` returns -- are read in place."""
    from .networks import evaluator
    _lib.require_gpu(lut)
    for t in (rgb, ins):
        if t is not None and not t.is_cuda:
            _lib.require_gpu(t)                         # raises: no CPU fallback
    if rgb.shape[-1] != 3:
        raise ValueError(f"frame_products: rgb must be [..., 3], got {tuple(rgb.shape)}")
    lead = rgb.shape[:-1]
    r, n, rs = evaluator._rows_view(rgb)
    dev = r.device
    rgb8 = torch.empty(*lead, 3, dtype=torch.uint8, device=dev)
    x, xs, C, label, mask, ins_img = None, 0, 0, None, None, None
    if ins is not None:
        if ins.shape[:-1] != lead:
            raise ValueError(f"frame_products: ins {tuple(ins.shape)} does not match rgb {tuple(rgb.shape)}")
        x, _, xs = evaluator._rows_view(ins)
        C = int(x.shape[-1])
        label = torch.empty(*lead, dtype=torch.int64, device=dev)
        mask = torch.empty(*lead, dtype=torch.uint8, device=dev)
        if lut is not None:
            if lut.dtype != torch.uint8 or tuple(lut.shape) != (C, 3):
                raise ValueError(f"frame_products: lut must be uint8 [{C}, 3], got {lut.dtype} {tuple(lut.shape)}")
            ins_img = torch.empty(*lead, 3, dtype=torch.uint8, device=dev)
    _lib.launch("dmnerf_edit_products", r, rs, x, xs, C, lut, n, rgb8, label, mask, ins_img)
    return rgb8, label, mask, ins_img


# ---- the label volume seen from a camera (csrc/label_trace.hip): an object from a pixel, an edit before it is rendered
def pick(label_grid, H, W, K, pose, pixels, near, far, labels=None):
    """The object under each pixel of ``pixels`` (an iterable of ``(col, row)``) -> numpy ``label [P]`` uint8, ``t [P]`` f32, ``point
    [P, 3]`` float64, ``cell [P, 3]`` int64: the first labelled cell of ``label_grid`` (a ``field.LabelGrid``) along the pixel's
    ``get_rays_k`` ray (``dmnerf_raygen_select``), restricted to ``labels`` (as in ``LabelGrid.trace``).  ``point = o + d t`` in
    float64, ``cell = (i, j, k)``; a pixel that hits nothing gets label 255, ``t = inf``, a non-finite ``point`` and ``cell = -1``.
    One host read at the end (eleven numbers per pixel)."""
    from .networks import helpers
    H, W = int(H), int(W)
    pixels = [(int(c), int(r)) for c, r in pixels]
    for c, r in pixels:
        if not (0 <= c < W and 0 <= r < H):
            raise ValueError(f"pick: pixel (col {c}, row {r}) outside the {W} x {H} frame")
    P = len(pixels)
    dev = label_grid.labels.device
    intr, c2w = helpers._camera(K, pose)
    idx = torch.tensor([r * W + c for c, r in pixels], dtype=torch.int64).to(dev)
    rays = torch.empty(2, P, 3, dtype=torch.float32, device=dev)
    if P:
        _lib.launch("dmnerf_raygen_select", H, W, intr, c2w, idx, P, rays[0], rays[1])
    out = label_grid.trace(rays[0], rays[1], near, far, labels)
    host = torch.cat([out["label"].double()[:, None], out["t"].double()[:, None], out["cell"].double()[:, None], rays[0].double(),
                      rays[1].double()], dim=1).cpu().numpy()                     # the one host read; every value is exact in float64
    label, t, g = host[:, 0].astype(np.uint8), host[:, 1].astype(np.float32), host[:, 2].astype(np.int64)
    with np.errstate(invalid="ignore"):
        point = host[:, 3:6] + host[:, 6:9] * host[:, 1:2]
    _, dy, dz = label_grid.dims
    cell = np.where(g[:, None] >= 0, np.stack([g // (dy * dz), (g // dz) % dy, g % dz], axis=1), -1)
    return label, t, point, cell


def edit_label_sets(C, target_labels, kinds, keep_labels=None):
    """The exchanger's per-sample rule as label sets -> ``(own, per_entry)``: ``own`` = what the original rays / a cell's own content
    may show, every kept label but those of MOVE and REMOVE entries (not where they were); ``per_entry[e]`` = what entry ``e`` may show,
    its own label if kept -- nothing for a REMOVE, which shows nothing anywhere."""
    allowed = set(range(C)) if keep_labels is None else {int(l) for l in keep_labels}
    gone = {int(l) for l, k in zip(target_labels, kinds) if k != 1}
    return sorted(allowed - gone), [[int(l)] if (k != 2 and int(l) in allowed) else [] for l, k in zip(target_labels, kinds)]


def check_edit_lengths(who, n_edits, n_labels):
    """One target label per edit, or ``ValueError`` in ``who``'s name."""
    if n_edits != n_labels:
        raise ValueError(f"{who}: {n_labels} target labels for {n_edits} edits")


class EditList:
    """One edit list, normalised and checked in ``who``'s name before anything touches a device: ``trans_list`` / ``target_labels`` of
    equal lengths, at most ``max_edits`` entries (``too_many`` ends that sentence), every target label and every label of
    ``keep_labels`` in ``[0, C)`` (``C = None``: the caller has checks of its own to make first and calls ``check_labels(C)`` after
    them).  Holds ``trans_list``, ``target_labels`` (ints), ``kinds`` (``edit_kind`` per entry), ``keep`` (the sorted keep set, or
    ``None``), ``E`` and ``C``."""

    def __init__(self, who, trans_list, target_labels, C, keep_labels=None, max_edits=None, too_many=""):
        self.who, self.C = who, None
        self.trans_list, self.target_labels = list(trans_list), [int(l) for l in target_labels]
        self.E = len(self.trans_list)
        check_edit_lengths(who, self.E, len(self.target_labels))
        if max_edits is not None and self.E > max_edits:
            raise ValueError(f"{who}: {self.E} edits, at most {max_edits}{too_many}")
        self.keep = None if keep_labels is None else sorted({int(l) for l in keep_labels})
        self.kinds = [edit_kind(trans) for trans in self.trans_list]
        if C is not None:
            self.check_labels(C)

    def check_labels(self, C):
        """Every target label and every kept label lies in ``[0, C)``; sets ``C``."""
        for l in self.target_labels + (self.keep or []):
            if not 0 <= l < C:
                raise ValueError(f"{self.who}: label {l} outside [0, {C})")
        self.C = C

    def label_sets(self):
        """``edit_label_sets`` of this list -> ``(own, per_entry)``."""
        return edit_label_sets(self.C, self.target_labels, self.kinds, self.keep)

    def entries(self, what_for):
        """``pack_entries`` of this list: the ``dmnerf_volume_edit_entry`` structs, ``None`` for an empty list."""
        return pack_entries(self.who, self.trans_list, self.target_labels, what_for)


def _preview_sets(who, label_grid, H, W, K, pose, trans_list, target_labels, keep_labels, max_sets=None):
    """The rays and label sets of an edit preview (``preview_frame``'s docstring) -> ``(rays [R, 2, H W, 3], R label sets)``: set 0 the
    original rays of ``ManipulationFrameRenderer`` with every label but those of MOVE and REMOVE entries, set ``1 + e`` the target rays
    of the e-th entry with rays and its own label; with ``keep_labels`` every set is intersected with it.  ``max_sets``: more sets
    raise ``ValueError``.  The argument checks come before anything touches a device."""
    import types
    C = label_grid.C
    edits = EditList(who, trans_list, target_labels, C, keep_labels)
    trans_list, target_labels, keep, kinds = edits.trans_list, edits.target_labels, edits.keep, edits.kinds
    with_rays = sum(k != 2 for k in kinds)
    if max_sets is not None and 1 + with_rays > max_sets:
        raise ValueError(f"{who}: {with_rays} edits with rays, at most {max_sets - 1} (one launch composites {max_sets} ray sets)")
    args = types.SimpleNamespace(N_importance=0, target_labels=target_labels)
    pose = torch.as_tensor(pose, dtype=torch.float32).cpu()                         # host data: 12 floats into the ray kernels' arguments
    fr = D.ManipulationFrameRenderer(H, W, K, pose, trans_list, None, args, ins_num=C - 1, rank=0, world=1,
                                     keep_labels=keep if (keep is not None or trans_list) else ())
    if fr.ori.device != label_grid.labels.device:
        raise RuntimeError(f"{who}: the label volume lives on another device than the rays")
    own, per_entry = edits.label_sets()
    sets = [own] + [s for s, k in zip(per_entry, kinds) if k != 2]
    rays = torch.cat([fr.ori[None], fr.tar], dim=0) if fr.T else fr.ori[None]
    return rays, sets


def _preview_colours(who, label, lut, C):
    """``lut[label]`` uint8 ``[H, W, 3]``, black where ``label == 255``; ``None`` without ``lut``."""
    if lut is None:
        return None
    _lib.require_gpu(lut)
    if lut.dtype != torch.uint8 or lut.dim() != 2 or lut.shape[1] != 3 or lut.shape[0] < C:
        raise ValueError(f"{who}: lut must be uint8 [>= {C}, 3], got {lut.dtype} {tuple(lut.shape)}")
    hit = label != 255
    return lut[torch.where(hit, label, torch.zeros_like(label)).long()] * hit[..., None].to(torch.uint8)


def preview_frame(label_grid, H, W, K, pose, trans_list=(), target_labels=(), keep_labels=None, near=0.0, far=float("inf"), lut=None):
    """What an edit does to a frame, from the label volume alone: ``label`` uint8 ``[H, W]`` (255: nothing), ``depth`` f32 ``[H, W]``
    (the hit's ``t``, ``+inf`` on a miss), ``source`` uint8 ``[H, W]`` (0: the original rays, ``1 + e``: the target rays of the e-th
    entry WITH rays, 255: nothing) and ``ins_img`` uint8 ``[H, W, 3]`` = ``lut[label]``, black on a miss (``None`` without ``lut``, the
    table of ``label_lut`` with at least ``C`` rows), all on the device.

    ``trans_list`` / ``target_labels`` / ``keep_labels`` are ``ManipulationFrameRenderer``'s: 4 x 4 matrices, ``Deform``, ``Remove()``,
    ``Copy(...)``.  The original and target rays ARE that renderer's (``models=None``: same ``trans @ pose``, same ray kernels, same
    ``Deform`` offsets).  ONE ``dmnerf_label_trace`` with ``R = 1 +`` (entries with rays) sets: set 0, the original rays, accepts
    every label but those of MOVE and REMOVE entries; set ``1 + e``, the target rays of entry e, accepts ``target_labels[e]`` only;
    with ``keep_labels`` every set is intersected with it.  This is the exchanger's per-sample rule: along the original ray the moved
    object's samples are dropped, along the target ray only its own are taken.  A pixel's rays share the ray parameter (a target ray
    is the original one under an affine map), so the smallest ``t`` over the sets is the nearest surface along the pixel.

    A hard-surface proxy: the first labelled cell, no transmittance, no colour; how well it agrees with ``argmax`` of
    ``manipulate_frame`` is measured on the analytic scene only; ``render_preview`` composites instead.  Nothing reaches the host: with matrices (the poses are
    host data) it can be captured in a graph after a warm-up call and follows ``label_grid.labels`` on replay; a ``Deform`` uploads
    its offset table on every call."""
    H, W = int(H), int(W)
    rays, sets = _preview_sets("preview_frame", label_grid, H, W, K, pose, trans_list, target_labels, keep_labels)
    out = label_grid.trace_sets(rays, sets, near, far)
    label = out["label"].reshape(H, W)
    ins_img = _preview_colours("preview_frame", label, lut, label_grid.C)
    return {"label": label, "depth": out["t"].reshape(H, W), "source": out["source"].reshape(H, W), "ins_img": ins_img}


def render_preview(baked, H, W, K, pose, trans_list=(), target_labels=(), keep_labels=None, near=0.0, far=float("inf"), stop=0.0, lut=None):
    """``preview_frame`` with colour and transmittance, from a ``field.BakedGrid``: the same rays and the same label sets, but ONE
    ``dmnerf_baked_render`` that volume-renders the baked cells of every set along the pixel instead of stopping at the first one
    (``BakedGrid.render_sets``).  Returns ``rgb`` f32 ``[H, W, 3]``, ``depth`` f32 ``[H, W]`` (the weighted ``t``, 0 on a miss), ``acc``
    f32 ``[H, W]``, ``label`` / ``source`` uint8 ``[H, W]`` (those of the heaviest segment; 255: nothing), ``nseg`` int32 ``[H, W]`` and
    ``ins_img`` as ``preview_frame`` makes it, all on the device.

    Matrices, ``Deform``, ``Remove``, ``Copy`` and ``keep_labels`` work as there.  The kernel keeps every set's walk in registers and
    takes at most 4 ray sets, so more than three entries with rays raise ``ValueError`` (``Remove`` entries have none).  ``stop``: a
    pixel ends once its transmittance is below it.  Still a proxy: one colour per cell, baked for one view direction
    (``field.bake_grid``), piecewise constant density, no background; DESIGN.md 8a has the measured agreement with rendered frames
    on the analytic scene.  Graph capture as for ``preview_frame``; a replay follows ``baked.labels`` and ``baked.cells``."""
    from . import field
    H, W, stop = int(H), int(W), float(stop)
    if not stop >= 0.0:
        raise ValueError(f"render_preview: stop must be >= 0, got {stop}")
    rays, sets = _preview_sets("render_preview", baked, H, W, K, pose, trans_list, target_labels, keep_labels, max_sets=field.MAX_RENDER_SETS)
    out = baked.render_sets(rays, sets, near, far, stop)
    label = out["label"].reshape(H, W)
    return {"rgb": out["rgb"].reshape(H, W, 3), "depth": out["depth"].reshape(H, W), "acc": out["acc"].reshape(H, W), "label": label,
            "source": out["source"].reshape(H, W), "nseg": out["nseg"].reshape(H, W),
            "ins_img": _preview_colours("render_preview", label, lut, baked.C)}


# ---- an edit applied to the volume itself (csrc/volume_edit.hip; tests/_volume_edit_restate.py states it in numpy)
MAX_VOLUME_EDITS = 32           # DMNERF_VOLUME_EDIT_MAX (include/dmnerf_hip.h)
VOLUME_RULES = {"first": 0, "densest": 1}


def _overlaps(a, b):
    """Two tensors share device memory."""
    if a is None or b is None or a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def pack_entries(who, trans_list, target_labels, what_for):
    """``trans_list`` / ``target_labels`` (equal lengths, checked by the caller) as ``dmnerf_volume_edit_entry`` structs, ``None`` for an
    empty list: kind, label, and rows 0..2 of the matrix rounded to f32 once.  A ``Deform``, bare or inside ``Copy``, and a matrix that
    is not 4 x 4 raise ``ValueError`` in ``who``'s name; ``what_for`` ends the sentence about the missing world-space map."""
    E = len(trans_list)
    entries = (_lib.VolumeEditEntry * E)() if E else None
    for e, (trans, label) in enumerate(zip(trans_list, target_labels)):
        matrix = trans.matrix if isinstance(trans, Copy) else trans
        if isinstance(matrix, Deform):
            raise ValueError(f"{who}: entry {e} is a {trans!r}: a deformation's target rays depend on the image row, so it has no "
                             f"world-space map to {what_for}")
        entries[e].kind, entries[e].label = edit_kind(trans), label
        if not isinstance(trans, Remove):
            m = (matrix.detach().cpu().numpy() if torch.is_tensor(matrix) else np.asarray(matrix)).astype(np.float64)
            if m.shape != (4, 4):
                raise ValueError(f"{who}: entry {e} must be a 4 x 4 matrix, a Remove() or a Copy(matrix), got shape {m.shape}")
            entries[e].m[:] = [float(v) for v in m.astype(np.float32)[:3, :4].reshape(-1)]
    return entries


def edit_volume(grid, trans_list, target_labels, keep_labels=None, rule="first", out=None):
    """The edit applied to the volume itself: ``grid`` (a ``field.LabelGrid`` or a ``field.BakedGrid``) resampled under ``trans_list``
    once -> ``{"grid", "source", "won", "claimed", "hits"}``, all on the device.  ``"grid"`` is a new object of ``grid``'s class over the
    same box and ``C``: a scene like any other, so ``stats()``, ``skip_grid()``, ``pick``, ``preview_frame`` / ``render_preview`` with an
    empty ``trans_list`` (ONE ray set per frame, for any number of edits) and a second ``edit_volume`` work on it unchanged.

    ``trans_list`` / ``target_labels`` / ``keep_labels`` are the renderers': 4 x 4 matrices (``about(...)`` products as they are),
    ``Remove()`` and ``Copy(matrix)``; at most 32 entries.  The target pose of an entry is ``trans @ pose``, so a point ``x`` of a pixel's
    original ray corresponds to ``trans x`` on its target ray: the edited volume at ``x`` is the source volume at ``trans x``.  The matrix
    (rounded to f32 once) maps the centre of a DESTINATION cell to its source point; no inverse is taken.  Per cell (``dmnerf_volume_edit``,
    one launch): candidate 0 is the cell's own content unless its label is that of a MOVE or REMOVE entry (or not in ``keep_labels``);
    candidate ``1 + e`` is the source cell of a MOVE / COPY entry ``e`` if it lies in the box and carries ``target_labels[e]``.
    ``rule="first"``: the lowest candidate wins; ``rule="densest"`` (baked volumes only): the one with the largest source sigma, the
    lowest on ties, a NaN sigma never beating a number.  Nearest-cell resampling, no interpolation; a rotated object keeps the colour
    baked for the box's +z direction; what leaves the box is lost.

    ``source`` uint8 ``[dx, dy, dz]``: the winner's candidate number, 255 for none.  Here ``1 + e`` is the index into ``trans_list``,
    ``Remove`` entries INCLUDED -- unlike ``preview_frame``'s ``source``, which counts only the entries with rays.  ``won [1 + E]``,
    ``claimed [E]``, ``hits [E, C]`` int64: cells per winner; cells where candidate ``1 + e`` exists, winner or not; and for every cell
    with two or more candidates, every entry ``e`` among them and every OTHER candidate ``b`` there, ``hits[e, label(b)] += 1``
    (``label(0)`` the cell's own label): ``hits[e, l] > 0`` reads "entry e lands on something that carries label l".  Integer atomics
    only: the same numbers every run.

    ``out``: an earlier result's ``"grid"`` (the same class, dims, ``C``, box and device) to write into (it must not share memory with ``grid``).
    Nothing reaches the host: after one warm-up call, ``edit_volume(..., out=res["grid"])`` can be captured in a graph and follows
    ``grid.labels`` / ``grid.cells`` on replay.

    ``ValueError``, before anything touches a device: a ``Deform``, bare or inside ``Copy`` (its target rays depend on the image row:
    there is no world-space map to resample under), more than 32 entries, a label outside ``[0, C)``, unequal list lengths,
    ``rule="densest"`` on a plain ``LabelGrid``, an ``out`` of another class / dims / ``C`` / box / device or one that aliases ``grid``.  CPU tensors
    raise as everywhere (``_lib.require_gpu``)."""
    from . import field
    who = "edit_volume"
    if not isinstance(grid, field.LabelGrid):
        raise TypeError(f"{who}: grid must be a field.LabelGrid or a field.BakedGrid")
    baked = isinstance(grid, field.BakedGrid)
    C = grid.C
    edits = EditList(who, trans_list, target_labels, None, keep_labels, MAX_VOLUME_EDITS, " in one call (apply the rest to the result)")
    E = edits.E
    if rule not in VOLUME_RULES:
        raise ValueError(f"{who}: rule must be 'first' or 'densest', got {rule!r}")
    if rule == "densest" and not baked:
        raise ValueError(f"{who}: rule='densest' compares baked densities: it needs a field.BakedGrid, not a plain LabelGrid")
    edits.check_labels(C)
    keep = range(C) if edits.keep is None else edits.keep
    entries = edits.entries("resample the volume under (preview_frame / render_preview take it)")
    src_cells = grid.cells if baked else None
    if out is not None:
        if out is not grid and (type(out) is not type(grid) or out.dims != grid.dims or out.C != C or not np.array_equal(out.lo, grid.lo)
                                or not np.array_equal(out.hi, grid.hi) or out.labels.device != grid.labels.device):
            raise ValueError(f"{who}: out must be a {type(grid).__name__} of dims {grid.dims}, C = {C} and the box {grid.lo} .. {grid.hi} on "
                             f"{grid.labels.device} (an earlier result's 'grid')")
        if out is grid or _overlaps(out.labels, grid.labels) or (baked and _overlaps(out.cells, grid.cells)):
            raise ValueError(f"{who}: out shares memory with the source volume (the kernel reads other cells than the one it writes)")
    _lib.require_gpu(grid.labels, src_cells)
    dev = grid.labels.device
    if out is None:
        labels = torch.empty_like(grid.labels)
        out = field.BakedGrid(labels, torch.empty_like(grid.cells), grid.lo, grid.hi, C) if baked else field.LabelGrid(labels, grid.lo, grid.hi, C)
    else:
        _lib.require_gpu(out.labels, out.cells if baked else None)
    res = {"grid": out, "source": torch.empty(grid.dims, dtype=torch.uint8, device=dev),
           "won": torch.empty(1 + E, dtype=torch.int64, device=dev), "claimed": torch.empty(E, dtype=torch.int64, device=dev),
           "hits": torch.empty(E, C, dtype=torch.int64, device=dev)}
    _lib.launch("dmnerf_volume_edit", grid.labels, src_cells, *_lib.box_args(grid), C,
                (ctypes.c_uint32 * 4)(*field.label_mask_words(keep, C)), entries, E, VOLUME_RULES[rule], out.labels,
                out.cells if baked else None, res["source"], res["won"], res["claimed"], res["hits"])
    return res


# ---- the trained field rendered through an edited volume (csrc/field_edit.hip; tests/_field_edit_restate.py states it in numpy)
FIELD_POLICIES = {"evaluate": 0, "empty": 1}    # DMNERF_SKIP_OUTSIDE_* (include/dmnerf_hip.h)


def field_edit_masks(C, target_labels, kinds, keep_labels=None):
    """The accept masks of ``dmnerf_field_edit_filter`` -> ``4 (1 + E)`` 32-bit words (host integers): row 0 = ``own`` of
    ``edit_label_sets``, row ``1 + e`` = ``per_entry[e]``, each packed by ``field.label_mask_words``."""
    from . import field
    own, per_entry = edit_label_sets(C, target_labels, kinds, keep_labels)
    return [w for s in [own] + per_entry for w in field.label_mask_words(s, C)]


class FieldEdit:
    """What ``render.run_network_edited`` needs to render the TRAINED FIELD through an edited volume: ``source`` uint8 ``[dx, dy, dz]``
    on the device (``edit_volume``'s: 0 the cell's own content, ``1 + e`` entry ``e`` of ``trans_list``, 255 nobody), its box (``lo``,
    ``hi``, ``cell``, ``inv_cell``, ``dims``: ``field.LabelGrid``'s arithmetic), the entries, the accept masks and two policies.

    A sample in a cell owned by 0 is evaluated at its own point, one owned by ``1 + e`` at the point entry ``e``'s matrix carries it back
    to (the matrix maps the edited scene to the trained one, as in ``edit_volume``; no inverse is taken), one owned by nobody not at all.
    ``outside`` / ``unowned`` (``"evaluate"``: owner 0, ``"empty"``: nobody) say what a sample outside the box and one in a cell of
    byte 255 get.  Behind the network the per-sample label decides whether the row counts (``masks``, ``(1 + E) x 4`` words, the sets
    of ``_preview_sets``): owner 0 accepts ``keep`` without the labels of MOVE and REMOVE entries, owner ``1 + e`` accepts
    ``{target_labels[e]} & keep``.

    ``source`` may be overwritten in place (an ``edit_volume`` of the same entries into it): a captured render follows it on replay.
    ``C`` is the number of labels, ``ins_num + 1`` of the models it is rendered with."""

    def __init__(self, source, lo, hi, trans_list, target_labels, C, keep_labels=None, outside="evaluate", unowned="evaluate", volume=None):
        from . import field
        who = "FieldEdit"
        _lib.require_gpu(source)
        if source.dtype != torch.uint8 or source.dim() != 3:
            raise ValueError(f"{who}: source must be uint8 [dx, dy, dz], got {source.dtype} {tuple(source.shape)}")
        self.C = int(C)
        if not 1 <= self.C <= field.MAX_LABELS:
            raise ValueError(f"{who}: C must be in [1, {field.MAX_LABELS}], got {self.C}")
        for name, policy in (("outside", outside), ("unowned", unowned)):
            if policy not in FIELD_POLICIES:
                raise ValueError(f"{who}: {name} must be 'evaluate' or 'empty', got {policy!r}")
        self.dims = field._dims3(tuple(source.shape))
        self.lo, self.hi, self.cell, self.inv_cell = field._box(who, lo, hi, self.dims)
        self.source, self.outside, self.unowned, self.volume = source, outside, unowned, volume
        edits = EditList(who, trans_list, target_labels, self.C, keep_labels, MAX_VOLUME_EDITS)
        self.target_labels, self.E, self.keep_labels, self.kinds = edits.target_labels, edits.E, edits.keep, edits.kinds
        self.entries = edits.entries("carry a sample back under")
        self.masks = (ctypes.c_uint32 * (4 * (1 + self.E)))(*field_edit_masks(self.C, self.target_labels, self.kinds, self.keep_labels))

    @classmethod
    def from_volume(cls, grid, trans_list, target_labels, keep_labels=None, rule="first", outside="evaluate", unowned="evaluate"):
        """``edit_volume(grid, trans_list, target_labels, keep_labels, rule)`` and its ``source``; the whole result stays as ``.volume``."""
        res = edit_volume(grid, trans_list, target_labels, keep_labels=keep_labels, rule=rule)
        return cls(res["source"], grid.lo, grid.hi, trans_list, target_labels, grid.C, keep_labels, outside, unowned, volume=res)

    @classmethod
    def from_source(cls, source, lo, hi, trans_list, target_labels, C=None, keep_labels=None, outside="evaluate", unowned="evaluate"):
        """Wraps a given byte volume over the box ``[lo, hi)``.  ``C``: the number of labels (default: the most a byte volume names)."""
        from . import field
        return cls(source, lo, hi, trans_list, target_labels, field.MAX_LABELS if C is None else C, keep_labels, outside, unowned)


def _render(H, W, K, pose, edits, models, args, frame_kw):
    fr = D.ManipulationFrameRenderer(H, W, K, pose, edits, models, args, **frame_kw)
    for c in range(fr.n_chunks):
        fr.step(c)
    return fr.gather()


MAP_NAMES = ("rgb", "ins", "tar_rgb", "tar_ins")


def manipulate_demo_path(view_poses, hwk, models, args, objs, objs_trans, ins_rgbs, color_dict, ins_map, keep_maps=False,
                         products=None, keep_labels=None, skip=None, skip_levels=("coarse", "fine"), field_edit=None, **frame_kw):
    """The pose loop of ``manipulator_demo`` (networks/manipulator.py:384-488) without its file output: per view ``i`` every
    object of ``objs`` is edited at once -- ``obj['mani_mode'] == 'deform'``: ``Deform(obj['deform_func'], i)``, otherwise the
    rigid ``objs_trans[obj['obj_name']][i]['transformation']`` -- with ``target_labels = [obj['tar_id'] ...]`` (:395, :437), one
    ``ManipulationFrameRenderer`` frame (``frame_kw`` goes to it: ``raygen=``, ``target_rays=``, ``manipulate_chunk=``, ``draws=``,
    ``rank=`` / ``world=`` ...), then ``frame_products`` with the table of ``render_label2img``.

    Returns a dict of stacked device tensors: ``rgb8 [P,H,W,3]`` (``{i}_rgb.png``), ``ins_img [P,H,W,3]`` (``{i}_ins.png``),
    ``mask [P,H,W]`` uint8 (``{i}_ins_pred_mask.png``), ``label [P,H,W]`` int64; ``keep_maps=True``: also the four float frames
    ``rgb, ins, tar_rgb, tar_ins``.  Never synchronises with the host (poses and transformations are host data).  ``products``
    (injectable, for tests of the loop on the CPU): a stand-in for ``frame_products``.

    Extension: a ``'transformation'`` of ``objs_trans`` may be a ``Remove()`` or a ``Copy(matrix)``, and ``keep_labels`` shows
    only the objects of that set (isolate); ``objs`` may then be empty.  ``skip=`` a ``field.SkipGrid`` / ``skip_levels=``: every
    frame skips empty space (``ManipulationFrameRenderer(skip=)``); moves, ``Deform``, ``Remove``, ``Copy`` and ``keep_labels`` work with it.
    ``field_edit=`` a ``FieldEdit``: every view is the field-edit render of that one edited volume (``ManipulationFrameRenderer(field_edit=)``);
    the edits are the ``FieldEdit``'s, so ``objs`` must be empty, and it cannot be combined with ``keep_labels=`` or ``skip=``."""
    H, W, K = hwk
    if field_edit is not None:
        if len(objs):
            raise ValueError("manipulate_demo_path: field_edit= carries the edits itself; objs must be empty")
        if keep_labels is not None or skip is not None:
            raise ValueError("manipulate_demo_path: field_edit= cannot be combined with keep_labels= (the keep set is the FieldEdit's) or skip=")
        frame_kw = dict(frame_kw, field_edit=field_edit)
    if keep_labels is not None:
        frame_kw = dict(frame_kw, keep_labels=keep_labels)
    if skip is not None:
        frame_kw = dict(frame_kw, skip=skip, skip_levels=skip_levels)
    products = products or frame_products
    a = copy.copy(args)
    a.target_labels = [obj["tar_id"] for obj in objs]
    lut, cols = None, {}
    for i, pose in enumerate(view_poses):
        edits = [Deform(obj["deform_func"], i) if obj["mani_mode"] == "deform" else objs_trans[obj["obj_name"]][i]["transformation"]
                 for obj in objs]
        frame = _render(H, W, K, pose, edits, models, a, frame_kw)
        if lut is None:
            lut = label_lut(frame[1].shape[-1], ins_rgbs, color_dict, ins_map, device=frame[1].device)
        for name, t in zip(("rgb8", "label", "mask", "ins_img"), products(frame[0], frame[1], lut)):
            cols.setdefault(name, []).append(t)
        if keep_maps:
            for name, t in zip(MAP_NAMES, frame):
                cols.setdefault(name, []).append(t)
    return {k: torch.stack(v, 0) for k, v in cols.items()}


def gt_color_table(rgbs, color_dict, device):
    """``render_gt_label2img``'s colours (tools/visualizer.py:57-69) as a table: uint8 ``[G + 1, 3]`` on the device, row ``g`` =
    ``rgbs[color_dict[str(g)]]`` for the labels ``color_dict`` holds, 0 elsewhere; row ``G`` (zeros) takes every other label."""
    from . import field
    keys = [int(k) for k in color_dict.keys() if int(k) >= 0]
    G = max(keys, default=-1) + 1
    return torch.from_numpy(field.color_table(G + 1, rgbs, color_dict, {str(k): k for k in keys})).to(device)


def _gt_colors(table, labels):
    G = table.shape[0] - 1
    return table[torch.where((labels >= 0) & (labels < G), labels, torch.full_like(labels, G))]


def manipulate_eval_path(ori_poses, hwk, models, args, trans, gt_rgbs=None, gt_labels=None, ins_rgbs=None, color_dict=None,
                         image_metrics=True, keep_maps=False, lpips=None, skip=None, skip_levels=("coarse", "fine"), **frame_kw):
    """The pose loop of ``manipulator_eval`` (networks/manipulator.py:233-339) for one transformation ``trans`` (4 x 4, or a
    ``Deform``), without its file output: per pose one ``ManipulationFrameRenderer`` frame with ``target_labels =
    [args.target_label]`` (:231), then on the device

    * ``rgb8``, ``tar_rgb8`` uint8 ``[P,H,W,3]``: the edited frame and the plain target render (:310-318);
    * given ``gt_rgbs [P,H,W,3]``: ``psnr [P]`` (float32) and, with ``image_metrics``, ``psnr_f64`` / ``ssim`` of the edited frame
      (:278-279, ``evaluator.img_metrics_device``: one call for all poses after the loop); with ``lpips=`` an
      ``evaluator.LPIPSVGG`` also ``lpips [P]`` (float64) of the edited frame (:280);
    * given ``gt_labels [P,H,W]``: ``ap [P,6]``, ``matched [P,ins_num]``, ``gt_num [P]`` of ``ins[..., :-1]`` against the rows
      ``unique(gt_label)`` (:287-297: the branch of ``render_path`` without a crop); with ``ins_rgbs`` and ``color_dict`` also
      ``label [P,H,W]`` (argmax over ALL channels, :321), ``ins_img`` coloured through that pose's own matching (:299-323:
      ``ins_map[str(matched row)] = gt label``, built on the device from ``matched`` and the rows) and ``gt_ins_img``
      (``render_gt_label2img``, :327).  A gt label that ``color_dict`` does not hold is black (the reference raises ``KeyError``).

    ``keep_maps=True`` adds the float frames ``rgb, ins, tar_rgb, tar_ins``.  ``distributed.results_table`` takes the result as it
    is (LPIPS from ``out["lpips"]``, ``nan`` without a model).  The frames are complete on every rank: every rank computes the same numbers.
    ``skip=`` a ``field.SkipGrid`` / ``skip_levels=``: every frame skips empty space (``ManipulationFrameRenderer(skip=)``)."""
    H, W, K = hwk
    render_kw = frame_kw if skip is None else dict(frame_kw, skip=skip, skip_levels=skip_levels)
    cols = {}
    table = None
    scored = image_metrics and gt_rgbs is not None
    perceptual = lpips is not None and gt_rgbs is not None
    for i, pose in enumerate(ori_poses):
        rgb, ins, tar_rgb, tar_ins = _render(H, W, K, pose, [trans], models, args, render_kw)
        cols.setdefault("rgb8", []).append(frame_products(rgb)[0])
        cols.setdefault("tar_rgb8", []).append(frame_products(tar_rgb)[0])
        if keep_maps or scored or perceptual:
            cols.setdefault("rgb", []).append(rgb)
        if keep_maps:
            for name, t in zip(MAP_NAMES[1:], (ins, tar_rgb, tar_ins)):
                cols.setdefault(name, []).append(t)
        if gt_rgbs is not None:
            gt = torch.as_tensor(gt_rgbs[i]).to(rgb)
            cols.setdefault("psnr", []).append(-10.0 * torch.log10(torch.mean((rgb - gt) ** 2)))
        if gt_labels is not None:
            C = ins.shape[-1]
            ap, matched, gt_num = D._frame_ap({"ins": [ins[..., :C - 1]]}, gt_labels[i], False, False, args, frame_kw)
            for name, t in zip(("ap", "matched", "gt_num"), (ap, matched, gt_num)):
                cols.setdefault(name, []).append(t)
            if ins_rgbs is not None and color_dict is not None:
                if table is None:
                    table = gt_color_table(ins_rgbs, color_dict, ins.device)
                gl = torch.as_tensor(gt_labels[i]).to(device=ins.device, dtype=torch.int64).reshape(H, W)
                rows = torch.unique(gl)                                             # the rows _frame_ap matched, ascending
                m = matched[:rows.numel()]
                lut = torch.zeros(C + 1, 3, dtype=torch.uint8, device=ins.device)   # row C: the unmatched gt rows
                lut[torch.where(m >= 0, m, torch.full_like(m, C))] = _gt_colors(table, rows)
                _, label, _, ins_img = frame_products(rgb, ins, lut[:C])
                for name, t in zip(("label", "ins_img", "gt_ins_img"), (label, ins_img, _gt_colors(table, gl))):
                    cols.setdefault(name, []).append(t)
    out = {k: torch.stack(v, 0) for k, v in cols.items()}
    if scored or perceptual:
        gt = torch.stack([torch.as_tensor(gt_rgbs[i]).to(out["rgb"]) for i in range(out["rgb"].shape[0])], 0)
    if scored:
        from .networks import evaluator
        out["ssim"], out["psnr_f64"] = evaluator.img_metrics_device(out["rgb"], gt)
    if perceptual:
        out["lpips"] = lpips(out["rgb"], gt)
    if (scored or perceptual) and not keep_maps:
        del out["rgb"]
    return out
