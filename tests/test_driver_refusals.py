"""The refusals of the Python ray drivers that answer before any device is touched: exception type, full text, the name of the
entry the caller used, and which check answers when two arguments are bad at once.  No GPU and no shared library is needed:
models are stand-ins with the three attributes the checks read, tensors live on the host, and a grid is a bare ``SkipGrid``
instance (``__new__`` only: the constructor itself wants device memory), which is all ``isinstance`` asks for.

Where the next check of an entry is ``_lib.require_gpu``, the host tensor's refusal (``CPU``) is asserted too: it pins that the
checks after it -- grid device, ``counts``, ``N_importance >= 0``, the shapes of the draws -- are NOT reachable without a device.
Not reachable either, and therefore not here: every ``LabelGrid`` constructor check (``require_gpu(labels)`` comes first), the
``bits`` check of ``SkipGrid``, ``TrainSkip``'s grid, and the shape / device checks of ``SkipGrid.mark`` and ``LabelGrid.trace*``."""
from types import SimpleNamespace as NS

import pytest
import torch

from dm_nerf_amd import autograd, distributed, field
from dm_nerf_amd.networks import manipulator as M
from dm_nerf_amd.networks import render as R

CPU = (RuntimeError, "dm_nerf_amd runs on MI355X only: got a CPU tensor (there is no CPU fallback)")
BIG = 1 << 31


def refused(exc_text, fn, *a, **kw):
    exc, text = exc_text
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    assert type(e.value) is exc and str(e.value) == text, (type(e.value), str(e.value))


def model(ok=True, ins_num=3):
    return NS(_fused_ok=lambda: ok, ins_num=ins_num, input_ch_pts=63, input_ch_views=27, parameters=lambda: iter(()))


def args(**kw):
    return NS(**dict(dict(N_importance=4, perturb=0.0, N_samples=4, near=0.0, far=1.0, target_labels=[1]), **kw))


GRID = field.SkipGrid.__new__(field.SkipGrid)
O = torch.zeros(2, 3)
Z = torch.zeros(2, 4)
Z_BIG = torch.zeros(1).expand(1 << 16, 1 << 15)                # 2^31 samples, one float of memory
RAYS = torch.zeros(2, 2, 3)


# ---- render.run_network_skip / autograd.run_network_train_skip ------------------------------------------------------------------
SELECT = {
    "run_network_skip": (lambda *a, **kw: R.run_network_skip(*a, **kw),
                         "no sparse network kernel for", "the sparse network kernels exist", "render in smaller chunks"),
    "run_network_train_skip": (lambda *a, **kw: autograd.run_network_train_skip(*a, **kw),
                               "no training through the grid for", "training through the grid exists", "train on smaller batches"),
}


@pytest.mark.parametrize("who", sorted(SELECT))
def test_skip_selection_refusals_in_their_order(who):
    fn, no_kernel, exists, smaller = SELECT[who]
    bad_grid = (TypeError, f"{who}: grid must be a field.SkipGrid")
    bad_split = (ValueError, f"{who}: {no_kernel} args.mfma_split = 'bf16x3' (f32 and 'f16x2' only)")
    bad_model = (ValueError, f"{who}: {exists} for the 8 x 256 network only")
    too_many = (ValueError, f"{who}: {BIG} samples do not fit the int32 selection; {smaller}")
    refused(bad_grid, fn, model(False), O, O, Z_BIG, object(), split="bf16x3")
    refused(bad_grid, fn, model(), O, O, Z, None)
    refused(bad_split, fn, model(False), O, O, Z_BIG, GRID, split="bf16x3")
    refused(bad_model, fn, model(False), O, O, Z_BIG, GRID)
    refused(bad_model, fn, model(False), O, O, Z_BIG, GRID, split="f16x2")
    refused(too_many, fn, model(), O, O, Z_BIG, GRID, counts=torch.zeros(3))
    refused(CPU, fn, model(), O, O, Z, GRID, counts=torch.zeros(3))       # the grid-device and counts checks come after this one


def test_train_skip_bucket_answers_between_the_network_and_the_size_check():
    fn = autograd.run_network_train_skip
    refused((ValueError, "run_network_train_skip: bucket must be >= 1, got 0"), fn, model(), O, O, Z_BIG, GRID, bucket=0)
    refused((ValueError, "run_network_train_skip: bucket must be >= 1, got -3"), fn, model(), O, O, Z, GRID, bucket=-3)
    refused((ValueError, "run_network_train_skip: training through the grid exists for the 8 x 256 network only"),
            fn, model(False), O, O, Z, GRID, bucket=0)


# ---- the fine entries -----------------------------------------------------------------------------------------------------------
FINE = {"dm_nerf_fine": "no args.mfma_split", "dm_nerf_fine_f16": 'args.mfma_split = "f16x2"',
        "dm_nerf_fine_skip": 'no args.mfma_split or "f16x2"', "dm_nerf_fine_mark": 'no args.mfma_split or "f16x2"'}
EMBEDDERS = (ValueError, "dm_nerf: the embedders' out_dim does not match the models' input channels")


def fine_call(who, mc, mf, a, grid=GRID, pe=None, ve=None, **kw):
    extra = (grid,) if who in ("dm_nerf_fine_skip", "dm_nerf_fine_mark") else ()
    return getattr(R, who)(RAYS, pe, ve, mc, mf, Z, a, *extra, **kw)


@pytest.mark.parametrize("who", sorted(FINE))
def test_fine_entries_refuse_what_they_do_not_serve(who):
    only = (ValueError, f"{who}: inference with the 8 x 256 network, N_importance >= 1 and {FINE[who]} only -- use dm_nerf")
    wrong = NS(out_dim=5)
    refused(only, fine_call, who, model(False), model(), args(), pe=wrong)
    refused(only, fine_call, who, model(), model(False), args())
    refused(only, fine_call, who, model(), model(), args(N_importance=0))
    refused(only, fine_call, who, model(), model(), args(mfma_split="bf16x3"))
    served = {"dm_nerf_fine": [False], "dm_nerf_fine_f16": ["f16x2"]}.get(who, [False, "f16x2"])
    for split in (False, "f16x2"):
        a = args(mfma_split=split)
        if split not in served:
            refused(only, fine_call, who, model(), model(), a)
            continue
        refused(EMBEDDERS, fine_call, who, model(), model(), a, pe=wrong)
        refused(EMBEDDERS, fine_call, who, model(), model(), a, ve=wrong)
        refused(CPU, fine_call, who, model(), model(), a, pe=NS(out_dim=63), ve=NS(out_dim=27))
    assert R.fine_eligible(model(), model(), args()) and not R.fine_f16_eligible(model(), model(), args())
    assert R.fine_f16_eligible(model(), model(), args(mfma_split="f16x2")) and not R.fine_eligible(model(), model(), args(mfma_split="f16x2"))
    assert R.fine_renderer(model(), model(), args()) is R.dm_nerf_fine
    assert R.fine_renderer(model(), model(), args(mfma_split="f16x2")) is R.dm_nerf_fine_f16
    for a, mc in ((args(mfma_split=True), model()), (args(N_importance=0), model()), (args(), model(False))):
        assert R.fine_renderer(mc, model(), a) is R.dm_nerf


@pytest.mark.parametrize("who", ["dm_nerf_fine_skip", "dm_nerf_fine_mark"])
def test_grid_entries_check_grid_then_levels_then_the_call(who):
    bad_grid = (TypeError, f"{who}: grid must be a field.SkipGrid")
    refused(bad_grid, fine_call, who, model(False), model(), args(), grid=object(), levels=())
    refused(bad_grid, fine_call, who, model(), model(), args(), grid=None)
    for levels, shown in (((), "()"), ("mid", "('mid',)"), (("coarse", "x"), "('coarse', 'x')"), ([], "()")):
        refused((ValueError, f"{who}: levels must name 'coarse' and / or 'fine', got {shown}"),
                fine_call, who, model(False), model(), args(), levels=levels)
    refused(CPU, fine_call, who, model(), model(), args(), levels="fine")


def test_dm_nerf_inference_prologue():
    wrong = NS(out_dim=5)
    refused(EMBEDDERS, R.dm_nerf, RAYS, wrong, None, model(), model(), Z, args(N_importance=-1))
    refused(EMBEDDERS, R.dm_nerf, RAYS, None, wrong, model(False), model(), Z, args())
    refused(CPU, R.dm_nerf, RAYS, None, None, model(), model(), Z, args(N_importance=-1))    # N_importance >= 0 comes after this one


def test_check_draws_shapes():
    u, t = torch.zeros(3), torch.zeros(2, 5)
    refused((ValueError, "dm_nerf: u must be [4] or [2, 4], got (3,)"), R.check_draws, None, u, 2, 4, 4, 0.0, "cpu")
    refused((ValueError, "dm_nerf: t_rand must be [2, 4] (one draw per coarse sample), got (2, 5)"), R.check_draws, t, u, 2, 4, 4, 1.0, "cpu")
    refused(CPU, R.check_draws, torch.zeros(2, 4), u, 2, 4, 4, 1.0, "cpu")
    assert R.check_skip_levels("x", "fine") == ("fine",) and R.check_skip_levels("x", ["fine", "coarse"]) == ("fine", "coarse")


# ---- autograd.dm_nerf_train ------------------------------------------------------------------------------------------------------
def test_dm_nerf_train_skip_refusals():
    fn = lambda skip, a=args(), **kw: autograd.dm_nerf_train(RAYS, model(), model(), Z, a, skip=skip, **kw)
    refused((TypeError, "dm_nerf_train: skip must be a field.SkipGrid or a field.TrainSkip"), fn, object(), skip_levels=())
    refused((ValueError, "dm_nerf_train: levels must name 'coarse' and / or 'fine', got ()"), fn, GRID, args(fuse_heads=True), skip_levels=())
    refused((ValueError, "dm_nerf_train: no training through the grid with args.fuse_heads (f32 and mfma_split = 'f16x2' only)"),
            fn, GRID, args(fuse_heads=True))
    refused(CPU, fn, GRID)
    holder = field.TrainSkip.__new__(field.TrainSkip)
    holder.grid = object()
    refused((TypeError, "dm_nerf_train: skip must be a field.SkipGrid or a field.TrainSkip"), fn, holder)


# ---- networks.manipulator --------------------------------------------------------------------------------------------------------
def manip(mc=None, mf=None, a=None, tar=(), **kw):
    return M.manipulator(None, None, mc or model(), mf or model(), RAYS, list(tar), a or args(), **kw)


@pytest.mark.parametrize("edit", [False, True])
def test_manipulator_skip_refusals(edit):
    kw = dict(kinds=[7]) if edit else {}                           # the skip plan answers before the kinds are looked at
    refused((TypeError, "manipulator: skip must be a field.SkipGrid"), manip, skip=object(), skip_levels=(), **kw)
    refused((ValueError, "manipulator: levels must name 'coarse' and / or 'fine', got ('both',)"),
            manip, a=args(mfma_split=True), skip=GRID, skip_levels="both", **kw)
    refused((ValueError, "manipulator: skip= has no sparse network kernel for args.mfma_split = 'bf16x3' (f32 and 'f16x2' only)"),
            manip, mc=model(False), a=args(mfma_split=True), skip=GRID, **kw)
    refused((ValueError, "manipulator: skip= needs the 8 x 256 network at the coarse level (the sparse kernels exist for it only)"),
            manip, mc=model(False), mf=model(False), skip=GRID, **kw)
    refused((ValueError, "manipulator: skip= needs the 8 x 256 network at the fine level (the sparse kernels exist for it only)"),
            manip, mc=model(False), mf=model(False), skip=GRID, skip_levels=("fine",), **kw)
    refused((ValueError, "args.mfma_split = 'x': expected False, True / 'bf16x3' or 'f16x2'"), manip, a=args(mfma_split="x"), skip=object(), **kw)


def test_manipulator_edit_refusals():
    refused((ValueError, "manipulator: 2 kinds for 1 target labels"), manip, kinds=[M.MOVE, 9])
    refused((ValueError, "manipulator: kinds must be MOVE (0), COPY (1) or REMOVE (2), got [3]"), manip, kinds=[3], tar=(RAYS, RAYS))
    refused((ValueError, "manipulator: 2 target ray sets for 1 MOVE / COPY entries"), manip, kinds=[M.COPY], tar=(RAYS, RAYS))
    refused((ValueError, "manipulator: 1 target ray sets for 0 MOVE / COPY entries"), manip, kinds=[M.REMOVE], tar=(RAYS,))
    refused((ValueError, "manipulator: no edit and no keep_labels"), manip, a=args(target_labels=[]), kinds=[])
    refused((ValueError, "edit_exchanger: 2 labels, 1 kinds, 2 / 2 targets"), M.edit_exchanger, Z, [None, None], Z, [None, None], [1, 2], [M.REMOVE])
    refused((ValueError, "keep_labels: label 4 outside [0, 4)"), M.keep_words, [0, 4], 4)
    refused((ValueError, "keep_labels: label -1 outside [0, 4)"), M.keep_words, [-1], 4)
    assert M.keep_words([0, 65], 128) == [1, 2]


# ---- distributed.FrameRenderer ---------------------------------------------------------------------------------------------------
def test_frame_renderer_exclusions():
    fr = lambda **kw: distributed.FrameRenderer(4, 4, None, None, None, 0.0, 1.0, args(), **kw)
    chunk = lambda *a, **kw: None
    refused((ValueError, "FrameRenderer: skip= routes the chunks through dm_nerf_fine_skip; it cannot be combined with render_chunk="),
            fr, skip=GRID, mark=GRID, render_chunk=chunk)
    refused((ValueError, "FrameRenderer: mark= records what a DENSE render uses; it cannot be combined with skip="), fr, skip=GRID, mark=GRID)
    refused((ValueError, "FrameRenderer: mark= routes the chunks through dm_nerf_fine_mark; it cannot be combined with render_chunk="),
            fr, mark=GRID, render_chunk=chunk)


# ---- field -----------------------------------------------------------------------------------------------------------------------
BOX = ((0, 0, 0), (1, 1, 1))


def test_dims3():
    assert field._dims3(4) == (4, 4, 4) and field._dims3([1, 2, 3]) == (1, 2, 3)
    for dims, shown in ((0, "(0, 0, 0)"), ((1, 2), "(1, 2)"), ((4, 0, 4), "(4, 0, 4)"), ((1, 2, 3, 4), "(1, 2, 3, 4)")):
        for make in (field.SkipGrid.empty, field.SkipGrid.full):
            refused((ValueError, f"dims must be one or three positive integers, got {shown}"), make, (0, 0, 0), (0, 0, 0), dims, "no", "cpu")
    refused((ValueError, f"{1 << 33} cells do not fit int32"), field.SkipGrid.empty, *BOX, 2048, device="cpu")
    refused((ValueError, f"{1 << 31} cells do not fit int32"), field.SkipGrid.empty, *BOX, (1 << 11, 1 << 10, 1 << 10), device="cpu")


def test_skip_grid_constructor():
    empty = field.SkipGrid.empty
    hi_lo = (ValueError, "SkipGrid: hi must be > lo on every axis")
    refused(hi_lo, empty, (0, 0, 0), (1, 0, 1), 2, "no", "cpu")
    refused(hi_lo, empty, (0, 0, 0), (1, float("nan"), 1), 2, device="cpu")
    refused(hi_lo, field.SkipGrid, (0, 0, 2), (1, 1, 1), 2, None)
    refused((ValueError, "SkipGrid: outside must be 'evaluate' or 'empty', got 'no'"), empty, *BOX, 2, "no", "cpu")
    refused((ValueError, "SkipGrid: outside must be 'evaluate' or 'empty', got None"), field.SkipGrid, *BOX, 2, torch.zeros(1), None)
    refused(CPU, empty, *BOX, 2, device="cpu")
    refused(CPU, field.SkipGrid.from_bits, [0], *BOX, 2, device="cpu")
    refused((ValueError, "TrainSkip: every must be >= 1 and warmup >= 0, got 0, 5"), field.TrainSkip, *BOX, every=0, warmup=5)
    refused((ValueError, "TrainSkip: every must be >= 1 and warmup >= 0, got 1, -1"), field.TrainSkip, *BOX, dims=0, every=1, warmup=-1)
    refused((TypeError, "SkipGrid.__or__: the other operand must be a SkipGrid"), lambda: GRID | 3)
    refused((ValueError, "SkipGrid.mark: threshold must be >= 0, got -1.0"), GRID.mark, None, None, None, None, -1)
    refused((ValueError, "SkipGrid.mark: rays_d must be a float32 tensor"), GRID.mark, O, O.double(), Z, Z)
    refused((ValueError, "or_gathered_words: (5,) words do not split over 2 ranks"), field.or_gathered_words, torch.zeros(5, dtype=torch.int32), 2)


def test_label_refusals():
    words = field.label_mask_words
    refused((ValueError, "keep_labels: label 4 outside [0, 4)"), words, 4, 4)
    refused((ValueError, "keep_labels: label -1 outside [0, 4)"), words, [1, -1], 4)
    refused((ValueError, "labels must be an int or an iterable of ints, got 1.5"), words, 1.5, 4)
    refused((ValueError, "label 1.0 is not an integer"), words, [0, 1.0], 4)
    assert words([0, 33, 127], 128) == [1, 2, 0, 1 << 31] and words(range(0), 4) == [0, 0, 0, 0]
    refused(CPU, field.LabelGrid, torch.zeros(2, 2, dtype=torch.uint8), *BOX, 0)          # nothing of LabelGrid answers before this
    lg = field.LabelGrid.__new__(field.LabelGrid)
    lg.C = 4
    refused((ValueError, "keep_labels: label 4 outside [0, 4)"), lg.skip_grid, [4])
    refused((ValueError, "LabelGrid.trace_sets: rays must be a float32 tensor"), lg.trace_sets, O.double(), [0], 0.0, 1.0)
    refused((ValueError, "LabelGrid.trace: rays_o must be a float32 tensor"), lg.trace, None, O, 0.0, 1.0)
    refused((ValueError, "label_grid: sigma_threshold must be >= 0, got -1.0"), field.label_grid, model(), object(), -1.0)
    refused((ValueError, "label_grid: sigma_threshold must be >= 0, got nan"), field.label_grid, model(), GRID, float("nan"))
    refused((TypeError, "label_grid: occ must be a SkipGrid"), field.label_grid, model(), object(), slab=0)
    refused((ValueError, "slab must be >= 1"), field.label_grid, model(), GRID, slab=0)
