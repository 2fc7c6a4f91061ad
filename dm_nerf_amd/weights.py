"""Reference state_dict -> the kernels' packed weights ("blobs").

``LAYOUTS`` describes every packed layout once -- which vector it gathers from, which library entries size it, index it and pack
it -- and ``pack`` follows it; ``DM_NeRF`` (networks/dm_nerf.py) keeps one cache over the layouts.  ``VARIANTS`` names, per kernel
variant, the layouts and library entries its consumers (autograd.py, networks/render.py) use."""

from collections import namedtuple

import numpy as np
import torch

from . import _lib

# DM_NeRF.__init__ / state_dict order (networks/dm_nerf.py:59-78 of the reference)
PARAM_MODULES = [f"mlps.{i}" for i in range(8)] + [
    "rgb_feature_linear", "ins_feature_linear", "rgb_feature_linears.0", "ins_feature_linears.0",
    "density_linear", "ins_linear", "rgb_linear"]
PARAM_KEYS = [f"{m}.{p}" for m in PARAM_MODULES for p in ("weight", "bias")]

HEAD_F_FLOATS = 128 * 256        # layout.h::HEAD_F_FLOATS
TAB_T_FLOATS = 1024              # layout.h::TAB_T_FLOATS

# layout (the name of its DM_NeRF accessor) -> (source, size entry, index entry, table, stream packer).
#   source: the vector gathered from -- "flat" (the parameters), "fused" (``fused_flat``) or "flat+F" (the parameters followed by
#           F = rgb_feature_linears.0.weight[:, :256] . rgb_feature_linear.weight, formed on the device by dmnerf_head_product);
#   table:  None -- the whole blob is ONE f32 gather (dmnerf_pack_weights) of the index entry's ``total`` ints; otherwise
#           (layout, floats): an f32 table gathered with the first ``floats`` of that layout's index, followed by a 16-bit stream
#           of ``total - floats`` words whose index has two ints per word.  A layout that names ITSELF gets table and stream index
#           from one call of its index entry.
LAYOUTS = {
    "blob": ("flat", "dmnerf_blob_floats", "dmnerf_build_pack_index", None, "dmnerf_pack_weights"),
    "blob_fused": ("fused", "dmnerf_blob_fused_floats", "dmnerf_build_pack_index_fused", None, "dmnerf_pack_weights"),
    "blob_t": ("flat+F", "dmnerf_blob_t_floats", "dmnerf_build_pack_index_t", None, "dmnerf_pack_weights"),
    "blob_split": ("fused", "dmnerf_blob_split_words", "dmnerf_build_pack_index_split", ("blob_fused", 4096), "dmnerf_pack_split"),
    "blob_f16": ("fused", "dmnerf_blob_f16_words", "dmnerf_build_pack_index_f16", ("blob_f16", 4096), "dmnerf_pack_f16"),
    "blob_t_split": ("flat+F", "dmnerf_blob_t_split_words", "dmnerf_build_pack_index_t_split", ("blob_t", TAB_T_FLOATS), "dmnerf_pack_split"),
    "blob_t_f16": ("flat+F", "dmnerf_blob_t_f16_words", "dmnerf_build_pack_index_t_f16", ("blob_t", TAB_T_FLOATS), "dmnerf_pack_f16"),
}

# kernel variant (None: the default f32 kernels | "fused": ``args.fuse_heads`` | ``split_mode(args)``) -> ``fused_heads`` of the
# render structs, the forward layout with its inference and training entries, the W^T layout with its data-gradient entry, the
# weight-gradient entry and the (sizes, plan) entries of its split-K plan.  "fused" is a forward only: default f32 backward.
Variant = namedtuple("Variant", "fused_heads blob fwd fwd_train blob_t dgrad wgrad plan")
VARIANTS = {
    None: Variant(0, "blob", "dmnerf_mlp_fwd_rays", "dmnerf_mlp_fwd_rays_train", "blob_t", "dmnerf_mlp_bwd_data",
                  "dmnerf_mlp_bwd_weights", ("dmnerf_wgrad_plan_sizes", "dmnerf_wgrad_plan")),
    "fused": Variant(1, "blob_fused", "dmnerf_mlp_fwd_rays_fused", "dmnerf_mlp_fwd_rays_train_fused", "blob_t", "dmnerf_mlp_bwd_data",
                     "dmnerf_mlp_bwd_weights", ("dmnerf_wgrad_plan_sizes", "dmnerf_wgrad_plan")),
    "bf16x3": Variant(2, "blob_split", "dmnerf_mlp_fwd_rays_split", "dmnerf_mlp_fwd_rays_train_split", "blob_t_split", "dmnerf_mlp_bwd_data_split",
                      "dmnerf_mlp_bwd_weights_split", ("dmnerf_wgrad_plan_sizes_split", "dmnerf_wgrad_plan_split")),
    "f16x2": Variant(3, "blob_f16", "dmnerf_mlp_fwd_rays_f16", "dmnerf_mlp_fwd_rays_train_f16", "blob_t_f16", "dmnerf_mlp_bwd_data_f16",
                     "dmnerf_mlp_bwd_weights_f16", ("dmnerf_wgrad_plan_sizes_f16", "dmnerf_wgrad_plan_f16")),
}

_index_cache = {}                # (ins_num, device, layout) -> (table index or None, index) on the device


def index_host(layout, ins_num):
    """``(table index or None, index)`` of ``layout`` as int32 numpy arrays (host only; works without a GPU).  The table index is
    there for a layout that builds its own (see ``LAYOUTS``)."""
    _, f_size, f_index, table, _ = LAYOUTS[layout]
    total = getattr(_lib.load(), f_size)(ins_num)
    if total <= 0:
        raise ValueError(f"unsupported ins_num={ins_num}")
    if table is None:
        idx = np.empty(total, dtype=np.int32)
    else:
        idx = np.empty((total - table[1]) * 2, dtype=np.int32)
        if table[0] == layout:
            tab = np.empty(table[1], dtype=np.int32)
            _lib.call(f_index, ins_num, tab, tab.size, idx, idx.size)
            return tab, idx
    _lib.call(f_index, ins_num, idx, idx.size)
    return None, idx


def _index(layout, ins_num, device):
    key = (ins_num, str(device), layout)
    if key not in _index_cache:
        _index_cache[key] = tuple(None if h is None else torch.from_numpy(h).to(device) for h in index_host(layout, ins_num))
    return _index_cache[key]


def pack_index_host(ins_num):
    """int32 numpy gather index of the default blob."""
    return index_host("blob", ins_num)[1]


def pack_index_t_host(ins_num):
    """Gather index of the backward (W^T) blob."""
    return index_host("blob_t", ins_num)[1]


def pack_index_fused_host(ins_num):
    """Gather index of the fused-heads inference blob."""
    return index_host("blob_fused", ins_num)[1]


def _f32_layout(transposed, fused):
    return "blob_t" if transposed else ("blob_fused" if fused else "blob")


def pack_index(ins_num, device, transposed=False, fused=False):
    return _index(_f32_layout(transposed, fused), ins_num, device)[1]


def fused_flat(flat, ins_num):
    """The flat parameter vector with the activation-free ``rgb_feature_linear`` / ``ins_feature_linear`` (dm_nerf.py:89,96)
    folded into the hidden layers that consume them -- formed on the device by ``dmnerf_fuse_heads`` (float64 accumulation,
    rounded once; csrc/heads.hip).  Inference only: the same function up to f32 re-association."""
    out = torch.empty_like(flat)
    _lib.launch("dmnerf_fuse_heads", flat, ins_num, out)
    return out


def flat_params(state):
    """Concatenate parameters in reference order.  ``state``: mapping key -> tensor (all on one GPU)."""
    return torch.cat([state[k].detach().reshape(-1).float() for k in PARAM_KEYS])


def split_mode(args):
    """``args.mfma_split`` -> None (off) | "bf16x3" (True or "bf16x3": three bf16 planes, six products) | "f16x2" (two f16
    planes, three products).  Both are f32-class, neither is the bitwise fmaf chain of the default kernels."""
    m = getattr(args, "mfma_split", False)
    if not m:
        return None
    if m is True or str(m) == "bf16x3":
        return "bf16x3"
    if str(m) == "f16x2":
        return "f16x2"
    raise ValueError(f"args.mfma_split = {m!r}: expected False, True / 'bf16x3' or 'f16x2'")


def pack(layout, flat, ins_num):
    """A NEW tensor holding ``layout`` (a key of ``LAYOUTS``) of the flat parameter vector ``flat`` of one DM_NeRF model."""
    source, f_size, _, table, f_stream = LAYOUTS[layout]
    lib = _lib.load()
    if flat.numel() != lib.dmnerf_param_count(ins_num):
        raise ValueError(f"parameter count {flat.numel()} != {lib.dmnerf_param_count(ins_num)} "
                         f"(only D=8, W=256, skips=[4], 63+27 input channels are supported)")
    _lib.require_gpu(flat)
    total = getattr(lib, f_size)(ins_num)
    if total <= 0:
        raise ValueError(f"unsupported ins_num={ins_num}")
    if source == "fused":
        flat = fused_flat(flat, ins_num)
    elif source == "flat+F":         # F sits behind the flat parameters and is gathered like any other weight
        ext = torch.empty(flat.numel() + HEAD_F_FLOATS, dtype=torch.float32, device=flat.device)
        ext[:flat.numel()] = flat
        _lib.launch("dmnerf_head_product", flat, ins_num, ext[flat.numel():])
        flat = ext
    idx_tab, idx = _index(layout, ins_num, flat.device)
    blob = torch.empty(total, dtype=torch.float32, device=flat.device)
    if table is None:
        _lib.launch(f_stream, flat, idx, blob, total)
        return blob
    tab_of, tab = table
    if tab_of != layout:
        idx_tab = _index(tab_of, ins_num, flat.device)[1][:tab].contiguous()
    _lib.launch("dmnerf_pack_weights", flat, idx_tab, blob, tab)
    _lib.launch(f_stream, flat, idx, blob[tab:], total - tab)
    return blob


def pack_blob(state, ins_num, transposed=False, fused=False, flat=None):
    """``pack`` of the default blob, the W^T blob of the backward data-gradient kernel (``transposed``) or the inference blob with
    the feature linears folded into the hidden layers (``fused``).  ``flat``: the flat parameter vector if the caller already has it."""
    return pack(_f32_layout(transposed, fused), flat_params(state) if flat is None else flat, ins_num)
