"""Drop-in for the reference's ``networks/dm_nerf.py``: Embedder, get_embedder, DM_NeRF.

Same constructor arguments, parameter names and state_dict keys as the reference
(networks/dm_nerf.py:8-106), so checkpoints (train_dmsr.py:78-86) and torch.optim.Adam work
unchanged.  The arithmetic runs in libdmnerf_hip.so.
"""
import torch
import torch.nn as nn

from .. import _lib, weights


class Embedder:
    """``Embedder`` (networks/dm_nerf.py:8-38).  Only the configuration ``get_embedder`` builds
    (include_input, log sampling, sin/cos, 3 input dims) exists in the reference's configs."""

    def __init__(self, **kwargs):
        self.kwargs = kwargs
        if not (kwargs.get('include_input', True) and kwargs.get('log_sampling', True)
                and kwargs.get('input_dims', 3) == 3):
            raise NotImplementedError("Embedder: only include_input=True, log_sampling=True, input_dims=3")
        self.num_freqs = int(kwargs['num_freqs'])
        if int(kwargs['max_freq_log2']) != self.num_freqs - 1:
            raise NotImplementedError("Embedder: max_freq_log2 must equal num_freqs - 1 (powers of two)")
        self.out_dim = 3 + 2 * 3 * self.num_freqs

    def embed(self, inputs):
        """``cat([x, sin(x f0), cos(x f0), ...], -1)`` (networks/dm_nerf.py:37-38)."""
        x = _lib.f32(inputs)
        _lib.require_gpu(x)
        if x.shape[-1] != 3:
            raise ValueError("Embedder.embed expects [..., 3]")
        M = x.numel() // 3
        out = torch.empty(*x.shape[:-1], self.out_dim, dtype=torch.float32, device=x.device)
        _lib.launch("dmnerf_embed", x, M, self.num_freqs, out)
        return out


def get_embedder(multires, i=0):
    """``get_embedder`` (networks/dm_nerf.py:41-55)."""
    if i == -1:
        return nn.Identity(), 3
    embed_kwargs = {
        'include_input': True,
        'input_dims': 3,
        'max_freq_log2': multires - 1,
        'num_freqs': multires,
        'log_sampling': True,
        'periodic_fns': [torch.sin, torch.cos],
    }
    embedder = Embedder(**embed_kwargs)
    return embedder, embedder.out_dim


class DM_NeRF(nn.Module):
    """``DM_NeRF`` (networks/dm_nerf.py:58-106): 8x256 trunk, skip at 4, sigma / rgb / object heads.

    Parameters are ordinary ``nn.Linear`` modules with the reference's names; the fused HIP
    kernel reads a permuted copy ("blob") that is rebuilt whenever a parameter changed.
    """

    def __init__(self, D=8, W=256, input_ch_pts=3, input_ch_views=3, skips=[4], ins_num=None):
        super().__init__()
        self.D, self.W = D, W
        self.skips = skips
        self.input_ch_pts = input_ch_pts
        self.input_ch_views = input_ch_views
        self.ins_num = ins_num
        self.mlps = nn.ModuleList(
            [nn.Linear(input_ch_pts, W)] +
            [nn.Linear(W, W) if i not in skips else nn.Linear(W + input_ch_pts, W) for i in range(D - 1)])
        self.rgb_feature_linear = nn.Linear(W, W)
        self.ins_feature_linear = nn.Linear(W, W)
        self.rgb_feature_linears = nn.ModuleList([nn.Linear(W + input_ch_views, W // 2)])
        self.ins_feature_linears = nn.ModuleList([nn.Linear(W, W // 2)])
        self.density_linear = nn.Linear(W, 1)
        self.ins_linear = nn.Linear(W // 2, ins_num + 1)
        self.rgb_linear = nn.Linear(W // 2, 3)
        self._packed = {}                                   # layout -> (key, tensor): see ``_cached`` (a plain attribute, no buffer)

    # -- kernel-layout weights --------------------------------------------------------------
    def _fused_ok(self):
        """True for the shape every shipped config uses (D=8, W=256, skips=[4], 63+27 input channels; config.py:126-138
        defaults), which the fused register-chained kernels are specialised for.  Any other shape (args.netdepth /
        netwidth / multires*) runs layer by layer on the kernels of csrc/generic.hip (dm_nerf_amd/generic.py)."""
        return (self.D == 8 and self.W == 256 and list(self.skips) == [4]
                and self.input_ch_pts == 63 and self.input_ch_views == 27)

    def _check_supported(self):
        if not self._fused_ok():
            raise NotImplementedError(
                "the packed weight blobs exist for the fused kernels' shape only (D=8, W=256, skips=[4], 63+27 input "
                "channels); other shapes go through dm_nerf_amd.generic")

    def _cached(self, layout):
        """The kernel-layout copy ``layout`` of the weights ("flat", or a key of ``weights.LAYOUTS``): the one made last, or -- when
        a parameter was updated in place or replaced since (see ``invalidate_blobs``) -- a NEW tensor, packed from ``flat()``.  Never
        re-packed in place: a pending backward (two forwards around an optimizer step, ``retain_graph``) keeps the copies ITS forward
        used, so its data gradients and its weight gradients see the same weights.  (``setdefault``: a module pickled whole before
        the cache was one dict has no ``_packed``.)"""
        if layout != "flat":
            self._check_supported()
        key = tuple((p.data_ptr(), p._version) for _, p in self.named_parameters())
        cache = self.__dict__.setdefault("_packed", {})
        ent = cache.get(layout)
        if ent is None or ent[0] != key:
            if layout == "flat":          # registration order: ``weights.PARAM_KEYS`` / ``flat_params`` for the fused kernels' shape
                ent = (key, torch.cat([p.detach().reshape(-1).float() for _, p in self.named_parameters()]))
            else:
                ent = (key, weights.pack(layout, self.flat(), self.ins_num))
            cache[layout] = ent
        return ent[1]

    def invalidate_blobs(self):
        """Forget every cached kernel-layout copy of the weights; the next call re-packs from the parameters.

        The cache is keyed on ``(data_ptr, tensor._version)`` of every parameter, which follows
        ``optimizer.step()``, ``load_state_dict`` and any in-place op on the parameter itself.  Updates made THROUGH
        ``.data`` (``p.data.add_(...)``, hand-written optimizers, EMA / weight-clipping code) do not bump ``_version``:
        call this after them, or the kernels keep using the stale copy."""
        self._packed = {}
        self._generic_net = None                            # the generic path's packed weights (generic.py ``_run``)

    def install_packed(self, flat, blob, blob_t):
        """Adopt kernel-layout copies made elsewhere from the CURRENT parameters (dm_nerf_amd.optim.FlatAdam re-packs all of them
        in the launch that follows its update, csrc/optim.hip::repack_kernel): ``flat()``, ``blob()`` and ``blob_t()`` return them
        until a parameter changes again.  Every other layout is forgotten: an update THROUGH the flat storage does not bump
        ``_version``, their keys could not tell."""
        key = tuple((p.data_ptr(), p._version) for _, p in self.named_parameters())
        self._packed = {"flat": (key, flat), "blob": (key, blob), "blob_t": (key, blob_t)}
        self._generic_net = None

    def flat(self):
        """The parameters as ONE flat f32 vector in state_dict order (what the packers gather from and what the backward's
        head kernels read, csrc/heads.hip); a NEW tensor whenever a parameter changed, so a pending backward keeps the
        vector its forward used."""
        return self._cached("flat")

    def blob(self):
        """Kernel-layout weights of the default f32 kernels (refresh rule: ``_cached``)."""
        return self._cached("blob")

    def blob_fused(self):
        """Inference blob with ``rgb_feature_linear`` / ``ins_feature_linear`` folded into the hidden layers
        (``dm_nerf(..., args)`` with ``args.fuse_heads = True``; same refresh rule as ``blob``)."""
        return self._cached("blob_fused")

    def blob_split(self):
        """Split-bf16 inference blob (``args.mfma_split``; same refresh rule as ``blob``)."""
        return self._cached("blob_split")

    def blob_f16(self):
        """Split-f16 inference blob (``args.mfma_split = "f16x2"``; same refresh rule as ``blob``)."""
        return self._cached("blob_f16")

    def blob_f16_density(self):
        """Split-f16 DENSITY blob (``dmnerf_mlp_fwd_rays_density_f16``): the table, the trunk groups and the ``density_linear`` groups of
        ``blob_f16()``, copied on the device; same refresh rule as ``blob_f16`` (it is keyed on that tensor: re-made whenever that
        blob is re-packed)."""
        src = self.blob_f16()
        ent = self._packed.get("blob_f16_density")
        if ent is None or ent[0] is not src:
            out = torch.empty(int(_lib.load().dmnerf_blob_f16_density_words(self.ins_num)), dtype=torch.float32, device=src.device)
            _lib.launch("dmnerf_blob_f16_density_from_f16", src, self.ins_num, out)
            ent = self._packed["blob_f16_density"] = (src, out)
        return ent[1]

    def blob_t_f16(self):
        """Split-f16 W^T blob of the opt-in data-gradient kernel (training with ``args.mfma_split = "f16x2"``)."""
        return self._cached("blob_t_f16")

    def blob_t_split(self):
        """Split-bf16 W^T blob of the opt-in data-gradient kernel (training with ``args.mfma_split``)."""
        return self._cached("blob_t_split")

    def blob_t(self):
        """W^T blob for the backward data-gradient kernel (same refresh rule as ``blob``)."""
        return self._cached("blob_t")

    def forward(self, x):
        """``[M, 63+27] -> [M, 4 + ins_num + 1]`` = cat[rgb, density, ins] (networks/dm_nerf.py:80-106)."""
        train = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if not self._fused_ok():
            from .. import generic
            if x.requires_grad:
                raise NotImplementedError("dm_nerf_amd: DM_NeRF.forward gives gradients for the parameters only")
            return generic.mlp_embedded(self, x, train)
        if train:
            from .. import autograd
            return autograd.mlp_forward_train(self, x)
        x2 = _lib.f32(x.reshape(-1, x.shape[-1]))
        _lib.require_gpu(x2)
        if x2.shape[-1] != self.input_ch_pts + self.input_ch_views:
            raise ValueError(f"DM_NeRF.forward expects {self.input_ch_pts + self.input_ch_views} input channels")
        M = x2.shape[0]
        out = torch.empty(M, 4 + self.ins_num + 1, dtype=torch.float32, device=x2.device)
        _lib.launch("dmnerf_mlp_fwd_embedded", self.blob(), self.ins_num, x2, M, out)
        return out.reshape(*x.shape[:-1], out.shape[-1])
