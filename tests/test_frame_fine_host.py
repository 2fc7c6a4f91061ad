"""Host-side checks (no GPU) of the fine-only frame path: the three new entry points validate their arguments before any device
is touched, and the density-only kernel's claim on the weight blob -- it reads the ordinary forward blob with the offsets of
``make_layout(ins_num)`` and is handed the fused-heads blob under ``args.fuse_heads`` -- holds for every offset it uses."""
import ctypes

import numpy as np
import pytest

from dm_nerf_amd import _lib, weights as W

TAB, QUARTER = 4096, 16384
TRUNK_QUARTERS = 1 + 5 * 4 + 1 + 2 * 4                 # w0 | st0..st4 | w5pe | st5 st6 (csrc/layout.h)


def test_new_entries_validate_arguments_before_touching_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(16)                                        # a non-null pointer that is never dereferenced
    rc = lib.dmnerf_mlp_fwd_rays_density(None, 13, None, None, None, 4, 64, None, None)
    assert rc == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_mlp_fwd_rays_density(one, 0, one, one, one, 4, 64, one, None) == -1 and "ins_num" in _lib.last_error()
    assert lib.dmnerf_mlp_fwd_rays_density(one, 200, one, one, one, 4, 64, one, None) == -1
    assert lib.dmnerf_mlp_fwd_rays_density(one, 13, one, one, one, -1, 64, one, None) == -1
    assert lib.dmnerf_mlp_fwd_rays_density(one, 13, one, one, one, 4, 0, one, None) == -1
    assert lib.dmnerf_mlp_fwd_rays_density(None, 13, None, None, None, 0, 64, None, None) == 0        # an empty batch is legal

    rc = lib.dmnerf_weights_from_sigma(None, None, None, 4, 64, None, None)
    assert rc == -1 and "null" in _lib.last_error()
    assert lib.dmnerf_weights_from_sigma(one, one, one, 4, 0, one, None) == -1
    assert lib.dmnerf_weights_from_sigma(one, one, one, -2, 64, one, None) == -1
    assert lib.dmnerf_weights_from_sigma(one, one, one, 4, 1 << 20, one, None) == -1
    assert lib.dmnerf_weights_from_sigma(None, None, None, 0, 64, None, None) == 0

    assert lib.dmnerf_render_rays_fwd_fine(None, None) == -1 and "null args" in _lib.last_error()
    a = _lib.RenderFineArgs()
    a.ins_num, a.N, a.S, a.n_imp = 13, 4, 64, 128
    rc = lib.dmnerf_render_rays_fwd_fine(ctypes.byref(a), None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    for name, _ in _lib.RenderFineArgs._fields_:
        if name.startswith("d_") and name != "d_t_rand":
            setattr(a, name, 16)
    for bad in (dict(S=2), dict(n_imp=0), dict(N=-1), dict(fused_heads=2), dict(fused_heads=3)):
        b = _lib.RenderFineArgs()
        ctypes.memmove(ctypes.byref(b), ctypes.byref(a), ctypes.sizeof(a))
        for k, v in bad.items():
            setattr(b, k, v)
        assert lib.dmnerf_render_rays_fwd_fine(ctypes.byref(b), None) == -1, bad
    e = _lib.RenderFineArgs()
    e.ins_num, e.N, e.S, e.n_imp = 13, 0, 64, 128                    # an empty chunk: its buffers may be null
    assert lib.dmnerf_render_rays_fwd_fine(ctypes.byref(e), None) == 0


def test_render_args_of_the_full_path_keep_their_layout():
    """The new entry is additive: ``dmnerf_render_args`` is the struct it was (26 fields, 200 bytes) and the ABI number stays."""
    assert ctypes.sizeof(_lib.RenderArgs) == 200 and len(_lib.RenderArgs._fields_) == 26
    assert _lib.load().dmnerf_abi_version() == 8


@pytest.mark.parametrize("ins_num", [13, 59, 93])
def test_default_and_fused_blob_agree_on_everything_the_density_kernel_reads(ins_num):
    a, b = W.pack_index_host(ins_num), W.pack_index_fused_host(ins_num)
    obi = (ins_num + 1 + 31) // 32
    b0, b_stage = 0, 256
    w_den = 256 + 9 * 256 + 128 + 128 + 32 * obi                     # layout.h::make_layout, the same for fused = false / true
    b_den = w_den + 256
    used = np.r_[b0:b0 + 256, b_stage:b_stage + 7 * 256, w_den:w_den + 256, b_den:b_den + 1]
    assert used.max() < TAB
    assert np.array_equal(a[used], b[used])
    assert (a[used] >= 0).all()                                      # every one of them is a parameter, none is padding
    # density_linear.weight / .bias are what sits at w_den / b_den: [half][128] in accumulator order + the bias
    base = int(a[w_den:w_den + 256].min())
    assert sorted(a[w_den:w_den + 256] - base) == list(range(256)) and a[b_den] == base + 256
    # the trunk: 30 quarters, the same gather indices in both blobs
    end = TAB + TRUNK_QUARTERS * QUARTER
    assert np.array_equal(a[TAB:end], b[TAB:end])
    # the look-ahead fetch of the last trunk quarter lands inside both blobs
    assert len(a) >= end + QUARTER and len(b) >= end + QUARTER
