"""Host-side checks of the f16x2 density-only / selection entries: symbols, the density blob's size and the argument checks, which
run before anything touches a device."""
import ctypes

import pytest

from dm_nerf_amd import _lib

NEW = ("dmnerf_blob_f16_density_words", "dmnerf_blob_f16_density_from_f16", "dmnerf_mlp_fwd_rays_density_f16",
       "dmnerf_mlp_fwd_rays_f16_sel", "dmnerf_mlp_fwd_rays_density_f16_sel")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_new_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.restype == _lib.SIGNATURES[name][0]
    assert lib.dmnerf_abi_version() == 8


def test_density_blob_words(lib):
    # the 4096-float table + (120 trunk + 2 density + 6 landing) groups of 4096 words
    assert lib.dmnerf_blob_f16_density_words(13) == 4096 + (122 + 6) * 4096
    assert lib.dmnerf_blob_f16_density_words(13) < lib.dmnerf_blob_f16_words(13)
    assert lib.dmnerf_blob_f16_density_words(0) == -1 and lib.dmnerf_blob_f16_density_words(500) == -1


P = ctypes.c_void_p(64)                # a non-null pointer that no rejected call may follow


def calls(lib):
    """name -> f(ptr, N, S): the entry with every pointer = ptr."""
    return {
        "mlp_fwd_rays_density_f16": lambda p, N, S, ins=13: lib.dmnerf_mlp_fwd_rays_density_f16(p, ins, p, p, p, N, S, p, None),
        "mlp_fwd_rays_f16_sel": lambda p, N, S, ins=13: lib.dmnerf_mlp_fwd_rays_f16_sel(p, ins, p, p, p, N, S, p, p, p, None),
        "mlp_fwd_rays_density_f16_sel": lambda p, N, S, ins=13: lib.dmnerf_mlp_fwd_rays_density_f16_sel(p, ins, p, p, p, N, S, p, p, p, None),
    }


@pytest.mark.parametrize("name", ["mlp_fwd_rays_density_f16", "mlp_fwd_rays_f16_sel", "mlp_fwd_rays_density_f16_sel"])
def test_argument_checks_run_before_any_device_work(lib, name):
    f = calls(lib)[name]
    assert f(None, 4, 8) == -1 and name in _lib.last_error() and "null pointer" in _lib.last_error()
    assert f(P, 4, 0) == -1 and "bad N=4 S=0" in _lib.last_error()
    assert f(P, -1, 8) == -1 and "bad N=-1" in _lib.last_error()
    assert f(P, 4, 8, ins=0) == -1 and "ins_num 0" in _lib.last_error()
    assert f(P, 4, 8, ins=500) == -1 and "ins_num 500" in _lib.last_error()
    assert f(None, 0, 8) == 0                                        # an empty batch: its buffers may be null
    if name.endswith("_sel"):
        assert f(P, 1 << 20, 1 << 11) == -1 and "int32" in _lib.last_error()


def test_density_blob_copy_checks_its_arguments(lib):
    assert lib.dmnerf_blob_f16_density_from_f16(None, 13, None, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.dmnerf_blob_f16_density_from_f16(P, 0, P, None) == -1 and "ins_num 0" in _lib.last_error()


def test_chains_still_refuse_bf16x3(lib):
    a = _lib.RenderFineArgs()
    a.fused_heads = 2
    a.N, a.S, a.n_imp, a.ins_num = 4, 8, 4, 13
    assert lib.dmnerf_render_rays_fwd_fine(ctypes.byref(a), None) == -1
    assert "fused_heads 2 unsupported" in _lib.last_error() and "render_rays_fwd_fine:" in _lib.last_error()
    k = _lib.RenderFineSkipArgs()
    k.fine = a
    assert lib.dmnerf_render_rays_fwd_fine_skip(ctypes.byref(k), None) == -1
    assert "fused_heads 2 unsupported" in _lib.last_error() and "no split-operand kernels over a selection" in _lib.last_error()
    a.fused_heads = 3                                                # accepted: the next check (null pointers) answers
    assert lib.dmnerf_render_rays_fwd_fine(ctypes.byref(a), None) == -1 and "null pointer" in _lib.last_error()
