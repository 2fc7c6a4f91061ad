"""``_lib.call`` / ``_lib.launch``: the two helpers every library call of the package goes through.  Host tests (argument
conversion, status check, the stream appended at call time, which helper each call site may use); one GPU test at the end."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from dm_nerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dmnerf_hip.h")
PACKAGE = os.path.join(ROOT, "dm_nerf_amd")


def declarations():
    """name -> (return type, parameter list) of every function include/dmnerf_hip.h declares (comments stripped, as test_abi.py)."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\s*\b(dmnerf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        out[name] = (" ".join(ret.split()), " ".join(params.split()))
    return out


def takes_stream(params):
    return re.search(r"void\s*\*\s*stream$", params) is not None


@pytest.fixture
def null_stream(monkeypatch):
    monkeypatch.setattr(_lib, "stream", lambda: ctypes.c_void_p(0))


@pytest.mark.parametrize("ins_num", [13, 1])             # 1: the smallest the library accepts (pack.cpp: ins_num < 1 is refused)
def test_call_fills_numpy_and_cpu_tensor_like_the_direct_call(ins_num):
    lib = _lib.load()
    n = lib.dmnerf_blob_floats(ins_num)
    assert n > 0 and lib.dmnerf_blob_floats(0) == -1
    want = np.full(n, -7, dtype=np.int32)
    assert lib.dmnerf_build_pack_index(ins_num, want.ctypes.data_as(ctypes.c_void_p), n) == 0
    got_np = np.full(n, -7, dtype=np.int32)
    assert _lib.call("dmnerf_build_pack_index", ins_num, got_np, n) is None
    assert np.array_equal(got_np, want)
    got_t = torch.full((n,), -7, dtype=torch.int32)
    _lib.call("dmnerf_build_pack_index", ins_num, got_t, n)
    assert np.array_equal(got_t.numpy(), want)
    assert (want != -7).all()                               # (the direct call did fill it)


def test_call_refuses_like_the_direct_call():
    n = _lib.load().dmnerf_blob_floats(13)
    with pytest.raises(RuntimeError, match=r"dmnerf_build_pack_index failed \(code -1\)"):
        _lib.call("dmnerf_build_pack_index", 0, np.empty(n, dtype=np.int32), n)


def test_none_is_null():
    assert _lib.call("dmnerf_wgrad_set_trace", None) is None


def test_launch_appends_the_stream_and_raises_todays_message(null_stream):
    with pytest.raises(RuntimeError, match=r"dmnerf_composite_fwd failed \(code -1\)") as e:
        _lib.launch("dmnerf_composite_fwd", None, None, None, 4, 64, 14, None, None, None, None)
    assert "null" in str(e.value)
    assert str(e.value) == f"dmnerf_composite_fwd failed (code -1): {_lib.last_error()}"


def test_launch_fetches_the_stream_at_call_time(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "stream", lambda: (seen.append(1), ctypes.c_void_p(0))[1])
    for _ in range(2):
        with pytest.raises(RuntimeError):
            _lib.launch("dmnerf_composite_fwd", None, None, None, 4, 64, 14, None, None, None, None)
    assert len(seen) == 2


def test_structure_goes_by_reference(null_stream):
    with pytest.raises(RuntimeError, match=r"dmnerf_render_rays_fwd_fine failed") as e:
        _lib.launch("dmnerf_render_rays_fwd_fine", _lib.RenderFineArgs())
    assert "null pointer" in str(e.value)


def test_wrong_argument_count_is_refused_by_ctypes(null_stream):
    before = _lib.last_error()
    with pytest.raises(TypeError):
        _lib.call("dmnerf_build_pack_index", 13)
    with pytest.raises(TypeError):
        _lib.launch("dmnerf_composite_fwd", None, None, None, 4, 64, 14, None, None, None)         # one short, stream included
    assert _lib.last_error() == before                      # the library was not entered


def test_every_call_site_uses_the_helper_its_entry_needs():
    decl = declarations()
    assert set(decl) == set(_lib.SIGNATURES)
    assert sum(1 for r, p in decl.values() if r == "int" and takes_stream(p)) == 107
    sites = 0
    for path in sorted(glob.glob(os.path.join(PACKAGE, "**", "*.py"), recursive=True)):
        src = open(path).read()
        rel = os.path.relpath(path, ROOT)
        if os.path.basename(path) != "_lib.py":
            assert "_lib.check(" not in src, f"{rel}: _lib.check( -- use _lib.launch / _lib.call"
        for helper, name in re.findall(r"_lib\.(launch|call)\(\s*\"(dmnerf_[a-z0-9_]+)\"", src):
            assert name in decl, f"{rel}: {name} is not declared in include/dmnerf_hip.h"
            ret, params = decl[name]
            sites += 1
            if helper == "launch":
                assert takes_stream(params), f"{rel}: _lib.launch(\"{name}\") but its last parameter is not void* stream"
            else:
                assert not takes_stream(params) and ret == "int", f"{rel}: _lib.call(\"{name}\") needs a host-only entry returning int"
    # the entries that dm_nerf_amd/weights.py names in its tables instead of at a call site: index and plan entries go through
    # _lib.call, stream packers and kernel entries through _lib.launch
    from dm_nerf_amd import weights
    by_table = [("call", f_index) for _, _, f_index, _, _ in weights.LAYOUTS.values()]
    by_table += [("launch", f_stream) for _, _, _, _, f_stream in weights.LAYOUTS.values()]
    for v in weights.VARIANTS.values():
        by_table += [("launch", v.fwd), ("launch", v.fwd_train), ("launch", v.dgrad), ("launch", v.wgrad), ("call", v.plan[0]), ("call", v.plan[1])]
    for helper, name in by_table:
        assert name in decl, f"weights.py: {name} is not declared in include/dmnerf_hip.h"
        ret, params = decl[name]
        sites += 1
        assert ret == "int" and takes_stream(params) == (helper == "launch"), f"weights.py: {name} is not an entry for _lib.{helper}"
    assert sites >= 100                                     # (the scan did see the package)


@pytest.mark.gpu
def test_launch_equals_the_spelled_out_idiom_eagerly_and_captured():
    """dmnerf_stratify at N = 3, S = 5 (odd, below one wave, a tail in every dimension): ``launch`` is bit-equal to the
    check / ptr / stream idiom, and the same launch captured in a graph (one kernel node, no parallel branches) replays to the same
    bits -- a stream fetched before the capture began would not be the capturing one and the capture would fail."""
    N, S = 3, 5
    g = torch.Generator().manual_seed(5)
    z = (2.0 + 4.0 * torch.rand(N, S, generator=g)).sort(dim=1).values.cuda()
    t = torch.rand(N, S, generator=g).cuda()
    old, new, cap = (torch.full((N, S), float("nan"), device="cuda") for _ in range(3))
    _lib.check(_lib.load().dmnerf_stratify(_lib.ptr(z), _lib.ptr(t), N, S, _lib.ptr(old), _lib.stream()), "dmnerf_stratify")
    _lib.launch("dmnerf_stratify", z, t, N, S, new)
    torch.cuda.synchronize()
    assert not torch.isnan(old).any() and torch.equal(old, new)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.launch("dmnerf_stratify", z, t, N, S, cap)
    cap.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, new)
