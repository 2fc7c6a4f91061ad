"""The numpy restatement of the grid from rendered views (tests/_mark_restate.py) against the restatement of the skip grid and
hand-built cases -- the GPU tests compare the kernels with it, so it is checked on its own first -- the pure-torch OR of the words
gathered from the ranks, and the ABI of the two new entries."""
import os
import re

import numpy as np
import pytest
import torch

import _mark_restate as RM
import _skip_restate as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (33, 8, 40)])
@pytest.mark.parametrize("r", [0, 1, 4])
def test_dilation_of_words_equals_the_dilation_of_cells(dims, r):
    rng = np.random.RandomState(dims[0] + r)
    cases = [np.zeros(dims, bool), np.ones(dims, bool)]
    if dims == (33, 8, 40):
        occ = np.zeros(dims, bool)
        for c in ((0, 0, 0), (32, 7, 39), (16, 0, 20), (5, 7, 0), (20, 3, 39)):     # two corners, two faces, an edge
            occ[c] = True
        occ |= rng.rand(*dims) < 0.002
        cases.append(occ)
        ref = RS.dilate_clipped_fast                                  # (test_skip_restate checks it against the loops)
    else:
        cases.append(rng.rand(*dims) < 0.1)
        ref = RS.dilate_clipped
    for occ in cases:
        got = RM.dilate(RS.pack_bits(occ), dims, r)
        assert got.dtype == np.uint32 and np.array_equal(got, RS.pack_bits(ref(occ, r)))
        tail = (dims[0] * dims[1] * dims[2]) & 31
        if tail:
            assert int(got[-1]) >> tail == 0


def mark_case(seed=0, n=6, s=9):
    """Box [0, 2)^3 in 0.5 cells (every product exact on the hand-placed samples).  Rays 0 and 1 are hand-placed, the others random."""
    dims, lo, hi = (4, 4, 4), (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)
    rng = np.random.RandomState(seed)
    o = (rng.rand(n, 3) * 2.0 - 0.2).astype(np.float32)
    d = (rng.rand(n, 3) - 0.3).astype(np.float32)
    z = np.sort((rng.rand(n, s) * 2.0).astype(np.float32), -1)
    w = (rng.rand(n, s) * (rng.rand(n, s) < 0.5)).astype(np.float32)
    o[0], d[0] = (0.0, 0.25, 0.25), (1.0, 0.0, 0.0)
    z[0] = [0.0, 0.5, 0.75, 1.0, 1.99, 2.0, 3.0, -0.25, 1.25]       # on lo: cell 0; on a boundary: cell 1; 1; 2; 3; on hi, beyond, below: outside; 2
    w[0] = [1.0, 0.0, -0.0, 0.25, np.nan, 1.0, 1.0, 1.0, np.nextafter(np.float32(0.25), np.float32(1))]
    o[1], d[1] = (np.nan, 0.25, 0.25), (1.0, 0.0, 0.0)               # a NaN point is outside whatever its weight
    w[1] = 1.0
    return dims, lo, hi, o, d, z, w


def cells(words, dims):
    return {tuple(int(v) for v in c) for c in np.argwhere(RS.unpack_bits(words, dims))}


def test_mark_by_hand():
    dims, lo, hi, o, d, z, w = mark_case()
    empty = np.zeros(2, np.uint32)
    one = lambda thr: cells(RM.mark(empty, o[:2], d[:2], z[:2], w[:2], lo, hi, dims, thr), dims)
    # threshold 0: weights 0 and -0.0 do not mark (cell 1 stays clear), NaN marks (cell 3), the three outside samples mark nothing
    assert one(0.0) == {(0, 0, 0), (2, 0, 0), (3, 0, 0)}
    # threshold 0.25: a weight of exactly 0.25 does not mark, the next float does (both fall into cell 2)
    assert one(0.25) == {(0, 0, 0), (2, 0, 0), (3, 0, 0)}
    w2 = w.copy()
    w2[0, 8] = 0.25
    assert cells(RM.mark(empty, o[:2], d[:2], z[:2], w2[:2], lo, hi, dims, 0.25), dims) == {(0, 0, 0), (3, 0, 0)}
    assert not empty.any()                                           # the input words are not written


def test_mark_is_monotone_idempotent_and_order_independent():
    dims, lo, hi, o, d, z, w = mark_case(seed=4, n=8)
    rng = np.random.RandomState(9)
    pre = RS.pack_bits(rng.rand(*dims) < 0.1)
    for thr in (0.0, 0.3):
        got = RM.mark(pre, o, d, z, w, lo, hi, dims, thr)
        assert np.array_equal(got & pre, pre)                        # monotone: what was set stays
        assert np.array_equal(got, RM.mark(np.zeros_like(pre), o, d, z, w, lo, hi, dims, thr) | pre)
        assert np.array_equal(RM.mark(got, o, d, z, w, lo, hi, dims, thr), got)                     # idempotent
        # the samples in another order: rays permuted, and the samples along every ray permuted
        pr, ps = rng.permutation(o.shape[0]), rng.permutation(z.shape[1])
        assert np.array_equal(RM.mark(pre, o[pr], d[pr], z[pr][:, ps], w[pr][:, ps], lo, hi, dims, thr), got)
        # a chunk at a time
        step = RM.mark(RM.mark(pre, o[:3], d[:3], z[:3], w[:3], lo, hi, dims, thr), o[3:], d[3:], z[3:], w[3:], lo, hi, dims, thr)
        assert np.array_equal(step, got)
    lo_thr, hi_thr = (RM.mark(pre, o, d, z, w, lo, hi, dims, t) for t in (0.0, 0.3))
    assert np.array_equal(hi_thr & lo_thr, hi_thr) and not np.array_equal(hi_thr, lo_thr) and not np.array_equal(lo_thr, pre)


@pytest.mark.parametrize("world", [1, 2, 7])
def test_or_of_gathered_words(world):
    from dm_nerf_amd import field
    n_words = 37                                                     # an odd word count
    rng = np.random.RandomState(world)
    parts = rng.randint(0, 2 ** 32, size=(world, n_words), dtype=np.uint64).astype(np.uint32)
    parts &= rng.randint(0, 2 ** 32, size=(world, n_words), dtype=np.uint64).astype(np.uint32)     # about a quarter of the bits
    want = np.bitwise_or.reduce(parts, axis=0)
    gathered = torch.from_numpy(parts.view(np.int32).reshape(-1).copy())
    keep = gathered.clone()
    got = field.or_gathered_words(gathered, world)
    assert got.dtype == torch.int32 and got.shape == (n_words,)
    assert np.array_equal(got.numpy().view(np.uint32), want)
    assert torch.equal(gathered, keep)                               # the gathered buffer is left alone
    if world > 1:
        assert not np.array_equal(want, parts[0])
        with pytest.raises(ValueError):
            field.or_gathered_words(gathered[:-1], world)


def test_header_declares_and_library_exports_the_two_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmnerf_hip.h")).read(), flags=re.S)
    from dm_nerf_amd import _lib
    lib = _lib.load()
    for name, n_args in (("dmnerf_skip_grid_mark", 10), ("dmnerf_skip_grid_dilate", 7)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, f"{name} is not declared in include/dmnerf_hip.h"
        assert len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1])
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.dmnerf_abi_version() == 8                             # additive: the version stays


def test_the_two_entries_refuse_bad_arguments_before_any_launch():
    """Host-side checks only: every call here returns before it touches a device."""
    import ctypes
    from dm_nerf_amd import _lib
    lib = _lib.load()
    g = _lib.SkipGridArgs()
    for a in range(3):
        g.lo[a], g.inv_cell[a], g.dims[a] = 0.0, 1.0, 2
    P = ctypes.c_void_p(256)                                         # never dereferenced
    mark = lambda grid=ctypes.byref(g), bits=P, o=P, N=4, S=8, thr=0.0: lib.dmnerf_skip_grid_mark(grid, bits, o, P, P, P, N, S, thr, None)
    for kw, text in ((dict(grid=None), "null grid"), (dict(bits=None), "null pointer"), (dict(o=None), "null pointer"),
                     (dict(S=0), "bad N=4 S=0"), (dict(N=-1), "bad N=-1"), (dict(N=1 << 20, S=1 << 11), "do not fit"),
                     (dict(thr=float("nan")), "threshold"), (dict(thr=-1e-6), "threshold")):
        assert mark(**kw) == -1 and text in _lib.last_error(), (kw, _lib.last_error())
    assert mark(N=0) == 0                                            # nothing to mark: no launch
    dil = lambda i=P, o=ctypes.c_void_p(512), dims=(2, 2, 2), r=1: lib.dmnerf_skip_grid_dilate(i, *dims, r, o, None)
    for kw, text in ((dict(i=None), "null pointer"), (dict(o=None), "null pointer"), (dict(o=P), "different buffers"),
                     (dict(r=5), "outside 0..4"), (dict(r=-1), "outside 0..4"), (dict(dims=(0, 2, 2)), "bad dims"),
                     (dict(dims=(2048, 1024, 1024)), "do not fit int32")):
        assert dil(**kw) == -1 and text in _lib.last_error(), (kw, _lib.last_error())
