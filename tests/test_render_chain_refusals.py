"""The refusals of the three inference chains of the C ABI (csrc/api.hip: ``dmnerf_render_rays_fwd``, ``.._fwd_fine``,
``.._fwd_fine_skip``): return code, full text and the order in which the checks answer.  Every call here is refused, or is an
empty chunk, before the library touches a device, so the file needs no GPU.

Each entry's checks are walked in their order.  The call for check k satisfies every check before k and violates k and, as far as
one set of arguments can, every check after it; check k must be the one that answers.  (Two checks cannot always be violated
together: the "twice" refusal wants ``fused_heads == 3``, which the ``fused_heads`` check accepts.)  The skip entry is never
called with ``N == 0`` and a non-null ``d_n_eval``: that path writes the two counters on the device."""
import ctypes

import pytest

from dm_nerf_amd import _lib

E_ARG, OK = -1, 0
P, Q = 16, 32                          # non-null pointers that no refused call may follow
OPTIONAL = ("d_t_rand",)               # (the two event handles do not start with d_)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def pointers(cls):
    return [n for n, _ in cls._fields_ if n.startswith("d_") and n not in OPTIONAL]


def fill(a, ptr, **kw):
    """Every required pointer of the struct `a` = ptr (None: null), then the fields of `kw`."""
    for n in pointers(type(a)):
        setattr(a, n, ptr)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def answer(fn, a):
    rc = fn(ctypes.byref(a) if a is not None else None, None)
    return rc, _lib.last_error()


# ---- dmnerf_render_rays_fwd: null args | empty chunk | null pointers | range -------------------------------------------------------
def test_render_rays_fwd(lib):
    fn, A = lib.dmnerf_render_rays_fwd, _lib.RenderArgs
    null, bad = "render_rays_fwd: null pointer in args", "render_rays_fwd: bad N={} S={} n_imp={}"
    assert answer(fn, None) == (E_ARG, "render_rays_fwd: null args")
    # null pointers, with the range violated as well (S = 2 also keeps an N = 0 call from being an empty chunk)
    for kw in (dict(N=-1, S=2, n_imp=0), dict(N=0, S=2, n_imp=1), dict(N=0, S=3, n_imp=0), dict(N=33, S=3, n_imp=2)):
        assert answer(fn, fill(A(), None, ins_num=13, **kw)) == (E_ARG, null), kw
    for name in pointers(A):
        a = fill(A(), P, ins_num=13, N=-1, S=2, n_imp=0)
        setattr(a, name, None)
        assert answer(fn, a) == (E_ARG, null), name
    # range
    for N, S, n_imp in ((-1, 3, 1), (33, 2, 1), (33, 3, 0), (0, 2, 1), (0, 3, 0), (-5, 0, -1)):
        assert answer(fn, fill(A(), P, ins_num=13, N=N, S=S, n_imp=n_imp)) == (E_ARG, bad.format(N, S, n_imp))
    # fused_heads is not validated: nothing but the checks above answers for any value
    for fused in (-1, 2, 3, 7):
        assert answer(fn, fill(A(), P, ins_num=13, N=-1, S=3, n_imp=1, fused_heads=fused)) == (E_ARG, bad.format(-1, 3, 1))
    # an empty chunk returns before any pointer is looked at, whatever fused_heads and ins_num say
    for ptr, fused, ins in ((None, 0, 13), (P, 0, 13), (None, 3, 13), (None, 9, 0)):
        assert answer(fn, fill(A(), ptr, ins_num=ins, N=0, S=3, n_imp=1, fused_heads=fused))[0] == OK


# ---- dmnerf_render_rays_fwd_fine: null args | fused_heads | empty chunk | null pointers | range | one blob twice -------------------
def test_render_rays_fwd_fine(lib):
    fn, A = lib.dmnerf_render_rays_fwd_fine, _lib.RenderFineArgs
    who = "render_rays_fwd_fine"
    fused_text = who + ": fused_heads {} unsupported (the split-operand blobs go through dmnerf_render_rays_fwd)"
    null, bad = who + ": null pointer in args", who + ": bad N={} S={} n_imp={}"
    twice = who + ": fused_heads 3 wants the f16 density blob as d_blob_coarse, got d_blob_fine twice"
    assert answer(fn, None) == (E_ARG, who + ": null args")
    # fused_heads, with null pointers (both blobs the same null), a bad range and even an empty chunk behind it
    for fused in (2, -1, 4):
        for kw in (dict(N=-1, S=2, n_imp=0), dict(N=0, S=3, n_imp=1)):
            assert answer(fn, fill(A(), None, ins_num=13, fused_heads=fused, **kw)) == (E_ARG, fused_text.format(fused)), (fused, kw)
    # null pointers, with the range violated and d_blob_coarse == d_blob_fine under fused_heads 3
    for kw in (dict(N=-1, S=2, n_imp=0), dict(N=0, S=2, n_imp=1), dict(N=33, S=3, n_imp=2)):
        assert answer(fn, fill(A(), None, ins_num=13, fused_heads=3, **kw)) == (E_ARG, null), kw
    for name in pointers(A):
        a = fill(A(), P, ins_num=13, fused_heads=3, N=-1, S=2, n_imp=0)
        setattr(a, name, None)
        assert answer(fn, a) == (E_ARG, null), name
    # range, with the one blob given twice
    for N, S, n_imp in ((-1, 3, 1), (33, 2, 1), (33, 3, 0), (0, 2, 1)):
        assert answer(fn, fill(A(), P, ins_num=13, fused_heads=3, N=N, S=S, n_imp=n_imp)) == (E_ARG, bad.format(N, S, n_imp))
    # one blob twice: the last check
    assert answer(fn, fill(A(), P, ins_num=13, fused_heads=3, N=33, S=3, n_imp=2)) == (E_ARG, twice)
    # an empty chunk returns before any pointer is looked at, in every legal mode
    for ptr in (None, P):
        for fused in (0, 1, 3):
            assert answer(fn, fill(A(), ptr, ins_num=13, N=0, S=3, n_imp=1, fused_heads=fused))[0] == OK


# ---- dmnerf_render_rays_fwd_fine_skip: null args | fused_heads | levels | range | int32 bound | null d_n_eval | (N == 0) |
# null pointers | one blob twice --------------------------------------------------------------------------------------------
SKIP_POINTERS = ("d_sel", "d_flag", "d_select_ws")


def skip_args(ptr, d_n_eval, levels, **fine):
    k = _lib.RenderFineSkipArgs()
    fill(k.fine, ptr, ins_num=13, **fine)
    for n in SKIP_POINTERS:
        setattr(k, n, ptr)
    k.grid.d_bits = ptr
    k.d_n_eval, k.levels = d_n_eval, levels
    return k


def test_render_rays_fwd_fine_skip(lib):
    fn = lib.dmnerf_render_rays_fwd_fine_skip
    who = "render_rays_fwd_fine_skip"
    fused_text = who + ": fused_heads {} unsupported (no split-operand kernels over a selection)"
    null = who + ": null pointer in args"
    twice = who + ": fused_heads 3 wants the f16 density blob as d_blob_coarse, got d_blob_fine twice"
    big = dict(N=1 << 30, S=2, n_imp=1)                              # violates the range (S < 3) AND the int32 bound (N * SF = 3 * 2^30)
    assert answer(fn, None) == (E_ARG, who + ": null args")
    for fused in (2, -1, 4):
        assert answer(fn, skip_args(None, None, 8, fused_heads=fused, **big)) == (E_ARG, fused_text.format(fused))
    for levels in (4, 8, -1, 7):
        assert answer(fn, skip_args(None, None, levels, fused_heads=3, **big)) == (E_ARG, f"{who}: bad levels mask {levels}")
    for N, S, n_imp in ((1 << 30, 2, 1), (-1, 3, 1), (1 << 31, 3, 0), (1 << 31, 2, 1)):
        assert answer(fn, skip_args(None, None, 3, fused_heads=3, N=N, S=S, n_imp=n_imp)) == (E_ARG, f"{who}: bad N={N} S={S} n_imp={n_imp}")
    for N, S, n_imp in ((1 << 30, 3, 1), (1 << 29, 3, 1), (1 << 31, 64, 128)):
        assert answer(fn, skip_args(None, None, 3, fused_heads=3, N=N, S=S, n_imp=n_imp)) == \
            (E_ARG, f"{who}: {N * (S + n_imp)} samples do not fit the int32 selection")
    # null d_n_eval: before the empty chunk (N = 0 with it null is refused, not written) and before the other pointers
    for ptr in (None, P):
        for N in (0, 33):
            for levels in (0, 1, 2, 3):
                assert answer(fn, skip_args(ptr, None, levels, fused_heads=3, N=N, S=3, n_imp=2)) == (E_ARG, null), (ptr, N, levels)
    # null pointers, d_n_eval given, the one blob twice (where both blobs are given)
    assert answer(fn, skip_args(None, Q, 3, fused_heads=3, N=33, S=3, n_imp=2)) == (E_ARG, null)
    for name in pointers(_lib.RenderFineArgs) + list(SKIP_POINTERS) + ["d_bits"]:
        k = skip_args(P, Q, 3, fused_heads=3, N=33, S=3, n_imp=2)
        setattr(k.grid if name == "d_bits" else k if name in SKIP_POINTERS else k.fine, name, None)
        assert answer(fn, k) == (E_ARG, null), name
    # one blob twice: the last check, whichever levels are skipped
    for levels in (0, 1, 2, 3):
        assert answer(fn, skip_args(P, Q, levels, fused_heads=3, N=33, S=3, n_imp=2)) == (E_ARG, twice)
