"""Argument checks of the entries that take a grid volume (an axis-aligned box of dx x dy x dz cells), entry by entry: return code,
message text, the entry's name as prefix, and which check answers when two arguments are bad at once.  Every call here is refused
(or is an empty batch that launches nothing) before the library touches a device, so the file needs no GPU.  The device pointers
are distinct non-null dummies that no refused call may follow."""
import ctypes
import itertools

import pytest

from dm_nerf_amd import _lib

E_ARG, OK = -1, 0
MAX_LOGITS = 128                       # DMNERF_MAX_LOGITS
MAX_E = 32                             # DMNERF_VOLUME_EDIT_MAX
BIG = (2048, 1024, 1024)               # 2^31 cells
D = [(k + 1) << 24 for k in range(12)]  # device pointers: 16 MiB apart, so volume_edit's overlap test has nothing to say


def f3(v):
    return None if v is None else (ctypes.c_float * 3)(*v)


def i3(v):
    return None if v is None else (ctypes.c_int * 3)(*v)


def u32(n, given=True):
    return (ctypes.c_uint32 * n)() if given else None


def entries(v):
    e = (_lib.VolumeEditEntry * (MAX_E + 1))()
    e[0].kind, e[0].label = v["kind0"], v["C"] if v["label0"] is None else v["label0"]
    return e


def skip_grid(v):
    if not v["grid"]:
        return None
    g = _lib.SkipGridArgs()
    g.lo[:], g.inv_cell[:], g.dims[:], g.outside, g.d_bits = v["lo"], v["inv"], v["dims"], 0, v["d"][11]
    return ctypes.byref(g)


# The arguments of every entry from one dict of values, in the order of the C signature (include/dmnerf_hip.h).
ARGS = {
    "label_trace": lambda v: [v["d"][0], f3(v["lo"]), f3(v["cell"]), f3(v["inv"]), i3(v["dims"]), v["C"], v["d"][1], 1, v["N"], u32(64, v["mask"]),
                              0.0, 1.0, v["d"][2], v["d"][3], v["d"][4], v["d"][5], None],
    "baked_render": lambda v: [v["d"][0], v["d"][1], f3(v["lo"]), f3(v["cell"]), f3(v["inv"]), i3(v["dims"]), v["C"], v["d"][2], 1, v["N"],
                               u32(16, v["mask"]), 0.0, 1.0, 0.0, v["d"][3], v["d"][4], v["d"][5], v["d"][6], v["d"][7], v["d"][8], None],
    "volume_edit": lambda v: [v["d"][0], None, f3(v["lo"]), f3(v["cell"]), f3(v["inv"]), i3(v["dims"]), v["C"], u32(4, v["mask"]), entries(v),
                              v["E"], 0, v["d"][1], None, v["d"][2], v["d"][3], v["d"][4], v["d"][5], None],
    "field_edit_select": lambda v: [v["d"][0], f3(v["lo"]), f3(v["inv"]), i3(v["dims"]), 0, 0, entries(v), v["E"], v["C"], v["d"][1], v["d"][2],
                                    v["d"][3], v["N"], v["S"], v["d"][4], v["d"][5], v["d"][6], v["d"][7], v["d"][8], v["d"][9], v["d"][10],
                                    v["d"][11], None, None],
    "field_edit_filter": lambda v: [v["d"][0], v["d"][1], v["N"], v["C"], u32(4 * (MAX_E + 2), v["mask"]), v["E"], v["d"][2], None, None],
    "skip_select": lambda v: [skip_grid(v), v["d"][0], v["d"][1], v["d"][2], v["N"], v["S"], v["d"][3], v["d"][4], v["d"][5], v["d"][6], None],
    "skip_select_fill": lambda v: [skip_grid(v), v["d"][0], v["d"][1], v["d"][2], v["N"], v["S"], v["d"][3], v["d"][4], v["d"][5], v["d"][6],
                                   v["d"][7], v["d"][8], 17, None, None],
    "skip_grid_mark": lambda v: [skip_grid(v), v["d"][0], v["d"][1], v["d"][2], v["d"][3], v["d"][4], v["N"], v["S"], 0.0, None],
    "skip_grid_build": lambda v: [v["d"][0], *v["dims"], 0.5, v["dilate"], v["d"][1], None],
    "skip_grid_dilate": lambda v: [v["d"][0], *v["dims"], v["dilate"], v["d"][1], None],
    "label_stats": lambda v: [v["d"][0], *v["dims"], v["C"], v["d"][1], v["d"][2], v["d"][3], v["d"][4], None],
    "skip_grid_from_labels": lambda v: [v["d"][0], v["ncells"], u32(4, v["mask"]), v["d"][1], None],
}

# Per entry: `order` lists its checks from the one that answers first, `msg` the text of each (after "<entry>: "), `dev` the number
# of device pointers it requires, `count` the index of the one it wants even for an empty batch.  The checks:
#   nullgrid  the grid struct is null              host    a host array (lo, cell, inv_cell, dims, a mask) is null
#   range     N < 0 / S < 1 / M or n_cells out of range      dims    a dim < 1            cells   2^31 cells or more
#   dilate    dilate outside 0..4                  C       C outside 1..MAX_LOGITS         E       E outside 0..MAX_E
#   kind      entry 0 has kind 3                   label   entry 0 has label C             count   the count pointer is null
#   rows      rows to fill but no fill row
#   empty     N == 0: DMNERF_OK, launches nothing, the other pointers are not looked at    null    a required device pointer is null
DIMS = "bad dims {dims[0]} x {dims[1]} x {dims[2]}"
CELLS = "{cells} cells do not fit int32"
C_RANGE = "C={C} outside 1..128"
E_RANGE = "E={E} outside 0..32"
KIND = "entry 0 has kind {kind0} (0 move, 1 copy, 2 remove)"
LABEL = "entry 0 has label {C} outside [0, {C})"
TABLE = {
    "label_trace": dict(order=("host", "range", "C", "dims", "cells", "empty", "null"), dev=6,
                        msg=dict(host="null pointer", range="bad N={N}", C=C_RANGE, dims=DIMS, cells=CELLS, null="null pointer")),
    "baked_render": dict(order=("host", "range", "C", "dims", "cells", "empty", "null"), dev=9,
                         msg=dict(host="null pointer", range="bad N={N}", C=C_RANGE, dims=DIMS, cells=CELLS, null="null pointer")),
    "volume_edit": dict(order=("host", "dims", "cells", "C", "E", "null", "kind", "label"), dev=6,
                        msg=dict(host="null host array", dims=DIMS, cells=CELLS, C=C_RANGE, E=E_RANGE, null="null pointer", kind=KIND, label=LABEL)),
    "field_edit_select": dict(order=("host", "range", "dims", "cells", "C", "E", "kind", "label", "count", "rows", "empty", "null"), dev=12, count=8,
                              fill=11, nulls=(0, 9),
                              msg=dict(host="null host array", range="bad N={N} S={S}", dims=DIMS, cells=CELLS, C=C_RANGE,
                                       E=E_RANGE, kind=KIND, label=LABEL, count="null pointer", rows="rows without a fill row", null="null pointer")),
    "field_edit_filter": dict(order=("range", "C", "E", "host", "empty", "null"), dev=3,
                              msg=dict(range="bad M={N} (0 <= M < 2^31)", C=C_RANGE, E=E_RANGE, host="null masks", null="null pointer")),
    # (an empty batch of the two selects launches the kernel that zeroes *d_count: it is not called here)
    "skip_select": dict(order=("nullgrid", "range", "dims", "cells", "count", "null"), dev=7, count=5, no_empty=True,
                        msg=dict(nullgrid="null grid", range="bad N={N} S={S}", dims=DIMS, cells=CELLS, count="null pointer",
                                 null="null pointer")),
    "skip_select_fill": dict(order=("nullgrid", "range", "dims", "cells", "count", "rows", "null"), dev=9, count=5, no_empty=True, fill=8,
                             nulls=(0, 6), msg=dict(nullgrid="null grid", range="bad N={N} S={S}", dims=DIMS, cells=CELLS,
                                                    count="null pointer", rows="rows without a fill row, or bad width 17", null="null pointer")),
    "skip_grid_mark": dict(order=("nullgrid", "range", "dims", "cells", "null", "empty"), dev=5,
                           msg=dict(nullgrid="null grid", range="bad N={N} S={S}", dims=DIMS, cells=CELLS,
                                    null="null pointer")),
    "skip_grid_build": dict(order=("dims", "dilate", "cells", "null"), dev=2,
                            msg=dict(dims=DIMS, dilate="dilate {dilate} outside 0..4", cells=CELLS, null="null pointer")),
    "skip_grid_dilate": dict(order=("dims", "dilate", "cells", "null"), dev=2,
                             msg=dict(dims=DIMS, dilate="dilate {dilate} outside 0..4", cells=CELLS, null="null pointer")),
    "label_stats": dict(order=("dims", "cells", "C", "null"), dev=5, msg=dict(dims=DIMS, cells=CELLS, C=C_RANGE, null="null pointer")),
    "skip_grid_from_labels": dict(order=("range", "null"), dev=2, msg=dict(range="bad n_cells={ncells}", null="null pointer")),
}
HOST_ARRAYS = {"label_trace": ("lo", "cell", "inv", "dims", "mask"), "baked_render": ("lo", "cell", "inv", "dims", "mask"),
               "volume_edit": ("lo", "cell", "inv", "dims", "mask"), "field_edit_select": ("lo", "inv", "dims"),
               "field_edit_filter": ("mask",)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def faults_of(name):
    """fault -> (the check it trips, overrides of the good call's values); only faults whose check the entry has."""
    spec = TABLE[name]
    order, n = spec["order"], spec["dev"]
    out = {}
    if "nullgrid" in order:
        out["nullgrid"] = ("nullgrid", {"grid": False})
    for a in HOST_ARRAYS.get(name, ()):
        out["host_" + a] = ("host", {a: None})
    if name == "skip_grid_from_labels":
        out.update(n0=("range", {"ncells": 0}), nbig=("range", {"ncells": 1 << 31}), mask=("null", {"mask": None}))
    elif "range" in order:
        out["nneg"] = ("range", {"N": -1})
        if "{S}" in spec["msg"]["range"]:
            out["szero"] = ("range", {"S": 0})
    if "dims" in order:
        out["dim0"] = ("dims", {"dims": (4, 0, 4)})
        out["cells"] = ("cells", {"dims": BIG})
    if "dilate" in order:
        out["dilate5"] = ("dilate", {"dilate": 5})
    if "C" in order:
        out["c0"] = ("C", {"C": 0})
        out["cbig"] = ("C", {"C": MAX_LOGITS + 1})
    if "E" in order:
        out["e33"] = ("E", {"E": MAX_E + 1})
    if "kind" in order:
        out["kind3"] = ("kind", {"kind0": 3})
        out["labelC"] = ("label", {"label0": None})
    count = spec.get("count")
    if count is not None:
        out["nocount"] = ("count", {"d": [None if k == count else p for k, p in enumerate(D)]})
    if "empty" in order:
        # where the null test comes first the pointers stay; elsewhere all but the count pointer go, to show that nobody looks at them
        keep_all = order.index("null") < order.index("empty")
        kept = (count, spec["fill"] - 1, spec["fill"]) if "rows" in order else (count,)       # (rows to fill want their fill row)
        out["empty"] = ("empty", {"N": 0, "d": [p if (keep_all or k in kept) else None for k, p in enumerate(D)]})
    elif spec.get("no_empty"):
        out["empty_nocount"] = ("count", {"N": 0, "d": [None if k == count else p for k, p in enumerate(D)]})
    if "rows" in order:
        out["nofill"] = ("rows", {"d": [None if k == spec["fill"] else p for k, p in enumerate(D)]})
    for k in spec.get("nulls", (0, n - 1)):
        if k != count:
            out[f"null{k}"] = ("null", {"d": [None if j == k else p for j, p in enumerate(D)]})
    return out


def call(lib, name, over):
    """The entry with good arguments (a 4 x 4 x 4 box, C = 13, two edits, one ray of one sample) except for `over`."""
    v = dict(lo=(0.0, 0.0, 0.0), cell=(0.25, 0.25, 0.25), inv=(4.0, 4.0, 4.0), dims=(4, 4, 4), C=13, E=2, N=1, S=1, kind0=0, label0=0,
             grid=True, mask=True, dilate=1, ncells=64, d=list(D))
    v.update(over)
    rc = getattr(lib, "dmnerf_" + name)(*ARGS[name](v))
    if v["dims"] is not None:
        v["cells"] = v["dims"][0] * v["dims"][1] * v["dims"][2]
    return rc, _lib.last_error(), v


def check(lib, name, chosen):
    """Apply the faults in `chosen` together; the earliest of their checks in the entry's order must answer."""
    spec, faults = TABLE[name], faults_of(name)
    over = {}
    for f in chosen:
        for k, val in faults[f][1].items():
            if k == "d" and "d" in over:
                val = [None if (a is None or b is None) else a for a, b in zip(over["d"], val)]
            elif k in over and over[k] != val:
                return False                                         # two faults want the same argument: not a pair
            over[k] = val
    keys = [faults[f][0] for f in chosen]
    assert keys, "a call with good arguments would launch"
    first = min(keys, key=spec["order"].index)
    rc, msg, v = call(lib, name, over)
    if first == "empty":
        assert rc == OK, (name, chosen, rc, msg)
    else:
        want = f"{name}: " + spec["msg"][first].format(**v)
        assert (rc, msg) == (E_ARG, want), (name, chosen, rc, msg, want)
    return True


def test_table_covers_every_entry_that_takes_a_box():
    assert set(TABLE) == set(ARGS)
    for name in TABLE:
        v = dict(lo=(0.0,) * 3, cell=(1.0,) * 3, inv=(1.0,) * 3, dims=(1, 1, 1), C=1, E=0, N=1, S=1, kind0=0, label0=0, grid=True, mask=True,
                 dilate=0, ncells=1, d=list(D))
        assert len(ARGS[name](v)) == len(_lib.SIGNATURES["dmnerf_" + name][1]), name
        assert TABLE[name]["dev"] <= len(D)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_each_bad_argument_alone(lib, name):
    for f in faults_of(name):
        assert check(lib, name, (f,))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_which_check_answers_when_two_arguments_are_bad(lib, name):
    n = sum(check(lib, name, pair) for pair in itertools.combinations(faults_of(name), 2))
    assert n >= len(faults_of(name)), (name, n)
