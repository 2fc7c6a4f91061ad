"""Argument checks of the connected-component entries (csrc/components.hip), as tests/test_grid_entry_validation.py makes them of the
other entries that take a grid volume: return code, message text with the entry's name as prefix, and which check answers when two
arguments are bad at once.  Every call here is refused before the library touches a device, so the file needs no GPU.  The device
pointers are distinct non-null dummies that no refused call may follow."""
import ctypes
import itertools

import pytest

from dm_nerf_amd import _lib

E_ARG = -1
BIG = (2048, 1024, 1024)               # 2^31 cells
D = [(k + 1) << 24 for k in range(9)]


def mask(v):
    return (ctypes.c_uint32 * 4)() if v["mask"] else None


# The arguments of every entry from one dict of values, in the order of the C signature (include/dmnerf_hip.h).
ARGS = {
    "label_components": lambda v: [v["d"][0], *v["dims"], v["C"], v["conn"], v["d"][1], v["d"][2], None],
    "label_components_largest": lambda v: [v["d"][0], *v["dims"], v["C"], v["d"][1], v["d"][2], v["d"][3], None],
    "label_components_filter": lambda v: [v["d"][0], v["cells"], *v["dims"], v["C"], mask(v), v["d"][1], v["d"][2], v["min"], v["mode"], v["d"][3],
                                          v["d"][4], v["out_cells"], v["d"][5], v["d"][6], None],
}
# Per entry: its checks from the one that answers first, the text of each (after "<entry>: "), and its number of device pointers.
DIMS = "bad dims {dims[0]} x {dims[1]} x {dims[2]}"
CELLS = "{n} cells do not fit int32"
C_RANGE = "C={C} outside 1..128"
TABLE = {
    "label_components": dict(order=("dims", "cells", "C", "conn", "null"), dev=3,
                             msg=dict(dims=DIMS, cells=CELLS, C=C_RANGE, conn="connectivity {conn} is neither 6 nor 26", null="null pointer")),
    "label_components_largest": dict(order=("dims", "cells", "C", "null"), dev=4, msg=dict(dims=DIMS, cells=CELLS, C=C_RANGE, null="null pointer")),
    "label_components_filter": dict(order=("dims", "cells", "C", "min", "mode", "host", "null", "pair", "align"), dev=7,
                                    msg=dict(dims=DIMS, cells=CELLS, C=C_RANGE, min="min_cells {min} must be >= 1", mode="mode {mode} (0 all, 1 largest)",
                                             host="null mask", null="null pointer", pair="d_cells and d_out_cells go together",
                                             align="cells must be 16-byte aligned")),
}


def faults_of(name):
    """fault -> (the check it trips, overrides of the good call's values)."""
    order, n = TABLE[name]["order"], TABLE[name]["dev"]
    out = {"dx0": ("dims", {"dims": (0, 4, 4)}), "dy0": ("dims", {"dims": (4, -1, 4)}), "dz0": ("dims", {"dims": (4, 4, 0)}),
           "cells": ("cells", {"dims": BIG}), "c0": ("C", {"C": 0}), "cbig": ("C", {"C": 129})}
    if "conn" in order:
        out.update(conn0=("conn", {"conn": 0}), conn18=("conn", {"conn": 18}), conn27=("conn", {"conn": 27}))
    if "min" in order:
        out.update(min0=("min", {"min": 0}), mode2=("mode", {"mode": 2}), modeneg=("mode", {"mode": -1}), nomask=("host", {"mask": False}),
                   cells_in_only=("pair", {"cells": D[7]}), cells_out_only=("pair", {"out_cells": D[8]}),
                   misaligned=("align", {"cells": D[7] + 4, "out_cells": D[8] + 16}))
    for k in range(n):
        out[f"null{k}"] = ("null", {"d": [None if j == k else p for j, p in enumerate(D)]})
    return out


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def check(lib, name, chosen):
    """Apply the faults in `chosen` together; the earliest of their checks in the entry's order must answer."""
    spec, faults = TABLE[name], faults_of(name)
    v = dict(dims=(4, 4, 4), C=13, conn=6, min=1, mode=0, mask=True, cells=None, out_cells=None, d=list(D))
    over = {}
    for f in chosen:
        for k, val in faults[f][1].items():
            if k == "d" and "d" in over:
                val = [None if (a is None or b is None) else a for a, b in zip(over["d"], val)]
            elif k in over and over[k] != val:
                return False                                         # two faults want the same argument: not a pair
            over[k] = val
    v.update(over)
    if "cells" in over and "out_cells" in over and over["cells"] == D[7]:
        return False                                                 # both sides given: no fault left
    first = min((faults[f][0] for f in chosen), key=spec["order"].index)
    rc = getattr(lib, "dmnerf_" + name)(*ARGS[name](v))
    v["n"] = v["dims"][0] * v["dims"][1] * v["dims"][2]
    want = f"{name}: " + spec["msg"][first].format(**v)
    assert (rc, _lib.last_error()) == (E_ARG, want), (name, chosen, rc, _lib.last_error(), want)
    return True


def test_the_table_covers_the_three_entries():
    assert set(ARGS) == set(TABLE) == {n[len("dmnerf_"):] for n in _lib.SIGNATURES if n.startswith("dmnerf_label_components")}
    v = dict(dims=(1, 1, 1), C=1, conn=6, min=1, mode=0, mask=True, cells=None, out_cells=None, d=list(D))
    for name in ARGS:
        assert len(ARGS[name](v)) == len(_lib.SIGNATURES["dmnerf_" + name][1]), name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_each_bad_argument_alone(lib, name):
    for f in faults_of(name):
        assert check(lib, name, (f,))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_which_check_answers_when_two_arguments_are_bad(lib, name):
    n = sum(check(lib, name, pair) for pair in itertools.combinations(faults_of(name), 2))
    assert n >= len(faults_of(name)), (name, n)
