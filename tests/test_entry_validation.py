"""Argument checks of the ray / sample MLP entries, entry by entry: return code, message text and which check answers when two
arguments are bad at once.  Every call here is refused (or is an empty batch) before the library touches a device, so the file
needs no GPU.  The expected texts are spelled out per entry: they are the library's contract with the callers that match them."""
import ctypes
import itertools

import pytest

from dm_nerf_amd import _lib

E_ARG, OK = -1, 0
MAX_LOGITS = 128                       # DMNERF_MAX_LOGITS
P = 64                                 # a non-null pointer that no refused call may follow

# Argument roles, in the order of the C signature:
#   p pointer (required)   o pointer (optional: never checked)   i ins_num   N rays / rows   S samples per ray
#   f fused_heads   v voxel   j n_jobs / n_outs   s stream
# `order` lists the entry's checks from the one that answers first; a text of None means the entry has no such check.
#   ins     ins_num outside 1 .. MAX_LOGITS - 1          range   N < 0, S < 1 (rows: M < 0; backward: M outside the launch limit)
#   sel     N * S does not fit the int32 selection       fused   fused_heads outside {0, 1}
#   empty   N == 0: DMNERF_OK, pointers not looked at    null    a required pointer is null
#   many    more workgroups than one launch holds        train   more samples than a training launch holds
#   badarg  the weight-gradient entries' single check of pointers and counts
RAYS = ("ins", "range", "empty", "null", "many", "train")
SEL = ("ins", "range", "sel", "fused", "empty", "null")
TABLE = {
    "mlp_fwd_rays": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays: ins_num {i} unsupported", range="mlp_fwd_rays: bad N={N} S={S}",
        null="mlp_fwd_rays: null pointer", many="mlp_fwd: {M} samples is too many for one launch"),
    "mlp_fwd_rays_fused": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays_fused: ins_num {i} unsupported", range="mlp_fwd_rays_fused: bad N={N} S={S}",
        null="mlp_fwd_rays_fused: null pointer", many="mlp_fwd: {M} samples is too many for one launch"),
    "mlp_fwd_rays_density": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays_density: ins_num {i} unsupported", range="mlp_fwd_rays_density: bad N={N} S={S}",
        null="mlp_fwd_rays_density: null pointer", many="mlp_fwd_rays_density: {M} samples is too many for one launch"),
    "mlp_fwd_rays_split": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays_split: ins_num {i} unsupported", range="mlp_fwd_rays_split: bad N={N} S={S}",
        null="mlp_fwd_rays_split: null pointer", many="mlp_fwd_rays_split: too many samples"),
    "mlp_fwd_rays_f16": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays_f16: ins_num {i} unsupported", range="mlp_fwd_rays_f16: bad N={N} S={S}",
        null="mlp_fwd_rays_f16: null pointer", many="mlp_fwd_rays_f16: too many samples"),
    "mlp_fwd_rays_density_f16": dict(
        sig="pipppNSps", order=RAYS, ins="mlp_fwd_rays_density_f16: ins_num {i} unsupported",
        range="mlp_fwd_rays_density_f16: bad N={N} S={S}", null="mlp_fwd_rays_density_f16: null pointer",
        many="mlp_fwd_rays_density_f16: too many samples"),
    "mlp_fwd_rays_train": dict(
        sig="pipppNSpps", order=RAYS, ins="mlp_fwd_rays_train: ins_num {i} unsupported", range="mlp_fwd_rays_train: bad N={N} S={S}",
        null="mlp_fwd_rays_train: null pointer", many="mlp_fwd: {M} samples is too many for one launch",
        train="mlp_fwd_train: {M} samples per launch exceed 1048576 (32-bit row offsets); split the batch"),
    "mlp_fwd_rays_train_fused": dict(
        sig="pipppNSpps", order=RAYS, ins="mlp_fwd_rays_train_fused: ins_num {i} unsupported",
        range="mlp_fwd_rays_train_fused: bad N={N} S={S}", null="mlp_fwd_rays_train_fused: null pointer",
        many="mlp_fwd: {M} samples is too many for one launch",
        train="mlp_fwd_train: {M} samples per launch exceed 1048576 (32-bit row offsets); split the batch"),
    "mlp_fwd_rays_train_split": dict(
        sig="pipppNSpps", order=RAYS, ins="mlp_fwd_rays_train_split: ins_num {i} unsupported",
        range="mlp_fwd_rays_train_split: bad N={N} S={S}", null="mlp_fwd_rays_train_split: null pointer",
        train="mlp_fwd_rays_train_split: {M} samples per launch exceed 1048576; split the batch"),
    "mlp_fwd_rays_train_f16": dict(
        sig="pipppNSpps", order=RAYS, ins="mlp_fwd_rays_train_f16: ins_num {i} unsupported",
        range="mlp_fwd_rays_train_f16: bad N={N} S={S}", null="mlp_fwd_rays_train_f16: null pointer",
        train="mlp_fwd_rays_train_f16: {M} samples per launch exceed 1048576; split the batch"),
    "mlp_fwd_rays_sel": dict(
        sig="pifpppNSppps", order=SEL, ins="mlp_fwd_rays_sel: ins_num {i} unsupported", range="mlp_fwd_rays_sel: bad N={N} S={S}",
        sel="mlp_fwd_rays_sel: {M} samples do not fit the int32 selection", fused="mlp_fwd_rays_sel: fused_heads {f} unsupported",
        null="mlp_fwd_rays_sel: null pointer"),
    "mlp_fwd_rays_density_sel": dict(
        sig="pipppNSppps", order=SEL, ins="mlp_fwd_rays_density_sel: ins_num {i} unsupported",
        range="mlp_fwd_rays_density_sel: bad N={N} S={S}", sel="mlp_fwd_rays_density_sel: {M} samples do not fit the int32 selection",
        null="mlp_fwd_rays_density_sel: null pointer"),
    "mlp_fwd_rays_f16_sel": dict(
        sig="pipppNSppps", order=SEL, ins="mlp_fwd_rays_f16_sel: ins_num {i} unsupported", range="mlp_fwd_rays_f16_sel: bad N={N} S={S}",
        sel="mlp_fwd_rays_f16_sel: {M} samples do not fit the int32 selection", null="mlp_fwd_rays_f16_sel: null pointer"),
    "mlp_fwd_rays_density_f16_sel": dict(
        sig="pipppNSppps", order=SEL, ins="mlp_fwd_rays_density_f16_sel: ins_num {i} unsupported",
        range="mlp_fwd_rays_density_f16_sel: bad N={N} S={S}",
        sel="mlp_fwd_rays_density_f16_sel: {M} samples do not fit the int32 selection", null="mlp_fwd_rays_density_f16_sel: null pointer"),
    "mlp_fwd_embedded": dict(
        sig="pipNps", order=RAYS, ins="mlp_fwd_embedded: ins_num {i} unsupported", range="mlp_fwd_embedded: M < 0",
        null="mlp_fwd_embedded: null pointer", many="mlp_fwd: {M} samples is too many for one launch"),
    "mlp_fwd_embedded_train": dict(
        sig="pipNpps", order=RAYS, ins="mlp_fwd_embedded_train: ins_num {i} unsupported", range="mlp_fwd_embedded_train: M < 0",
        null="mlp_fwd_embedded_train: null pointer", many="mlp_fwd: {M} samples is too many for one launch",
        train="mlp_fwd_train: {M} samples per launch exceed 1048576 (32-bit row offsets); split the batch"),
    "mlp_fwd_points_density": dict(
        sig="pipNpvs", order=RAYS, ins="mlp_fwd_points_density: ins_num {i} unsupported",
        range="mlp_fwd_points_density: bad M={N} voxel=0.5", null="mlp_fwd_points_density: null pointer",
        many="mlp_fwd_points_density: {M} samples is too many for one launch"),
    # (M above the training-launch limit is the same check as M < 0 here: the `train` fault answers with the range text)
    "mlp_bwd_data": dict(
        sig="ppippNpos", order=("ins", "range", "empty", "null"), ins="mlp_bwd_data: ins_num {i} unsupported",
        range="mlp_bwd_data: M={N} outside [0,1048576]", null="mlp_bwd_data: null pointer", train_is_range=True),
    "mlp_bwd_data_split": dict(
        sig="pippNpos", order=("ins", "range", "empty", "null"), ins="mlp_bwd_data_split: ins_num {i} unsupported",
        range="mlp_bwd_data_split: M={N} outside [0,1048576]", null="mlp_bwd_data_split: null pointer", train_is_range=True),
    "mlp_bwd_data_f16": dict(
        sig="pippNpoos", order=("ins", "range", "empty", "null"), ins="mlp_bwd_data_f16: ins_num {i} unsupported",
        range="mlp_bwd_data_f16: M={N} outside [0,1048576]", null="mlp_bwd_data_f16: null pointer", train_is_range=True),
    # one check of every pointer and count comes first and an empty batch is not legal: M = 0 is a bad argument
    "mlp_bwd_weights": dict(
        sig="pppNpjpjpipps", order=("badarg", "ins"), ins="mlp_bwd_weights: ins_num {i} unsupported",
        badarg="mlp_bwd_weights: bad argument"),
    "mlp_bwd_weights_split": dict(
        sig="pppNpjpjpipps", order=("badarg", "ins"), ins="mlp_bwd_weights_split: ins_num {i} unsupported",
        badarg="mlp_bwd_weights_split: bad argument"),
    "mlp_bwd_weights_f16": dict(
        sig="pppNpjpjpippos", order=("badarg", "ins"), ins="mlp_bwd_weights_f16: ins_num {i} unsupported",
        badarg="mlp_bwd_weights_f16: bad argument"),
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def faults_of(spec):
    """name -> (the check it trips, overrides of the good call's arguments); only faults whose check the entry has."""
    sig, wgrad = spec["sig"], "badarg" in spec["order"]
    out = {"ins0": ("ins", {"i": 0}), "insmax": ("ins", {"i": MAX_LOGITS}), "nneg": ("badarg" if wgrad else "range", {"N": -1})}
    if "S" in sig:
        out["szero"] = ("range", {"S": 0})
    if spec.get("sel"):
        out["sel"] = ("sel", {"N": 1 << 20, "S": 1 << 11})
    if spec.get("fused"):
        out["fused"] = ("fused", {"f": 2})
    if spec.get("many"):
        out["many"] = ("many", {"N": 1 << 40})
    if spec.get("train"):
        out["train"] = ("train", {"N": (1 << 20) + 1})
    if spec.get("train_is_range"):
        out["train"] = ("range", {"N": (1 << 20) + 1})
    out["empty"] = ("badarg" if wgrad else "empty", {"N": 0, "p": [None] * sig.count("p")})
    for k in range(sig.count("p")):
        out[f"null{k}"] = ("badarg" if wgrad else "null", {"p": [None if j == k else P for j in range(sig.count("p"))]})
    if wgrad:
        out["jobs0"] = ("badarg", {"j": 0})
    return out


def call(lib, name, spec, over):
    """The entry with good arguments (N = 1 row, every pointer P) except for `over`; -> (return code, message)."""
    vals = {"i": 13, "N": 1, "S": 1, "f": 0, "v": 0.5, "j": 1}
    vals.update({k: v for k, v in over.items() if k != "p"})
    ptrs = iter(over.get("p", [P] * spec["sig"].count("p")))
    args = [next(ptrs) if r == "p" else P if r == "o" else None if r == "s" else vals[r] for r in spec["sig"]]
    rc = getattr(lib, "dmnerf_" + name)(*args)
    return rc, _lib.last_error(), vals


def check(lib, name, spec, chosen):
    """Apply the faults in `chosen` together; the earliest of their checks in the entry's order must answer."""
    faults = faults_of(spec)
    over = {}
    for f in chosen:
        for k, v in faults[f][1].items():
            if k == "p" and "p" in over:
                v = [None if (a is None or b is None) else P for a, b in zip(over["p"], v)]
            elif k in over and over[k] != v:
                return False                                         # two faults want the same argument: not a pair
            over[k] = v
    keys = [faults[f][0] for f in chosen]
    assert keys, "a call with good arguments would launch"
    first = min(keys, key=spec["order"].index)
    rc, msg, vals = call(lib, name, spec, over)
    if first == "empty":
        assert rc == OK, (name, chosen, rc, msg)
    else:
        want = spec[first].format(i=vals["i"], N=vals["N"], S=vals["S"], M=vals["N"] * vals["S"], f=vals["f"])
        assert (rc, msg) == (E_ARG, want), (name, chosen, rc, msg, want)
    return True


def test_table_covers_every_ray_and_sample_entry():
    fams = ("dmnerf_mlp_fwd_", "dmnerf_mlp_bwd_data", "dmnerf_mlp_bwd_weights")
    assert {n for n in _lib.SIGNATURES if n.startswith(fams)} == {"dmnerf_" + n for n in TABLE}
    for name, spec in TABLE.items():
        assert len(spec["sig"]) == len(_lib.SIGNATURES["dmnerf_" + name][1]), name
        for r, t in zip(spec["sig"], _lib.SIGNATURES["dmnerf_" + name][1]):
            assert t is {"p": _lib.c_vp, "o": _lib.c_vp, "s": _lib.c_vp, "N": _lib.c_i64, "v": _lib.c_float}.get(r, _lib.c_int), (name, r)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_each_bad_argument_alone(lib, name):
    spec = TABLE[name]
    for f in faults_of(spec):
        assert check(lib, name, spec, (f,))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_which_check_answers_when_two_arguments_are_bad(lib, name):
    spec = TABLE[name]
    n = sum(check(lib, name, spec, pair) for pair in itertools.combinations(faults_of(spec), 2))
    assert n >= 10, (name, n)


def test_messages_name_the_entry(lib):
    for name, spec in TABLE.items():
        for n in (0, MAX_LOGITS):
            assert call(lib, name, spec, {"i": n})[:2] == (E_ARG, f"{name}: ins_num {n} unsupported")
