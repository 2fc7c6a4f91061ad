"""Host tests (no GPU) of the edit operator's restatement (tests/_edit_kinds_restate.py) against ``oracle.ref_cpu.exchanger``,
of the fixture the GPU test shares with it, and of the argument checks of ``dmnerf_edit_exchange``."""
import ctypes

import pytest
import torch

import _edit_kinds_restate as RS
from oracle import ref_cpu as O

N, S, C = 37, 13, 14


def test_all_moves_are_the_reference_exchanger():
    for labels in ([0], [0, 5, 3], [3, 0, 5, 7, 1, 9, 2, 12]):
        c = RS.make_case(N, S, C, labels, [RS.MOVE] * len(labels), seed=41 + len(labels))
        want = O.exchanger(c["ori"].clone(), [t.clone() for t in c["tars"]], c["ori_acc"], c["tar_accs"], labels)
        counts = {}
        got = RS.edit_restate(c["ori"].clone(), c["tars"], c["ori_acc"], c["tar_accs"], labels, [RS.MOVE] * len(labels), counts=counts)
        assert torch.equal(RS.bits(got[0]), RS.bits(want[0])) and torch.equal(got[1], want[2])
        assert all(counts[k] >= 1 for k in ("occlusion", "fill", "exchange1", "exchange3", "eliminate")), counts
        assert not torch.equal(RS.bits(got[0]), RS.bits(c["ori"]))


def test_removal_is_the_reference_exchanger_with_an_empty_target():
    """The reference's own way to a removal: the target IS the untouched original and its accumulated label is never the entry's.
    The fill then copies identical rows and the target mask is empty: what remains is the eliminate branch."""
    Ls = [0, 5, 3]
    c = RS.make_case(N, S, C, Ls, [RS.REMOVE] * 3, seed=7)
    ori0 = c["ori"]
    accs = []
    for L in Ls:
        acc = torch.zeros(N, C)
        acc[:, (L + 1) % (C - 1)] = 5.0
        assert not bool((torch.argmax(torch.sigmoid(acc[..., :-1]), -1) == L).any())
        accs.append(acc)
    want = O.exchanger(ori0.clone(), [ori0.clone()] * len(Ls), c["ori_acc"], accs, Ls)
    counts = {}
    got = RS.edit_restate(ori0.clone(), [None] * 3, c["ori_acc"], [None] * 3, Ls, [RS.REMOVE] * 3, counts=counts)
    assert torch.equal(RS.bits(got[0]), RS.bits(want[0])) and torch.equal(got[1], want[2])
    assert counts["remove"] >= 1 and counts["occlusion"] >= 1
    removed = (got[0] == 0).all(-1)
    assert int(removed.sum()) == counts["remove"] and bool((RS.bits(got[0])[~removed] == RS.bits(ori0)[~removed]).all())
    assert bool((RS.bits(got[0]) == -2 ** 31).any())                     # x * 0 keeps the sign: -0.0 where x < 0


def test_fixture_reaches_every_branch_and_holds_both_kinds_of_tie():
    labels, kinds = [0, 5, 3, 7], [RS.MOVE, RS.COPY, RS.REMOVE, RS.MOVE]
    c = RS.make_case(N, S, C, labels, kinds, seed=19)
    counts = {}
    out, _ = RS.edit_restate(c["ori"].clone(), c["tars"], c["ori_acc"], c["tar_accs"], labels, kinds, keep_labels=[0, 1, 5, 8, 13], counts=counts)
    assert sorted(counts) == sorted(RS.BRANCHES) and all(counts[k] >= 1 for k in RS.BRANCHES), counts
    # the inputs hold an exact logit tie and a tie that only the saturated sigmoid makes; both resolve to the FIRST maximum
    logits = c["ori"][..., 4:]
    top2 = logits.topk(2, -1).values
    assert bool((top2[..., 0] == top2[..., 1]).any())
    sat = (logits > 20).sum(-1) >= 2
    assert bool(sat.any())
    sig = torch.sigmoid(logits[sat])
    assert bool(((sig == 1.0).sum(-1) >= 2).all()) and bool((sig.argmax(-1) != logits[sat].argmax(-1)).all())
    assert int(torch.sigmoid(logits[0, 0]).argmax()) == 0 and int(torch.sigmoid(logits[0, 1]).argmax()) == 0
    # ... and the decision shows in the result: ray 0 is a ray of label 0, so removing 0 zeroes both rows, removing C - 1 neither
    first = RS.edit_restate(c["ori"].clone(), [None], c["ori_acc"], [None], [0], [RS.REMOVE])[0]
    last = RS.edit_restate(c["ori"].clone(), [None], c["ori_acc"], [None], [C - 1], [RS.REMOVE])[0]
    assert bool((first[0, :2] == 0).all()) and torch.equal(RS.bits(last[0, :2]), RS.bits(c["ori"][0, :2]))


def test_keep_mask_ignores_the_order_of_the_edits():
    labels, kinds = [0, 5, 3], [RS.REMOVE, RS.COPY, RS.REMOVE]
    c = RS.make_case(N, S, C, labels, kinds, seed=23)
    l0 = torch.argmax(torch.sigmoid(c["ori"][..., 4:]), -1)
    keep = [0, 5, 7]
    out, _ = RS.edit_restate(c["ori"].clone(), c["tars"], c["ori_acc"], c["tar_accs"], labels, kinds, keep_labels=keep)
    dropped = ~torch.isin(l0, torch.tensor(keep))
    assert bool((out[dropped] == 0).all()) and bool(dropped.any()) and bool((out[~dropped] != 0).any())
    only = RS.edit_restate(c["ori"].clone(), [], c["ori_acc"], [], [], [], keep_labels=keep)[0]
    assert torch.equal((only == 0).all(-1), dropped)


def _call(E, kinds, labels, raws, accs, keep=None, C_=14, S_=4, N_=3):
    from dm_nerf_amd import _lib
    lib = _lib.load()
    n = max(E, 1)
    P = ctypes.c_void_p * n
    k = (ctypes.c_int * n)(*kinds)
    lab = (ctypes.c_int * n)(*labels)
    kp = None if keep is None else (ctypes.c_uint64 * 2)(*keep)
    rc = lib.dmnerf_edit_exchange(ctypes.c_void_p(64), P(*raws), ctypes.c_void_p(64), P(*accs), lab, k, E, kp, N_, S_, C_, None, None)
    return rc, _lib.last_error()


def test_argument_errors_are_reported_before_anything_touches_a_device():
    """Every call below hands over addresses that are never dereferenced: the checks come first, on a host without a GPU too."""
    X = 64                                                                   # a non-null stand-in for a device pointer
    rc, msg = _call(9, [0] * 9, [1] * 9, [X] * 9, [X] * 9)
    assert rc == -1 and "E=9" in msg
    rc, msg = _call(0, [0], [0], [None], [None])                             # no edit and no keep mask
    assert rc == -1 and "E=0" in msg
    rc, msg = _call(1, [3], [1], [X], [X])
    assert rc == -1 and "kind" in msg
    rc, msg = _call(2, [2, 0], [1, 2], [None, None], [None, X])              # a MOVE without its target rows
    assert rc == -1 and "null target" in msg
    rc, msg = _call(1, [1], [1], [X], [None])                                # a COPY without its accumulated map
    assert rc == -1 and "null target" in msg
    rc, msg = _call(1, [2], [1], [X], [None])                                # a REMOVE must not be given a target
    assert rc == -1 and "removal" in msg
    rc, msg = _call(1, [2], [14], [None], [None])
    assert rc == -1 and "label" in msg
    rc, msg = _call(1, [2], [-1], [None], [None])
    assert rc == -1 and "label" in msg
    rc, msg = _call(1, [2], [1], [None], [None], C_=129)
    assert rc == -1 and "C=129" in msg
    rc, msg = _call(1, [2], [0], [None], [None], C_=1)
    assert rc == -1
    rc, msg = _call(1, [2], [1], [None], [None], S_=0)
    assert rc == -1
    assert _call(1, [2], [1], [None], [None], N_=0)[0] == 0                  # no rays: a no-op after the checks
    assert _call(0, [0], [0], [None], [None], keep=[5, 0], N_=0)[0] == 0


def test_python_surface_checks():
    from dm_nerf_amd import editing as E
    from dm_nerf_amd.networks import manipulator as MA
    assert (MA.MOVE, MA.COPY, MA.REMOVE) == (RS.MOVE, RS.COPY, RS.REMOVE) == (0, 1, 2)
    assert MA.keep_words([0, 63, 64, 127], 128) == [1 | 1 << 63, 1 | 1 << 63]
    with pytest.raises(ValueError):
        MA.keep_words([14], 14)
    m = torch.eye(4)
    assert [E.edit_kind(t) for t in (m, E.Deform("ex", 0), E.Copy(m), E.Remove(), E.Copy(E.Deform("ln", 1)))] == [0, 0, 1, 2, 1]
    assert E.Remove() == E.Remove() and repr(E.Remove()) == "Remove()"
    for bad in (E.Remove(), E.Copy(m), torch.eye(3)):
        with pytest.raises(ValueError):
            E.Copy(bad)
