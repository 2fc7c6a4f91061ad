"""CPU checks of the semantics the manipulation render's ``skip=`` route rests on (tests/_manip_skip_restate.py): the empty row E is
exactly neutral to the compositing, its label is the last channel, ``fill_rows`` touches nothing else -- and the power case of
tests/test_gpu_manip_skip.py really tells E rows from all-zero rows, shown here on the CPU oracle."""
import numpy as np
import pytest
import torch

import _manip_skip_restate as MR
from oracle import ref_cpu as O

RENDER = getattr(O, "manipulator_render", MR.manipulator_render_cpu)


def random_raw(n, s, C, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(n, s, 4 + C, generator=g) * 2.0                # sigma of both signs
    z = (4.0 + 11.0 * torch.rand(n, s, generator=g)).sort(-1).values
    d = torch.randn(n, 3, generator=g)
    flag = (torch.rand(n, s, generator=g) < 0.4).to(torch.uint8)
    flag[0] = 0                                                       # a ray without one evaluated sample
    flag[1] = 1                                                       # ... and one without a skipped sample
    return raw, z, d, flag


@pytest.mark.parametrize("C", [2, 14, 94])
def test_the_empty_row_is_neutral_to_the_compositing(C):
    """Rows replaced by E and rows replaced by zeros composite to the same rgb, weights, depth and object map, bitwise: sigma = 0
    gives alpha = 1 - exp(-0) = 0 exactly, the weight 0 * T = 0, and the row's terms are 0 * x."""
    raw, z, d, flag = random_raw(9, 13, C, seed=C)
    with_e = RENDER(MR.fill_rows(raw, flag, C), z, d)
    with_0 = RENDER(MR.fill_rows(raw, flag, C, zero_rows=True), z, d)
    for a, b in zip(with_e, with_0):
        assert torch.equal(a, b)
    assert not bool(with_e[1][flag == 0].any())                       # a skipped sample weighs exactly nothing
    assert float(with_e[1][1].sum()) > 0 and not torch.equal(with_e[0], RENDER(raw, z, d)[0])


@pytest.mark.parametrize("C", [2, 14, 94])
def test_the_empty_row_is_labelled_empty(C):
    row = MR.empty_row(C)
    assert row.shape == (4 + C,) and not bool(row[:4].any()) and not bool(row[4:-1].any()) and float(row[-1]) == 1.0
    assert int(torch.argmax(row[4:])) == C - 1
    assert int(torch.argmax(torch.sigmoid(row[4:]))) == C - 1        # the exchanger's per-sample label
    assert int(torch.argmax(torch.zeros(C))) == 0                     # ... where an all-zero row reads as object 0


@pytest.mark.parametrize("C", [2, 14])
def test_fill_rows_leaves_flagged_rows_bit_identical(C):
    raw, _, _, flag = random_raw(9, 13, C, seed=100 + C)
    raw[2, 3, 1] = float("nan")
    flag[2, 3] = 1
    for zero_rows in (False, True):
        out = MR.fill_rows(raw, flag, C, zero_rows)
        keep = flag != 0
        assert np.array_equal(out[keep].numpy().view(np.int32), raw[keep].numpy().view(np.int32))
        want = torch.zeros(4 + C) if zero_rows else MR.empty_row(C)
        assert bool((out[~keep] == want).all())
    assert MR.fill_rows(raw, flag.numpy(), C).data_ptr() != raw.data_ptr()
    assert np.array_equal(MR.fill_rows(raw, flag.numpy(), C).numpy().view(np.int32), MR.fill_rows(raw, flag, C).numpy().view(np.int32))


def test_the_power_case_tells_empty_rows_from_zero_rows_on_the_oracle():
    """The case of ``test_a_skipped_sample_is_never_the_moved_object``, run through the CPU oracle's ``manipulator`` with the fill after
    every network call: moving label 0 with E rows and with all-zero rows must give different frames.  ``POWER['bias0']`` was chosen
    by this computation: of 130 rays, 2 differ at bias 0, 20 at 0.12, 96 at 0.2 (chosen) and none from 0.5 on, where EVERY sample is
    labelled 0 and overwriting a vacated sample by a zero row changes nothing."""
    P = MR.POWER
    ori, tars = MR.case_rays(O, 130, 1)
    spec = MR.random_spec(P["dims"], P["frac"], P["grid_seed"], P["outside"])
    us = MR.case_draws(130, 8, 3)
    sds = MR.power_weights(O)
    e = MR.oracle_chain(O, sds, ori, tars, spec, [P["label"]], us, 8, 8, zero_rows=False)
    z = MR.oracle_chain(O, sds, ori, tars, spec, [P["label"]], us, 8, 8, zero_rows=True)
    differ = (e[0] - z[0]).abs().max(-1).values > 1e-3
    assert int(differ.sum()) >= 30, int(differ.sum())                 # far beyond float noise, on many rays
    assert all(bool(torch.isfinite(t).all()) for t in e)
