"""Host tests of ``tests/golden/occupancy.npz`` (made by tests/golden/make_golden_occupancy.py from the reference's own grid and
network code): the fixture loads, the float32 restatement of the grid kernel's prologue reproduces the reference's query points
bit for bit, and the stored occupancies are probabilities."""
import os

import numpy as np
import pytest

import _occupancy_restate as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occupancy.npz")


@pytest.fixture(scope="module")
def G():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_loads_and_is_small(G):
    assert os.path.getsize(GOLDEN) < 100 * 1024
    for dim in (5, 8):
        assert G[f"points_{dim}"].shape == (dim ** 3, 3) and G[f"points_{dim}"].dtype == np.float32
        assert G[f"sigma_14_{dim}"].shape == (dim ** 3,) and G[f"occ_14_{dim}"].shape == (dim ** 3,)
    assert G["sigma_94_5"].shape == (125,) and G["occ_94_5"].shape == (125,)
    assert G["transform"].shape == (4, 4) and G["extents"].tolist() == [1.9, 7.0, 7.0]
    assert float(G["voxel"]) == (float(G["far"]) - float(G["near"])) / int(G["n_importance"])
    R = G["transform"][:3, :3]
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12      # rotated ...
    assert np.abs(R - np.eye(3)).max() > 0.1 and np.abs(G["transform"][:3, 3]).min() > 0           # ... and translated


@pytest.mark.parametrize("dim", [5, 8])
def test_restated_prologue_equals_the_reference_points(G, dim):
    got = RS.grid_points(G["occ_range"], G["extents"], G["transform"], dim)
    assert got.dtype == np.float32 and np.array_equal(got, G[f"points_{dim}"])


def test_stored_occupancy_is_a_probability(G):
    for key in ("14_5", "14_8", "94_5"):
        occ, sigma = G["occ_" + key], G["sigma_" + key]
        assert occ.dtype == np.float32 and (occ >= 0).all() and (occ <= 1).all()
        assert (occ[sigma <= 0] == 0).all() and (occ[sigma > 0] > 0).all()
    assert (G["sigma_14_5"] < 0).any() and (G["sigma_14_5"] > 0).any()
