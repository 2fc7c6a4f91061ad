"""The generic path's gate for the chained trunk (dm_nerf_amd/generic.py ``_chain_ok``) agrees with the entry point it guards
(csrc/gemm_chain.hip ``dmnerf_mlp_chain``): inference must take the chain exactly where the library accepts it, or a supported shape
raises instead of falling back to the layer-by-layer trunk.  Host-only: the entry point validates its sizes before the M = 0 return,
so it runs without a GPU."""
import pytest


@pytest.mark.parametrize("W", [32, 64, 96, 128, 160, 192])
def test_chain_gate_matches_the_entry_point(W):
    from dm_nerf_amd import _lib, generic as G
    lib = _lib.load()
    for inp in (3, 27, 39, 63, 99):
        for D in range(1, 18):
            rc = lib.dmnerf_mlp_chain(None, 0, 0, inp, None, D, W, None, 0, 0, None)
            assert G._chain_ok(W, inp, D) == (rc == 0), (W, inp, D, rc, _lib.last_error())
    # the corners of the table: the bias table is full at 16 layers x 4 out-blocks, over at 13 x 5; 17 layers never chain
    assert G._chain_ok(128, 63, 16) and not G._chain_ok(160, 63, 13) and G._chain_ok(160, 63, 12) and not G._chain_ok(64, 39, 17)
