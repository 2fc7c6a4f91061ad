"""CPU: the restatement of the training step that skips empty space (tests/_train_skip_restate.py) against hand-written
expectations -- gather, scatter, padding, the masked referee -- and the hand-written scenes' own conditions."""
import numpy as np
import pytest
import torch

import _train_skip_restate as T


def test_padded_length():
    assert [T.padded_length(n, 64) for n in (0, 1, 63, 64, 65, 128, 129)] == [0, 64, 64, 64, 128, 128, 192]
    assert T.padded_length(5, 1) == 5


def test_gather_samples_by_hand():
    o = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.float32)
    d = -o
    z = np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]], dtype=np.float32)
    oc, dc, zc = T.gather_samples(o, d, z, [1, 4, 5], 5)              # samples (ray 0, s 1), (ray 2, s 0), (ray 2, s 1)
    assert oc.tolist() == [[1, 2, 3], [7, 8, 9], [7, 8, 9], [7, 8, 9], [7, 8, 9]]
    assert np.array_equal(dc, -oc)
    assert zc.tolist() == [np.float32(0.2), np.float32(0.5), np.float32(0.6), np.float32(0.6), np.float32(0.6)]
    oc, dc, zc = T.gather_samples(o, d, z, [], 0)
    assert oc.shape == (0, 3) and zc.shape == (0,)
    with pytest.raises(AssertionError):
        T.gather_samples(o, d, z, [], 4)                              # nothing to repeat


def test_scatter_and_gather_by_hand():
    dst = np.full((5, 2), -7.0, dtype=np.float32)
    src = np.array([[1, 2], [3, 4], [9, 9], [9, 9]], dtype=np.float32)          # two rows and two padded rows
    out = T.rows_scatter(dst, src, [0, 3])
    assert out.tolist() == [[1, 2], [-7, -7], [-7, -7], [3, 4], [-7, -7]]
    assert (dst == -7.0).all()                                                  # a copy
    g = np.arange(10, dtype=np.float32).reshape(5, 2)
    assert T.rows_gather(g, [0, 3], 4).tolist() == [[0, 1], [6, 7], [0, 0], [0, 0]]
    assert T.rows_gather(g, [], 0).shape == (0, 2)
    # gather is the transpose of scatter: <scatter(0, x), g> == <x, gather(g)>
    rs = np.random.RandomState(0)
    x, g = rs.randn(8, 3), rs.randn(11, 3)
    sel = [1, 2, 5, 7, 10]
    assert np.isclose((T.rows_scatter(np.zeros((11, 3)), x, sel) * g).sum(), (x * T.rows_gather(g, sel, 8)).sum())


@pytest.mark.parametrize("S", [5, 7])
@pytest.mark.parametrize("outside", ["empty", "evaluate"])
def test_hand_scene_is_not_degenerate(S, outside):
    s = T.hand_scene(S, outside)                                      # (asserts its own conditions)
    assert s["flag"].shape == (T.N_RAYS, S) and s["count"] == int(s["flag"].sum())
    assert np.array_equal(s["sel"], np.nonzero(s["flag"].reshape(-1))[0])
    assert 0.2 <= s["count"] / s["flag"].size <= 0.8 and s["count"] % 32


def test_exact_scenes_hit_the_bucket_edges():
    assert T.exact_scene(64)["count"] == 64 and T.exact_scene(65)["count"] == 65
    assert T.padded_length(64, 64) == 64 and T.padded_length(65, 64) == 128


def test_masked_referee_ignores_unflagged_samples():
    from oracle import ref_cpu as O
    sd = O.make_weights(3, 13, gain=1.7)
    g = torch.Generator().manual_seed(3)
    o, d = torch.randn(3, 3, generator=g), torch.randn(3, 3, generator=g)
    z = torch.rand(3, 4, generator=g) * 3 + 1
    cot = torch.randn(3, 4, 18, generator=g)
    flag = np.array([[1, 0, 0, 1], [0, 0, 0, 0], [1, 1, 0, 0]], dtype=np.uint8)
    raw, want = T.masked_oracle_grads(sd, o, d, z, cot, flag)
    assert raw.dtype == torch.float64 and raw.shape == (3, 4, 18)
    # the same gradients from the flagged samples alone, each as its own one-sample ray
    idx = np.nonzero(flag.reshape(-1))[0]
    oc, dc, zc = T.gather_samples(o.numpy(), d.numpy(), z.numpy(), idx, len(idx))
    cot_c = cot.reshape(-1, 18)[torch.from_numpy(idx)][:, None, :]
    _, alone = T.masked_oracle_grads(sd, torch.from_numpy(oc), torch.from_numpy(dc), torch.from_numpy(zc)[:, None], cot_c,
                                     np.ones((len(idx), 1), dtype=np.uint8))
    for k in want:
        assert torch.allclose(want[k], alone[k], rtol=1e-10, atol=1e-12), k
    # a cotangent on an unflagged sample changes nothing
    cot2 = cot.clone()
    cot2[1] += 5.0
    _, again = T.masked_oracle_grads(sd, o, d, z, cot2, flag)
    assert all(torch.equal(want[k], again[k]) for k in want)
