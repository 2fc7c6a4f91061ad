"""numpy float32 restatement of the grid prologue of csrc/mlp_fwd_points.hip (``dmnerf_occupancy_slab``): the query points of the
reference's ``mesh_main`` -- ``grid_within_bound`` (tools/visualizer.py:111-155) and the axis swap of mesh_generator.py:28-29 --
one sample at a time, every product and every sum rounded to float32 on its own.  ``tests/golden/make_golden_occupancy.py``
proves it against the reference's own tensors; ``tests/test_occupancy_golden.py`` re-checks it against the stored ones."""
import numpy as np
import torch


def grid_constants(occ_range, extents, transform, dim):
    """``t [dim]`` (torch.linspace on the host, as the reference evaluates it), ``scale [3]`` f32, ``T [3, 4]`` f32."""
    lo, hi = float(occ_range[0]), float(occ_range[1])
    t = torch.linspace(lo, hi, steps=dim).numpy()
    scale = (np.asarray(extents, dtype=np.float64) / ((hi - lo) * 1.0)).astype(np.float32)
    T = np.asarray(transform).astype(np.float32)[:3, :4]
    return t, scale, T


def grid_points(occ_range, extents, transform, dim):
    """``[dim^3, 3]`` float32; sample ``g``: ``i = g / dim^2, j = (g / dim) % dim, k = g % dim``."""
    t, s, T = grid_constants(occ_range, extents, transform, dim)
    f = np.float32
    g = np.arange(dim ** 3)
    i, j, k = g // (dim * dim), (g // dim) % dim, g % dim
    x, y, z = (t[i] * s[0]).astype(f), (t[j] * s[1]).astype(f), (t[k] * s[2]).astype(f)
    q = []
    for r in range(3):
        a = ((T[r, 0] * x).astype(f) + (T[r, 1] * y).astype(f)).astype(f)
        a = (a + (T[r, 2] * z).astype(f)).astype(f)
        q.append((a + T[r, 3]).astype(f))
    return np.stack([q[0], -q[2], q[1]], axis=-1)
