"""numpy restatement of the grid from rendered views (``dmnerf_skip_grid_mark`` / ``dmnerf_skip_grid_dilate`` in csrc/skip.hip,
``field.SkipGrid.mark`` / ``.dilated``) on packed uint32 words.  The cell arithmetic is the select's of tests/_skip_restate.py (float32
operations in the stated order); the dilation works on the words themselves, bit by bit.  Array ops on float32 arrays (numpy rounds each
one to f32 on its own) and loops: nothing here shares code with the product."""
import numpy as np

from _grid_restate import cells_f32, grid_consts
from _skip_restate import pack_bits, unpack_bits

F = np.float32


def mark(words, rays_o, rays_d, z, weights, lo, hi, dims, threshold=0.0):
    """-> new uint32 words = ``words`` OR the bit of the cell of every sample ``(n, s)`` that is inside the box and whose weight is
    not ``<= threshold`` (so NaN marks).  The cell of a sample is ``_grid_restate.cells_f32`` (a NaN point is outside).  A sample
    outside the box marks nothing; a set bit is never cleared."""
    lo, _, inv = grid_consts(lo, hi, dims)
    o, d, z, w = (np.asarray(t, dtype=F) for t in (rays_o, rays_d, z, weights))
    out = np.array(words, dtype=np.uint32, copy=True)
    assert out.shape == ((dims[0] * dims[1] * dims[2] + 31) // 32,)
    assert w.shape == z.shape and o.shape == d.shape == (z.shape[0], 3)
    inside, g = cells_f32(o, d, z, lo, inv, dims)
    with np.errstate(invalid="ignore"):
        hit = ~(w <= F(threshold)) & inside                          # NaN: marks
    for cell in np.unique(g[hit]):
        out[cell >> 5] |= np.uint32(1) << np.uint32(cell & 31)
    return out


def dilate(words, dims, r):
    """-> uint32 words: bit ``g`` = OR of the bits of ``words`` over the ``(2 r + 1)^3`` neighbourhood of cell ``g``, clipped at the
    faces; the unused bits of the last word are 0.  Walks the SET bits of the input and sets their clipped neighbourhoods."""
    dx, dy, dz = dims
    words = np.asarray(words, dtype=np.uint32)
    out = np.zeros_like(words)
    for g in range(dx * dy * dz):
        if not (int(words[g >> 5]) >> (g & 31)) & 1:
            continue
        i, j, k = g // (dy * dz), (g // dz) % dy, g % dz
        for ii in range(max(i - r, 0), min(i + r, dx - 1) + 1):
            for jj in range(max(j - r, 0), min(j + r, dy - 1) + 1):
                for kk in range(max(k - r, 0), min(k + r, dz - 1) + 1):
                    h = (ii * dy + jj) * dz + kk
                    out[h >> 5] |= np.uint32(1) << np.uint32(h & 31)
    return out


__all__ = ["mark", "dilate", "grid_consts", "pack_bits", "unpack_bits"]
