"""What the numpy restatements of the grid volumes share (csrc/grid_volume.h states the same rules for the kernels): the box constants
as the host computes them, the 128-bit label mask, and the cell of a sample.  Array ops on float32 arrays -- numpy rounds every one to
f32 on its own -- and nothing here shares code with the product."""
import numpy as np

f32 = np.float32


def grid_consts(lo, hi, dims):
    """``lo``, ``cell = float32(hi - lo) / float32(dims)``, ``inv_cell = float32(1) / cell`` (float32 ``[3]``, one rounding each), as
    ``field.SkipGrid`` / ``field.LabelGrid`` compute them on the host."""
    lo, hi = np.asarray(lo, dtype=f32).reshape(3), np.asarray(hi, dtype=f32).reshape(3)
    cell = ((hi - lo) / np.asarray(dims, dtype=f32)).astype(f32)
    return lo, cell, (f32(1.0) / cell).astype(f32)


def mask_words(labels, C):
    """``field.label_mask_words``: label l is bit l & 31 of word l >> 5 of four 32-bit words."""
    w = [0, 0, 0, 0]
    for l in labels:
        assert 0 <= int(l) < C
        w[int(l) >> 5] |= 1 << (int(l) & 31)
    return w


def _in_mask(l, words):
    """labels (int64 array or int) -> bool: bit l of the 128-bit mask, False for l >= 128."""
    l = np.asarray(l, dtype=np.int64)
    words = np.asarray(list(words)[:4] + [0], dtype=np.uint64)
    return ((words[np.minimum(l >> 5, 4)] >> (l & 31).astype(np.uint64)) & np.uint64(1)) != 0


def cells_f32(rays_o, rays_d, z, lo, inv_cell, dims):
    """The cell of every sample -> ``(inside [N,S] bool, flat cell [N,S] int64 (0 where outside))``.  ``p = o + d * z`` (multiply, then
    add, each rounded to f32), ``c = floor((p - lo) * inv_cell)`` (subtract, multiply, each rounded), inside iff ``0 <= c < dims`` on
    the float for all axes (a NaN point is outside), cell ``(c_x * dy + c_y) * dz + c_z``."""
    o, d, z = np.asarray(rays_o, f32), np.asarray(rays_d, f32), np.asarray(z, f32)
    inside = np.ones(z.shape, dtype=bool)
    g = np.zeros(z.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            p = (o[:, a:a + 1] + (d[:, a:a + 1] * z).astype(f32)).astype(f32)
            c = np.floor(((p - f32(lo[a])).astype(f32) * f32(inv_cell[a])).astype(f32))
            inside &= (c >= 0) & (c < f32(dims[a]))
            g = g * dims[a] + np.where(inside, c, 0).astype(np.int64)
    return inside, np.where(inside, g, 0)
