"""numpy restatement of the occupancy bit grid of ``dm_nerf_amd.field.SkipGrid`` / csrc/skip.hip: the grid build (threshold,
clipped dilation, bit packing), the select (float32 operations in the stated order, the ``outside`` policy, ascending ``sel``) and
the masking of rows.  Loops and array ops only: nothing here shares code with the product."""
import numpy as np

from _grid_restate import cells_f32, grid_consts

F = np.float32


def occupied(sigma, threshold):
    """A cell is occupied iff sigma > threshold; NaN counts as occupied."""
    sigma = np.asarray(sigma, dtype=F)
    return ~(sigma <= F(threshold))


def dilate_clipped(occ, dilate):
    """``out[i,j,k]`` = any of ``occ`` in the ``(2 dilate + 1)^3`` neighbourhood, clipped at the faces."""
    dx, dy, dz = occ.shape
    out = np.zeros_like(occ, dtype=bool)
    for i in range(dx):
        for j in range(dy):
            for k in range(dz):
                out[i, j, k] = occ[max(i - dilate, 0):i + dilate + 1, max(j - dilate, 0):j + dilate + 1,
                                   max(k - dilate, 0):k + dilate + 1].any()
    return out


def dilate_clipped_fast(occ, dilate):
    """The same by shifted ORs (for the larger test grids); ``test_skip_restate`` checks it against the loops."""
    out = occ.copy()
    for axis in range(3):
        acc = out.copy()
        for s in range(1, dilate + 1):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -s), slice(s, None)
            if out.shape[axis] > s:
                acc[tuple(hi)] |= out[tuple(lo)]
                acc[tuple(lo)] |= out[tuple(hi)]
        out = acc
    return out


def pack_bits(occ):
    """Cell ``g = (i * dy + j) * dz + k`` -> bit ``g & 31`` of word ``g >> 5``; uint32 ``[ceil(cells / 32)]``, unused bits 0."""
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, dtype=np.uint32)
    for g in np.nonzero(flat)[0]:
        words[g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    return words


def unpack_bits(words, dims):
    n = dims[0] * dims[1] * dims[2]
    g = np.arange(n)
    return (((np.asarray(words, dtype=np.uint32)[g >> 5] >> (g & 31).astype(np.uint32)) & 1) != 0).reshape(dims)


def build(sigma, threshold=0.0, dilate=1, fast=False):
    occ = occupied(sigma, threshold)
    return pack_bits((dilate_clipped_fast if fast else dilate_clipped)(occ, dilate))


def cell_centres(lo, hi, dims):
    """``lo + (idx + 0.5) * cell`` in f32 -> ``[dx dy dz, 3]`` in cell order."""
    lo, cell, _ = grid_consts(lo, hi, dims)
    ax = [((np.arange(dims[a], dtype=F) + F(0.5)) * cell[a] + lo[a]).astype(F) for a in range(3)]
    out = np.zeros(tuple(dims) + (3,), dtype=F)
    out[..., 0] = ax[0][:, None, None]
    out[..., 1] = ax[1][None, :, None]
    out[..., 2] = ax[2][None, None, :]
    return out.reshape(-1, 3)


def select(rays_o, rays_d, z, words, lo, hi, dims, outside="evaluate"):
    """-> ``(flag [N,S] uint8, sel int32 ascending, count)``.  The cell of a sample is ``_grid_restate.cells_f32``; inside: the
    cell's bit; outside (a NaN point included): 1 for ``"evaluate"``, 0 for ``"empty"``."""
    assert outside in ("evaluate", "empty")
    lo, _, inv = grid_consts(lo, hi, dims)
    inside, g = cells_f32(rays_o, rays_d, z, lo, inv, dims)
    occ = unpack_bits(words, dims).reshape(-1)
    flag = np.where(inside, occ[g], outside == "evaluate").astype(np.uint8)
    sel = np.nonzero(flag.reshape(-1))[0].astype(np.int32)
    return flag, sel, int(sel.size)


def mask_rows(rows, flag):
    """Rows whose flag is clear become exactly zero (what the sparse networks leave of a zero-filled buffer)."""
    rows = np.array(rows, copy=True)
    rows[np.asarray(flag) == 0] = 0
    return rows
