"""Generate ``tests/golden/surface.npz`` by RUNNING scikit-image's marching cubes (an interpreter that has scikit-image 0.18, the
generation the reference's own calls target; run by hand, never by the suite):

    python3.9 tests/golden/make_golden_surface.py          # writes tests/golden/surface.npz next to this file

Imports numpy and skimage only, nothing from the package.  Ten float32 fields that look like an occupancy -- a sum of a few Gaussians
pushed through ``1 - exp(-k f)`` -- with seeds 0, 1, 2 at 9^3, 17^3 and 33^3 and one at 9 x 13 x 17.  Per field ``<n>``:

  * ``field_<n>``;
  * ``lew_v_<n>`` / ``lew_f_<n>`` / ``lew_vol_<n>`` / ``lew_area_<n>``: vertices, faces, signed volume and area of
    ``marching_cubes(field, level=0.45, gradient_direction='ascent')`` (Lewiner, the reference's call, mesh_generator.py:68);
  * ``lor_*_<n>``: the same with ``method='lorensen'``;
  * ``vertex_tol_<n>``: 4 d, d = the largest coordinate difference between Lewiner's vertices and ``i + (level - a) / (b - a)`` in
    float32 on the sign-crossing grid edges, both sorted lexicographically.

It refuses to write unless, on every field: no grid value is within 1e-6 of the level; Lewiner's vertex count equals the number of
sign-crossing grid edges; both methods give the same vertex set and face count; every mesh edge is in exactly two triangles;
d <= 1e-4.  ``names`` lists the fields.
"""
import os

import numpy as np
from skimage.measure import marching_cubes

HERE = os.path.dirname(os.path.abspath(__file__))
LEVEL = 0.45
SHAPES = [((n, n, n), seed) for n in (9, 17, 33) for seed in (0, 1, 2)] + [((9, 13, 17), 0)]


def make_field(shape, seed):
    rng = np.random.default_rng(1000 * seed + shape[0] + 7 * shape[2])
    grid = np.stack(np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij"), axis=-1)
    f = np.zeros(shape)
    for _ in range(int(rng.integers(2, 5))):
        centre = rng.uniform(0.3, 0.7, size=3)
        width = rng.uniform(0.07, 0.13, size=3)
        f += rng.uniform(0.6, 1.4) * np.exp(-(((grid - centre) / width) ** 2).sum(-1) / 2.0)
    return (1.0 - np.exp(-3.0 * f)).astype(np.float32)


def crossing_vertices(v, level):
    """``i + t`` on every sign-crossing grid edge, ``t = (level - a) / (b - a)`` in float32."""
    f = np.float32
    lvl = f(level)
    inside = v > lvl
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(None, -1), slice(1, None)
        idx = np.nonzero(inside[tuple(lo)] != inside[tuple(hi)])
        va, vb = v[tuple(lo)][idx], v[tuple(hi)][idx]
        t = ((lvl - va).astype(f) / (vb - va).astype(f)).astype(f)
        pos = np.stack(idx, axis=-1).astype(f)
        pos[:, a] = (pos[:, a] + t).astype(f)
        out.append(pos)
    return np.concatenate(out)


def lexsorted(v):
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))]


def volume_area(v, faces):
    p = v.astype(np.float64)[faces]
    vol = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum() / 2.0
    return np.float64(vol), np.float64(area)


def undirected_edge_counts(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def main():
    out = {}
    names = []
    for shape, seed in SHAPES:
        name = "x".join(map(str, shape)) + f"_s{seed}"
        v = make_field(shape, seed)
        assert float(np.abs(v.astype(np.float64) - LEVEL).min()) > 1e-6, name
        want = crossing_vertices(v, LEVEL)
        lew_v, lew_f, _, _ = marching_cubes(v, level=LEVEL, gradient_direction="ascent")
        lor_v, lor_f, _, _ = marching_cubes(v, level=LEVEL, gradient_direction="ascent", method="lorensen")
        assert len(want) > 0 and lew_v.shape[0] == want.shape[0], (name, lew_v.shape, want.shape)
        assert lor_v.shape == lew_v.shape and lor_f.shape == lew_f.shape, name
        assert np.array_equal(lexsorted(lew_v), lexsorted(lor_v)), name
        for faces in (lew_f, lor_f):
            assert (undirected_edge_counts(faces) == 2).all(), name
        d = float(np.abs(lexsorted(lew_v).astype(np.float64) - lexsorted(want).astype(np.float64)).max())
        assert d <= 1e-4, (name, d)
        names.append(name)
        out[f"field_{name}"] = v
        for tag, (mv, mf) in (("lew", (lew_v, lew_f)), ("lor", (lor_v, lor_f))):
            vol, area = volume_area(mv, mf)
            out[f"{tag}_v_{name}"] = mv.astype(np.float32)
            out[f"{tag}_f_{name}"] = mf.astype(np.int32)
            out[f"{tag}_vol_{name}"] = vol
            out[f"{tag}_area_{name}"] = area
        out[f"vertex_tol_{name}"] = np.float64(4.0 * d)
        print(f"{name}: V {lew_v.shape[0]} F {lew_f.shape[0]} d {d:.3e} vol {out[f'lew_vol_{name}']:.4f} / {out[f'lor_vol_{name}']:.4f}")
    out["names"] = np.array(names)
    out["level"] = np.float64(LEVEL)
    path = os.path.join(os.environ.get("DMNERF_GOLDEN_OUT", HERE), "surface.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
