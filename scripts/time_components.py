"""Time the connected components of a label volume (field.LabelGrid.components / cleaned, field.Components.table).

    python scripts/time_components.py [--out profiles/components/timing.jsonl]
    python scripts/time_components.py --dims 256 --fills voronoi --legs components6       # one case, e.g. under a kernel trace

Volumes of ``--dims``^3 cells (default 128 and 256) at C = 14 over [-8, 8)^3: ``random5`` / ``random25`` / ``random100`` are
``T.random_labels`` at 5 / 25 / 100 % (noise: very many tiny components), ``voronoi`` is ``T.voronoi_labels`` (13 objects and 3 % of the
cells relabelled at random as strays).  Per row, milliseconds, median and minimum of ``--iters`` runs after ``--warmup``:

    components6 / components26         ``LabelGrid.components(connectivity)``, HIP events
    cleaned_min64 / cleaned_largest    ``cleaned(min_cells=64)`` / ``cleaned(keep="largest")`` at connectivity 6 on a ``LabelGrid``, HIP events
    baked_min64 / baked_largest        the same on a ``BakedGrid``
    table                              ``components(6).table()``, host clock round a synchronise: its host read is part of the cost
    scipy                              what a caller had to do before, host clock: ``labels.cpu()``, ``scipy.ndimage.label`` per label at
                                       connectivity 6, the ids back on the device; ``--yardstick-iters`` runs after one warm-up.  Where scipy
                                       does not import the row says so and the other times stand as absolute

and the number of components at both connectivities.  The first line records the device and its clocks (sclk among them) as
``rocm-smi`` reports them (read-only).  One JSON object per line."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

C = 14
FILLS = ("random5", "random25", "random100", "voronoi")
LEGS = ("components6", "components26", "cleaned_min64", "cleaned_largest", "baked_min64", "baked_largest", "table", "scipy")


def volume(fill, dims):
    if fill == "voronoi":
        return T.voronoi_labels(dims, C - 1, C)
    return T.random_labels(int(fill[len("random"):]), dims, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-iters", type=int, default=7)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--fills", nargs="+", default=list(FILLS), choices=FILLS)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    from dm_nerf_amd import field as F
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    dev = torch.device("cuda")
    lo, hi = T.BOX
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, yardstick_iters=a.yardstick_iters, C=C, scipy=ndimage is not None)]
    print(lines[0], flush=True)
    for dims in a.dims:
        for fill in a.fills:
            labels = torch.from_numpy(volume(fill, dims)).to(dev)
            grid = F.LabelGrid.from_labels(labels, lo, hi, C)
            cells = torch.randn(dims, dims, dims, 4, generator=torch.Generator(device=dev).manual_seed(0), device=dev)
            cells[labels == T.UNLABELLED] = 0.0
            baked = F.BakedGrid.from_arrays(labels, cells, lo, hi, C)
            row = {"leg": "components", "dims": dims, "fill": fill, "labelled_fraction": float((labels < C).float().mean())}
            for conn in (6, 26):
                comp = grid.components(conn)
                row[f"components_{conn}"] = int((comp.root.reshape(-1) == torch.arange(dims ** 3, dtype=torch.int32, device=dev)).sum())
            outs = {g: g.cleaned()[0] for g in (grid, baked)}

            def yardstick():
                host = labels.cpu().numpy()
                ids, k0 = np.zeros(host.shape, np.int32), 0
                for l in range(C):
                    lab, k = ndimage.label(host == l, structure=ndimage.generate_binary_structure(3, 1))
                    ids[lab > 0] = lab[lab > 0] + k0
                    k0 += k
                return torch.from_numpy(ids).to(dev)

            legs = {"components6": (T.time_events, lambda: grid.components(6)), "components26": (T.time_events, lambda: grid.components(26)),
                    "cleaned_min64": (T.time_events, lambda: grid.cleaned(min_cells=64, out=outs[grid])),
                    "cleaned_largest": (T.time_events, lambda: grid.cleaned(keep="largest", out=outs[grid])),
                    "baked_min64": (T.time_events, lambda: baked.cleaned(min_cells=64, out=outs[baked])),
                    "baked_largest": (T.time_events, lambda: baked.cleaned(keep="largest", out=outs[baked])),
                    "table": (T.time_host, lambda: grid.components(6).table()), "scipy": (T.time_host, yardstick)}
            for name in a.legs:
                timer, fn = legs[name]
                if name == "scipy":
                    if ndimage is None:
                        row["scipy"] = "scipy does not import here: the times stand as absolute"
                        continue
                    t = timer(fn, a.yardstick_iters, 1)
                else:
                    t = timer(fn, a.iters, a.warmup)
                row[name + "_ms_median"], row[name + "_ms_min"] = t.median, t.min
            if "scipy_ms_median" in row and "components6_ms_median" in row:
                row["scipy_over_components6"] = row["scipy_ms_median"] / row["components6_ms_median"]
            print(row, flush=True)
            lines.append(row)
    T.write_jsonl(lines, a.out, echo=False)


if __name__ == "__main__":
    main()
