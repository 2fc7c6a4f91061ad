"""Time the label grid (field.label_grid, LabelGrid.stats, LabelGrid.skip_grid) by the fraction of set cells.

    python scripts/time_label_grid.py [--out profiles/label_grid/timing_f32.jsonl]
    python scripts/time_label_grid.py --mfma-split f16x2 [--out profiles/label_grid/timing_f16x2.jsonl]

A 128^3 grid over [-8, 8)^3, ins_num 13, the benchmark's fine model; ``occ`` is synthetic: cells set at random with probability 5, 25
and 100 %.  Per row, HIP-event milliseconds, median and minimum of ``--iters`` runs after ``--warmup``:

    label_grid     the whole call (slabs of 2^20 cells: rays, select-and-fill, sparse network, label pass)
    network        the same slabs through ``label_rays`` + ``run_network_skip`` only
    label_pass     ``dmnerf_label_cells`` over the slabs' rows, on a buffer of network rows that is already there
    stats          ``LabelGrid.stats()`` (``dmnerf_label_stats`` and the float64 quantities derived from it)
    skip_grid      ``LabelGrid.skip_grid(k)`` of the most frequent label, without dilation

and the evaluated fraction (samples evaluated / samples, counted on the device by ``run_network_skip(counts=)``) and the labelled
fraction.  There is no earlier implementation to compare against: these are absolute times of this tree.  The first line records
the device and its clocks (sclk among them) as ``rocm-smi`` reports them (read-only).  One JSON object per line."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dims", type=int, default=128)
    ap.add_argument("--mfma-split", default=None, choices=["f16x2"], help="the network kernels (default: f32)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T.require_gpu(__file__)
    import bench_common as C
    from dm_nerf_amd import _lib, field as F
    from dm_nerf_amd.networks import render as R
    dev = torch.device("cuda")
    _, _, _, mf = C.build_models(dev, ins_num=13)
    n_logits = mf.ins_num + 1
    (lo, hi), dims = T.BOX, (a.dims,) * 3
    slab = 1 << 20
    step = max(1, slab // (dims[1] * dims[2]))
    lines = [T.device_line(iters=a.iters, warmup=a.warmup, dims=a.dims, ins_num=mf.ins_num, mfma_split=a.mfma_split)]
    lib = _lib.load()
    rng = np.random.RandomState(0)
    with torch.no_grad():
        for p in (0.05, 0.25, 1.0):
            cells = rng.rand(a.dims ** 3) < p                        # (one generator through the three rows, not random_bits' seed per row)
            occ = F.SkipGrid.full(lo, hi, dims, device=dev) if p == 1.0 else F.SkipGrid.from_bits(T.pack_bits(cells), lo, hi, dims, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)

            def network(counts=None):
                for i0 in range(0, dims[0], step):
                    o, d, z = F.label_rays(occ, i0, min(i0 + step, dims[0]))
                    R.run_network_skip(mf, o, d, z, occ, split=a.mfma_split, counts=counts)

            network(counts)
            evaluated, samples = counts.tolist()
            o, d, z = F.label_rays(occ, 0, step)
            raw = R.run_network_skip(mf, o, d, z, occ, split=a.mfma_split)
            out = torch.empty(raw.shape[0] * raw.shape[1], dtype=torch.uint8, device=dev)

            def label_pass():
                for _ in range(0, dims[0], step):
                    _lib.check(lib.dmnerf_label_cells(_lib.ptr(raw), out.numel(), n_logits, 0.0, _lib.ptr(out), _lib.stream()),
                               "dmnerf_label_cells")

            lg = F.label_grid(mf, occ, slab=slab, split=a.mfma_split)
            top = int(torch.bincount(lg.labels.reshape(-1).long(), minlength=256)[:n_logits].argmax())
            row = {"leg": "label_grid", "set_fraction": float(occ.occupancy()), "evaluated_fraction": evaluated / samples,
                   "labelled_fraction": float((lg.labels != F.UNLABELLED).float().mean()), "top_label": top}
            for name, fn in (("label_grid", lambda: F.label_grid(mf, occ, slab=slab, split=a.mfma_split)), ("network", network),
                             ("label_pass", label_pass), ("stats", lg.stats), ("skip_grid", lambda: lg.skip_grid(top))):
                t = T.time_events(fn, a.iters, a.warmup)
                row[name + "_ms_median"], row[name + "_ms_min"] = t.median, t.min
            lines.append(row)
    T.write_jsonl(lines, a.out)


if __name__ == "__main__":
    main()
