"""Time ``field.object_surfaces`` (csrc/object_surface.hip) against what a caller had to write before it: the loop over the labels
round ``field.extract_surface`` on ``torch.where(labels == k, value, 0)``, which is the parent commit's code, in the same session.

    python scripts/time_object_surfaces.py                    # 128^3 and 256^3, ins_num 13 and 93; one JSON object per line
    python scripts/time_object_surfaces.py --dims 128 --ins-nums 13

Synthetic volumes: Voronoi labels of ``ins_num + 1`` random seeds (every label present), a smooth field of Gaussian blobs through
the occupancy activation, about 2.5 % of the cells unlabelled.  Host clock round a device synchronise (both routes read totals on
the host, so that is what a caller waits for), median (``*_ms``) and minimum (``*_ms_min``) of ``--iters`` after ``--warmup`` runs.  The first line records the device and
its clocks (sclk among them, read-only).

    loop_open_ms     the per-label loop on the volume as it is: open meshes where an object touches the box (C extracts, C host reads)
    loop_closed_ms   the same loop on a volume padded by one point (the referee of ``closed=True``), the padded copy made once
    one_pass_ms      ``object_surfaces(closed=True)``; ``one_pass_open_ms`` with ``closed=False``
    count_ms / emit_ms / sort_ms   the parts of the closed single pass: count kernel + scans + the read of the totals, the two emit
                     kernels, and the two sorts + gathers + searchsorted
    measures_ms      ``ObjectSurfaces.measures()``"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402


def synthetic(dim, C, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ax = torch.arange(dim, dtype=torch.float32, device="cuda")
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    seeds = torch.rand(C, 3, generator=g, device="cuda") * (dim - 1)
    best = torch.full((dim, dim, dim), float("inf"), device="cuda")
    labels = torch.zeros(dim, dim, dim, dtype=torch.uint8, device="cuda")
    for k in range(C):
        d2 = ((grid - seeds[k]) ** 2).sum(-1)
        labels = torch.where(d2 < best, torch.full_like(labels, k), labels)
        best = torch.minimum(best, d2)
    value = torch.zeros(dim, dim, dim, device="cuda")
    for _ in range(12):
        c, r = torch.rand(3, generator=g, device="cuda") * (dim - 1), (0.15 + 0.2 * float(torch.rand(1, generator=g, device="cuda"))) * dim
        value += torch.exp(-((grid - c) ** 2).sum(-1) / (2.0 * r * r))
    value = (1.0 - torch.exp(-0.9 * value)).contiguous()
    labels[torch.rand(dim, dim, dim, generator=g, device="cuda") < 0.025] = 255
    return labels.contiguous(), value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ins-nums", type=int, nargs="+", default=[13, 93])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--level", type=float, default=0.45)
    a = ap.parse_args()
    T.require_gpu(__file__)

    import ctypes

    import torch
    from dm_nerf_amd import _lib, field as F

    print(json.dumps(T.device_line(iters=a.iters, warmup=a.warmup)), flush=True)
    for dim in a.dims:
        for ins_num in a.ins_nums:
            C = ins_num + 1
            labels, value = synthetic(dim, C, 100 * dim + ins_num)
            grid = F.LabelGrid.from_labels(labels, *T.BOX, C)
            zero = torch.zeros_like(value)

            def loop(lab, val):
                out = []
                for k in range(C):
                    out.append(F.extract_surface(torch.where(lab == k, val, torch.zeros_like(val)), a.level))
                return out

            def loop_closed():
                lab = torch.nn.functional.pad(labels, (1,) * 6, value=255).contiguous()
                val = torch.nn.functional.pad(value, (1,) * 6, value=0.0).contiguous()
                return loop(lab, val)

            surf = F.object_surfaces(grid, value, a.level)
            ref = loop_closed()
            vo = surf.vertex_offset.tolist()
            assert all(torch.equal(ref[k][0] - 1.0, surf.vertices[vo[k]:vo[k + 1]]) for k in range(C)), "the single pass differs from the loop"
            line = {"leg": "object_surfaces", "dim": dim, "ins_num": ins_num, "C": C, "vertices": int(surf.vertices.shape[0]),
                    "triangles": int(surf.faces.shape[0]), "objects": int((surf.face_offset[1:] > surf.face_offset[:-1]).sum())}

            def timed(name, fn):
                t = T.time_host(fn, a.iters, a.warmup)
                line[name + "_ms"], line[name + "_ms_min"] = t.median, t.min

            timed("loop_open", lambda: loop(labels, value))
            timed("loop_closed", loop_closed)
            timed("one_pass", lambda: F.object_surfaces(grid, value, a.level))
            timed("one_pass_open", lambda: F.object_surfaces(grid, value, a.level, closed=False))
            line["ratio_closed"] = line["loop_closed_ms"] / line["one_pass_ms"]
            line["ratio_open"] = line["loop_open_ms"] / line["one_pass_open_ms"]

            # the parts of the closed pass, through the entries themselves
            mask = (ctypes.c_uint32 * 4)(*F.label_mask_words(range(C), C))
            head = (value, labels, dim, dim, dim, C, mask, a.level, 1)
            n = (dim + 2) ** 3
            counts = torch.empty(2, n, dtype=torch.uint8, device="cuda")
            state = {}

            def count():
                _lib.launch("dmnerf_object_surface_count", *head, counts[0], counts[1])
                state["scans"] = torch.cumsum(counts, dim=1, dtype=torch.int64)
                state["V"], state["F"] = state["scans"][:, -1].tolist()
            count()
            V, Fn = state["V"], state["F"]
            vkey, vpos = torch.empty(V, dtype=torch.int64, device="cuda"), torch.empty(V, 3, device="cuda")
            vcell = torch.empty(V, dtype=torch.int32, device="cuda")
            tkey, ckey = torch.empty(Fn, dtype=torch.int64, device="cuda"), torch.empty(Fn, 3, dtype=torch.int64, device="cuda")

            def emit():
                _lib.launch("dmnerf_object_surface_emit", *head, counts[0], counts[1], state["scans"][0], state["scans"][1], V, Fn, vkey, vpos,
                            vcell, tkey, ckey)

            def sort():
                vk, vorder = torch.sort(vkey)
                tk, torder = torch.sort(tkey)
                return vpos[vorder], vcell[vorder], torch.searchsorted(vk, ckey[torder]).to(torch.int32)
            emit()
            timed("count", count)
            timed("emit", emit)
            timed("sort", sort)
            timed("measures", surf.measures)
            print(json.dumps(line), flush=True)
            del surf, ref, zero


if __name__ == "__main__":
    main()
