"""The limit on a kernel's dynamic LDS is raised once per device by whichever entry launches the kernel first (csrc/common.h:
dmn_launch_lds).  Entries that share a kernel, or a kernel family, must therefore work in either order: a fresh process calls
them in the order opposite to the one the rest of the suite meets them in, and every output must be ``torch.equal`` to the same
call made here in the usual order.  A missing attribute would make a launch return an error code, which fails the test."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS_NUM, C = 13, 14
SHAPES = [(2, 3), (3, 43)]             # 6 samples: one ragged 32-sample block; 129: a second workgroup with one live lane
SENTINEL = 777.0
# (first, second) in the usual order; the child process swaps each pair
PAIRS = [("composite_fwd", "manipulator_render"), ("mlp_fwd_rays", "mlp_fwd_rays_sel"), ("mlp_fwd_rays_density", "mlp_fwd_rays_density_sel"),
         ("mlp_fwd_rays_density_f16", "mlp_fwd_rays_density_f16_sel"), ("composite_bwd", "composite_pen_bwd")]


def run(reverse):
    """Every entry of PAIRS on both shapes -> {label: output tensor on the CPU}; inputs come from seeded CPU generators."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import _gpu                            # after ROOT is on the path: the child process starts without it
    from dm_nerf_amd import _lib as L
    from oracle import ref_cpu as O
    lib = L.load()
    model = _gpu.model_from(O.make_weights(61, INS_NUM, gain=1.7, sigma_bias=0.3), INS_NUM)
    blob, blob_hd = model.blob(), model.blob_f16_density()
    out = {}

    def keep(label, rc, *tensors):
        assert rc == 0, (label, rc, L.last_error())
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            out[f"{label}/{i}"] = t.cpu()

    for N, S in SHAPES:
        g = torch.Generator().manual_seed(100 * N + S)
        rnd = lambda *shape: torch.rand(*shape, generator=g)
        ro, rd = (rnd(N, 3) - 0.5).cuda(), (rnd(N, 3) - 0.5).cuda()
        z = (4.0 + 11.0 * rnd(N, S)).sort(-1).values.cuda()
        raw = (2.0 * rnd(N, S, 4 + C) - 0.5).cuda()
        g_rgb, g_ins, g_depth, g_w = rnd(N, 3).cuda(), rnd(N, C - 1).cuda(), rnd(N).cuda(), rnd(N, S).cuda()
        g_part = torch.rand(N, 4, generator=g, dtype=torch.float64).cuda()
        half = torch.arange(0, N * S, 2, dtype=torch.int32).cuda()                       # every second sample
        sels = {"half": (half, torch.tensor([half.numel()], dtype=torch.int32).cuda()),
                "empty": (half, torch.zeros(1, dtype=torch.int32).cuda())}
        new = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
        fwd = {}                                                                          # composite_fwd's maps, read by the backward pair
        tag = f"N{N}S{S}"

        def composite(name, ncol):
            rgb, w, depth, ins = new(N, 3), new(N, S), new(N), new(N, ncol)
            rc = getattr(lib, "dmnerf_" + name)(L.ptr(raw), L.ptr(z), L.ptr(rd), N, S, C, L.ptr(rgb), L.ptr(w), L.ptr(depth), L.ptr(ins), L.stream())
            keep(f"{tag}/{name}", rc, rgb, w, depth, ins)
            fwd[name] = (ins, depth)

        def dense(name, b, width):
            o = new(N, S, width)
            keep(f"{tag}/{name}", getattr(lib, "dmnerf_" + name)(L.ptr(b), INS_NUM, L.ptr(ro), L.ptr(rd), L.ptr(z), N, S, L.ptr(o), L.stream()), o)

        def over_selection(name, b, width, *lead):
            for which, (sel, count) in sels.items():
                o = new(N, S, width)
                rc = getattr(lib, "dmnerf_" + name)(L.ptr(b), INS_NUM, *lead, L.ptr(ro), L.ptr(rd), L.ptr(z), N, S, L.ptr(sel), L.ptr(count), L.ptr(o),
                                                    L.stream())
                keep(f"{tag}/{name}/{which}", rc, o)

        def backward(name):
            ins, depth = fwd["composite_fwd"]
            grad = new(N, S, 4 + C)
            head = (L.ptr(raw), L.ptr(z), L.ptr(rd), L.ptr(ins))
            gs = (L.ptr(g_rgb), L.ptr(g_ins), L.ptr(g_depth), L.ptr(g_w))
            if name == "composite_bwd":
                rc = lib.dmnerf_composite_bwd(*head, *gs, N, S, C, L.ptr(grad), L.stream())
            else:
                rc = lib.dmnerf_composite_pen_bwd(*head, L.ptr(depth), *gs, L.ptr(g_part), N, S, C, 0.05, 0.005, 7.978845608, L.ptr(grad), L.stream())
            keep(f"{tag}/{name}", rc, grad)

        steps = {
            "composite_fwd": lambda: composite("composite_fwd", C - 1),
            "manipulator_render": lambda: composite("manipulator_render", C),
            "mlp_fwd_rays": lambda: dense("mlp_fwd_rays", blob, 4 + C),
            "mlp_fwd_rays_sel": lambda: over_selection("mlp_fwd_rays_sel", blob, 4 + C, 0),
            "mlp_fwd_rays_density": lambda: dense("mlp_fwd_rays_density", blob, 1),
            "mlp_fwd_rays_density_sel": lambda: over_selection("mlp_fwd_rays_density_sel", blob, 1),
            "mlp_fwd_rays_density_f16": lambda: dense("mlp_fwd_rays_density_f16", blob_hd, 1),
            "mlp_fwd_rays_density_f16_sel": lambda: over_selection("mlp_fwd_rays_density_f16_sel", blob_hd, 1),
            "composite_bwd": lambda: backward("composite_bwd"),
            "composite_pen_bwd": lambda: backward("composite_pen_bwd"),
        }
        for pair in PAIRS:
            for name in (pair[::-1] if reverse else pair):
                steps[name]()
    return out


@pytest.mark.gpu
def test_entries_that_share_a_kernel_work_in_either_order(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    want = run(reverse=False)
    path = str(tmp_path / "reversed.pt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    got = torch.load(path)
    assert sorted(got) == sorted(want) and len(want) == len(SHAPES) * (2 * 4 + 3 * (1 + 2) + 2)
    for label in want:
        assert torch.equal(got[label], want[label]), label
    sel_rows = want["N3S43/mlp_fwd_rays_sel/half/0"].reshape(-1, 4 + C)
    assert not bool((sel_rows[0::2] == SENTINEL).any()) and bool((sel_rows[1::2] == SENTINEL).all())    # the selection was honoured
    assert bool((want["N3S43/mlp_fwd_rays_sel/empty/0"] == SENTINEL).all())
    assert torch.equal(sel_rows[0::2], want["N3S43/mlp_fwd_rays/0"].reshape(-1, 4 + C)[0::2])


if __name__ == "__main__":                # the child: a fresh process in which no entry has run, the pairs swapped
    torch.save(run(reverse=True), sys.argv[1])
