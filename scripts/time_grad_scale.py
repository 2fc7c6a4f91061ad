import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _timing as T  # noqa: E402

from dm_nerf_amd import _lib  # noqa: E402

T.require_gpu(__file__)
lib = _lib.load()
dev = torch.device("cuda:0")
for n in (786432 * 18, 262144 * 18, 1000003):
    g = torch.randn(n, device=dev) * 1e-5
    g[n // 3] = 3.7e-4
    sc = torch.zeros(4, device=dev)

    def calls(k):
        for _ in range(k):
            _lib.check(lib.dmnerf_grad_scale(_lib.ptr(g), n, _lib.ptr(sc), _lib.stream()), "gs")

    calls(3)
    ms = T.time_events(lambda: calls(20), 1, 0).median / 20
    mx = float(g.abs().max())
    want = 2.0 ** (6 - math.frexp(mx)[1])
    print(n, "us per call", ms * 1e3, "scale", sc.tolist()[:2], "want", want, "GB/s", n * 4 / (ms * 1e-3) / 1e9)
    assert sc[0].item() == want and sc[2].item() == 0 and sc[3].item() == 0
