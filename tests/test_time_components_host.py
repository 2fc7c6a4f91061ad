"""scripts/time_components.py without a device: the two checks tests/test_timing_scripts.py makes of the other timing scripts (it
parses its arguments before it touches the device; without a device it fails in the one way ``_timing.require_gpu`` fails), and the
Voronoi fixture it adds to scripts/_timing.py."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
NAME = "time_components"


@pytest.fixture
def timing(monkeypatch):
    monkeypatch.setattr(sys, "path", [SCRIPTS] + sys.path)           # (the scripts put entries on the path: restored after the test)
    import _timing
    return _timing


def run_main(argv, monkeypatch):
    path = os.path.join(SCRIPTS, NAME + ".py")
    monkeypatch.setattr(sys, "argv", [path] + argv)
    spec = importlib.util.spec_from_file_location("_script_under_test_" + NAME, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    with pytest.raises(SystemExit) as e:
        module.main()
    return e.value


def test_help_comes_before_any_device_use(timing, monkeypatch, capsys):
    assert run_main(["--help"], monkeypatch).code == 0
    assert "usage:" in capsys.readouterr().out


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the script would measure")
def test_one_failure_without_a_device(timing, monkeypatch):
    with pytest.raises(SystemExit) as want:
        timing.require_gpu(NAME + ".py")
    assert run_main([], monkeypatch).code == want.value.code == f"{NAME}.py measures on the GPU: no device found"


def test_voronoi_fixture(timing):
    v = timing.voronoi_labels(12, 5, 7, stray_pct=0.0, seed=1)
    points = np.random.RandomState(1).randint(0, 12, size=(5, 3))
    idx = np.stack(np.indices((12,) * 3), axis=-1)
    d2 = ((idx[..., None, :] - points) ** 2).sum(-1)
    assert v.dtype == np.uint8 and np.array_equal(v, np.argmin(d2, axis=-1))
    w = timing.voronoi_labels(12, 5, 7, stray_pct=10.0, seed=1)
    changed = w != v
    assert 0 < changed.mean() < 0.1 and w.max() < 7 and np.array_equal(w, timing.voronoi_labels(12, 5, 7, stray_pct=10.0, seed=1))
