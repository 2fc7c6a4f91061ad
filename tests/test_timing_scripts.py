"""The stand-alone timing scripts (scripts/time_*.py) and the module they share (scripts/_timing.py), without a device: every script
parses its arguments before it touches the device and fails in one way when there is none; the shared fixtures are the constructions
the scripts carried before, written out here; the reduction of a list of runs is the median (the mean of the two middle runs of an
even count), the minimum and the maximum."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
PORTED = ("time_skip", "time_manip_skip", "time_mark", "time_train_skip", "time_field_edit", "time_label_grid", "time_label_trace",
          "time_baked", "time_volume_edit", "time_object_surfaces", "time_occupancy", "time_surface", "time_lpips", "time_img_metrics",
          "time_ins_eval", "time_edit_frame", "time_edit_kinds")


@pytest.fixture
def timing(monkeypatch):
    monkeypatch.setattr(sys, "path", [SCRIPTS] + sys.path)           # (the scripts put entries on the path: restored after the test)
    import _timing
    return _timing


def run_main(name, argv, monkeypatch):
    path = os.path.join(SCRIPTS, name + ".py")
    monkeypatch.setattr(sys, "argv", [path] + argv)
    spec = importlib.util.spec_from_file_location("_script_under_test_" + name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    with pytest.raises(SystemExit) as e:
        module.main()
    return e.value


@pytest.mark.parametrize("name", PORTED)
def test_help_comes_before_any_device_use(name, timing, monkeypatch, capsys):
    assert run_main(name, ["--help"], monkeypatch).code == 0
    assert "usage:" in capsys.readouterr().out


@pytest.mark.skipif(torch.cuda.is_available(), reason="there is a device: the scripts would measure")
@pytest.mark.parametrize("name", PORTED)
def test_one_failure_without_a_device(name, timing, monkeypatch):
    with pytest.raises(SystemExit) as want:
        timing.require_gpu(name + ".py")
    assert run_main(name, [], monkeypatch).code == want.value.code == f"{name}.py measures on the GPU: no device found"


def test_fixtures_are_the_scripts_constructions(timing):
    T = timing
    for d in (8, 5):                                                 # (5: 125 bits are no whole number of words)
        for pct in (0, 5, 100):
            occ = np.random.RandomState(pct).rand(d, d, d) < pct / 100.0
            words = np.packbits(occ.reshape(-1), bitorder="little")
            words = np.concatenate([words, np.zeros(-words.size % 4, np.uint8)]).view(np.uint32)
            got = T.random_bits(pct, d)
            assert got.dtype == np.uint32 and np.array_equal(got, words)
            assert np.array_equal(T.pack_bits(occ), words)
            assert int(sum(bin(w).count("1") for w in got)) == int(occ.sum())
            # time_label_trace.py's volume (C = 14) and time_field_edit.py's (labels 0 .. 12)
            for C in (14, 13):
                rng = np.random.RandomState(pct)
                vol = rng.randint(0, C, size=(d,) * 3).astype(np.uint8)
                vol[rng.rand(d, d, d) >= pct / 100.0] = 255
                got = T.random_labels(pct, d, C)
                assert got.dtype == np.uint8 and np.array_equal(got, vol)
            # time_baked.py's and time_volume_edit.py's volume
            rng = np.random.RandomState(pct)
            set_cells = rng.rand(d, d, d) < pct / 100.0
            vol = rng.randint(0, 14, size=(d,) * 3).astype(np.uint8)
            vol[~set_cells] = 255
            cells = np.zeros((d, d, d, 4), np.float32)
            cells[..., :3] = rng.randn(d, d, d, 3)
            cells[..., 3] = rng.uniform(0.0, 8.0, size=(d, d, d))
            cells[~set_cells] = 0.0
            got = T.random_baked(pct, d, 14)
            assert np.array_equal(got[0], set_cells) and np.array_equal(got[1], vol) and np.array_equal(got[2], cells)
            assert got[1].dtype == np.uint8 and got[2].dtype == np.float32
    assert np.array_equal(T.random_bits(5, 8, seed=3), T.pack_bits(np.random.RandomState(3).rand(8, 8, 8) < 0.05))
    assert T.UNLABELLED == 255 and T.BOX == ((-8.0, -8.0, -8.0), (8.0, 8.0, 8.0)) and (T.H, T.W) == (480, 640)

    for e in (0, 7):                                                 # time_volume_edit.py's series
        ang = 0.1 + 0.02 * e
        want = np.array([[np.cos(ang), -np.sin(ang), 0., 0.3 + 0.05 * e], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1 * (e % 5)],
                         [0., 0., 0., 1.]])
        got = T.rigid(e, series="volume")
        assert got.dtype == np.float64 and np.array_equal(got, want)
    for k in (0, 3):                                                 # time_field_edit.py's series
        ang = 0.2 + 0.05 * k
        s = 1.0 if k % 2 == 0 else -1.0
        want = np.array([[np.cos(ang), -np.sin(ang), 0., 0.3 * s], [np.sin(ang), np.cos(ang), 0., -0.2 + 0.02 * k], [0., 0., 1., 0.1 * s],
                         [0., 0., 0., 1.]], dtype=np.float64)
        got = T.rigid(k)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    ang = 0.2                                                        # the one move of time_manip_skip.py, time_label_trace.py, time_baked.py
    rows = [[np.cos(ang), -np.sin(ang), 0., 0.3], [np.sin(ang), np.cos(ang), 0., -0.2], [0., 0., 1., 0.1], [0., 0., 0., 1.]]
    assert np.array_equal(T.rigid(), np.array(rows, dtype=np.float64))
    assert torch.equal(torch.tensor(T.rigid(), dtype=torch.float32), torch.tensor(rows, dtype=torch.float32))

    from oracle import ref_cpu as O                                  # the study view: the benchmark's camera
    H, W, K, pose = T.study_view()
    assert (H, W) == (480, 640) and np.array_equal(np.asarray(K), np.asarray(O.dmsr_intrinsics(480, 640)))
    assert torch.equal(pose, O.pose_spherical(30.0, -65.0, 7.0)) and pose.device.type == "cpu"


def test_reduction_is_median_min_max(timing):
    assert timing.reduce_ms([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert timing.reduce_ms([4.0, 1.0, 3.0, 2.0]) == (2.5, 1.0, 4.0)     # an even count: the mean of the two middle runs, not a run
    assert timing.reduce_ms([7.5]) == (7.5, 7.5, 7.5)
    assert all(type(v) is float for v in timing.reduce_ms(np.float32([1.0, 2.0])))
