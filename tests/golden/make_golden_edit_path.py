"""Generate tests/golden/edit_path.npz by RUNNING THE REFERENCE's ``manipulator_demo`` (build container only).

    python tests/golden/make_golden_edit_path.py          # needs the reference checkout (DMNERF_REFERENCE)

The function (networks/manipulator.py:367-491) is CALLED unmodified, on the pattern of ``make_golden.py::gen_manipulator_frame``:
cwd = the reference (its ``./data/color_dict.json``), image / metric / mesh modules stubbed, ``manipulator`` and ``sample_pdf``
wrapped by recorders, ``imageio.imwrite`` / ``cv2.imwrite`` replaced by recorders of the arrays they are handed.  Two runs, each two
views of a 10 x 16 frame with N_test = 64 (160 rays per view: chunks of 64, 64 and a ragged 32), ins_num = 7, the PEAKY weights of
seeds 721 / 722, ``torch.manual_seed(741)``:

  run a   two rigid objects (a translation and a rotation per view),
  run b   two deformed objects, ``sin`` and ``ex``.

Recorded per run (prefix ``a_`` / ``b_``): the view poses, per view the original and target ray batches of all chunks and the four
outputs the loop accumulates, the three images written (``*_rgb.png``, ``*_ins.png``, ``*_ins_pred_mask.png``); once: the colour
rows, ``color_dict`` and ``ins_map`` as plain arrays.  The ``2 + T`` draws of every chunk are NOT stored (1.3 MB of random bits):
the generator asserts that they are the successive ``torch.rand([n, 128])`` calls after the seed, so a test remakes them.
The file holds arrays only; no reference source travels.
"""
import os
import sys
import tempfile
import types
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("DMNERF_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from oracle import ref_cpu as O  # noqa: E402

for mod in ("imageio", "lpips", "cv2", "skimage", "skimage.metrics", "open3d", "matplotlib", "matplotlib.pyplot",
            "matplotlib.cm", "h5py", "configargparse", "trimesh"):
    sys.modules.setdefault(mod, MagicMock())

import networks.dm_nerf as R_model  # noqa: E402  (reference)
import networks.manipulator as R_mani  # noqa: E402

torch.autograd.set_detect_anomaly(False)  # the reference switches it on at import (dm_nerf.py:5)
torch.set_num_threads(1)                  # fixtures must not depend on the thread count

H_, W_, N_TEST, INS, SEED = 10, 16, 64, 7, 741
VIEWS = [(75.0, -65.0, 7.0), (60.0, -60.0, 7.0)]
INS_MAP = {"0": 0, "1": 3, "2": 5, "3": 1, "4": 12, "6": 7, "7": 9}      # label 5 has no entry: black in the object image


def _rot(ang, t):
    return [[np.cos(ang), -np.sin(ang), 0., t[0]], [np.sin(ang), np.cos(ang), 0., t[1]], [0., 0., 1., t[2]], [0., 0., 0., 1.]]


RUNS = {
    "a": dict(objs=[dict(obj_name="chair", tar_id=2, mani_mode="translation"), dict(obj_name="table", tar_id=4, mani_mode="rotation")],
              objs_trans={"chair": [dict(transformation=_rot(0.0, (0.3, -0.2, 0.1))), dict(transformation=_rot(0.0, (-0.4, 0.25, 0.0)))],
                          "table": [dict(transformation=_rot(0.2, (0.0, 0.0, 0.0))), dict(transformation=_rot(-0.35, (0.1, 0.0, 0.05)))]}),
    "b": dict(objs=[dict(obj_name="chair", tar_id=2, mani_mode="deform", deform_func="sin"),
                    dict(obj_name="table", tar_id=4, mani_mode="deform", deform_func="ex")],
              objs_trans={}),
}


def run(tag, spec, ins_rgbs):
    sd_c, sd_f = O.make_weights(721, INS, **O.PEAKY), O.make_weights(722, INS, **O.PEAKY)
    mc, mf = R_model.DM_NeRF(8, 256, 63, 27, [4], INS), R_model.DM_NeRF(8, 256, 63, 27, [4], INS)
    mc.load_state_dict(sd_c); mf.load_state_dict(sd_f)
    mc, mf = mc.eval(), mf.eval()
    pe, _ = R_model.get_embedder(10, 0); ve, _ = R_model.get_embedder(4, 0)
    K = O.dmsr_intrinsics(H_, W_)
    poses = [O.pose_spherical(*v) for v in VIEWS]
    T = len(spec["objs"])
    calls, pdf_us, written = [], [], []
    orig_m, orig_pdf = R_mani.manipulator, R_mani.sample_pdf
    orig_io, orig_cv = R_mani.imageio.imwrite, R_mani.cv2.imwrite

    def w_pdf(bins, weights, N, det=False):
        st = torch.get_rng_state()
        r = orig_pdf(bins, weights, N, det)
        after = torch.get_rng_state()
        torch.set_rng_state(st); u = torch.rand(list(weights.shape[:-1]) + [N]); torch.set_rng_state(after)
        pdf_us.append(u)
        return r

    def w_mani(p, v, c, f, ori_rays, tar_rays, a):
        k = len(pdf_us)
        r = orig_m(p, v, c, f, ori_rays, tar_rays, a)
        calls.append(dict(ori=ori_rays.clone(), tar=tar_rays.clone(), us=pdf_us[k:], out=[t.clone() for t in r], labels=list(a.target_labels)))
        return r

    def w_write(path, arr):
        written.append((os.path.basename(path), np.array(arr)))

    a = types.SimpleNamespace(N_samples=64, N_importance=128, near=4.0, far=15.0, N_test=N_TEST, datadir="./data/dmsr/study",
                              device="cpu", ins_num=INS, mani_type="golden")
    R_mani.manipulator, R_mani.sample_pdf = w_mani, w_pdf
    R_mani.imageio.imwrite, R_mani.cv2.imwrite = w_write, w_write
    cwd = os.getcwd()
    try:
        os.chdir(REF)
        with tempfile.TemporaryDirectory() as tmp, torch.no_grad():
            torch.manual_seed(SEED)
            R_mani.manipulator_demo(pe, ve, mc, mf, None, (H_, W_, K), spec["objs_trans"], tmp, ins_rgbs, spec["objs"], poses, INS_MAP, a)
    finally:
        os.chdir(cwd)
        R_mani.manipulator, R_mani.sample_pdf = orig_m, orig_pdf
        R_mani.imageio.imwrite, R_mani.cv2.imwrite = orig_io, orig_cv
    sizes = [64, 64, 32]
    assert [c["ori"].shape[1] for c in calls] == sizes * len(VIEWS), [c["ori"].shape for c in calls]
    assert all(len(c["us"]) == 2 + T and tuple(c["tar"].shape) == (T, 2, c["ori"].shape[1], 3) for c in calls)
    assert all(c["labels"] == [o["tar_id"] for o in spec["objs"]] for c in calls)
    # the draws are the successive torch.rand calls after the seed: a test remakes them instead of reading 1.3 MB of random bits
    torch.manual_seed(SEED)
    for c in calls:
        for u in c["us"]:
            assert torch.equal(u, torch.rand(c["ori"].shape[1], 128)), "draws are not the plain torch.rand stream"
    assert [w[0] for w in written] == [f"{i}_{s}.png" for i in range(len(VIEWS)) for s in ("rgb", "ins", "ins_pred_mask")]
    out = {f"{tag}_poses": torch.stack(poses)}
    for i in range(len(VIEWS)):
        cs = calls[3 * i:3 * i + 3]
        out[f"{tag}_ori_rays{i}"] = torch.cat([c["ori"] for c in cs], 1)                 # [2, 160, 3]
        out[f"{tag}_tar_rays{i}"] = torch.cat([c["tar"] for c in cs], 2)                 # [T, 2, 160, 3]
        for k, name in enumerate(("full_rgb", "full_ins", "full_tar_rgb", "full_tar_ins")):
            out[f"{tag}_{name}{i}"] = torch.cat([c["out"][k] for c in cs], 0)
        for k, name in enumerate(("rgb8", "ins_img", "mask")):
            arr = written[3 * i + k][1]
            assert arr.dtype == np.uint8 and arr.shape[:2] == (H_, W_), (name, arr.dtype, arr.shape)
            out[f"{tag}_{name}{i}"] = arr
    labels = torch.cat([out[f"{tag}_full_ins{i}"] for i in range(len(VIEWS))]).argmax(-1)
    print(f"  run {tag}: {len(calls)} chunks, final labels {np.bincount(labels.numpy(), minlength=INS + 1).tolist()}")
    return out


def main():
    import json
    color_dict = json.load(open(os.path.join(REF, "data", "color_dict.json")))["dmsr"]["study"]
    ins_rgbs = np.random.RandomState(9).randint(1, 256, size=(max(color_dict.values()) + 1, 3))
    out = dict(HWN=np.array([H_, W_, N_TEST]), ins_num=np.int64(INS), seeds=np.array([721, 722]), rng_seed=np.int64(SEED),
               K=O.dmsr_intrinsics(H_, W_), ins_rgbs=ins_rgbs.astype(np.int64),
               color_dict=np.array([[int(k), int(v)] for k, v in color_dict.items()], dtype=np.int64),
               ins_map=np.array([[int(k), int(v)] for k, v in INS_MAP.items()], dtype=np.int64))
    for tag, spec in RUNS.items():
        out.update(run(tag, spec, ins_rgbs))
        out[f"{tag}_tar_id"] = np.array([o["tar_id"] for o in spec["objs"]], dtype=np.int64)
    out["a_trans"] = np.array([[RUNS["a"]["objs_trans"][o["obj_name"]][i]["transformation"] for i in range(len(VIEWS))]
                               for o in RUNS["a"]["objs"]], dtype=np.float32)                  # [T, views, 4, 4]
    out["b_func"] = np.array([["sin", "ex"].index(o["deform_func"]) for o in RUNS["b"]["objs"]], dtype=np.int64)   # 0 sin, 1 ex
    path = os.path.join(os.environ.get("DMNERF_GOLDEN_OUT", HERE), "edit_path.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()})
    size = os.path.getsize(path)
    assert size <= 1 << 20, size
    print(f"  wrote edit_path.npz  ({size / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
