"""dm_nerf_amd.dropin: the reference's own modules load unmodified and exactly their hot-path names are rebound, before
other reference modules copy them.  The checkout is a stand-in the test writes (the reference's module layout and its
import-time copies of hot-path names, placeholder bodies); DMNERF_REFERENCE=<a DM-NeRF checkout> runs the same probe on a
real one.  It is run in a subprocess so that the checkout's import side effects (the reference switches anomaly detection on,
dm_nerf.py:5) stay out of this session."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DMNERF_REFERENCE")

# the stand-in: what each module copies from the others at import, as the reference's do (config.py:6, render.py:3,
# tester.py:11-13, manipulator.py:12-14), and the names beyond dropin.PATCHES that the probe checks are NOT rebound
STAND_IN_IMPORTS = {"config": "from networks.dm_nerf import get_embedder, DM_NeRF\n",
                    "networks.render": "from networks.helpers import sample_pdf\n",
                    "networks.tester": "from networks.render import dm_nerf\nfrom networks.evaluator import to8b, ins_eval\n"
                                       "from networks.helpers import get_rays_k, z_val_sample\n",
                    "networks.manipulator": "from networks.evaluator import to8b, ins_eval\nfrom networks.helpers import get_rays_k, sample_pdf\n"}
STAND_IN_OWN = {"config": ["initial"], "networks.helpers": ["get_rays"], "networks.evaluator": ["calculate_ap", "to8b", "ins_eval"],
                "networks.tester": ["render_test"]}


def _stand_in_checkout(root):
    """A checkout with the reference's layout -- config.py beside a ``networks`` namespace package -- whose modules define every
    name of dropin.PATCHES (placeholders) and copy each other's hot-path names at import as the reference's modules do."""
    import dm_nerf_amd.dropin as D
    for mod in sorted(set(D.PATCHES) | set(STAND_IN_IMPORTS) | set(STAND_IN_OWN)):
        src = STAND_IN_IMPORTS.get(mod, "")
        for name in list(D.PATCHES.get(mod, {})) + STAND_IN_OWN.get(mod, []):
            src += (f"\n\nclass {name}:\n    pass\n" if name[0].isupper() else
                    f"\n\ndef {name}(*args, **kwargs):\n    raise NotImplementedError('stand-in')\n")
        path = os.path.join(root, *mod.split(".")) + ".py"
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(src)
    return root


PROBE = r'''
import sys
from unittest.mock import MagicMock
for mod in ("imageio", "lpips", "cv2", "skimage", "skimage.metrics", "open3d", "matplotlib", "matplotlib.pyplot", "matplotlib.cm", "h5py",
            "configargparse", "trimesh", "mcubes", "plyfile"):
    sys.modules.setdefault(mod, MagicMock())              # third-party packages of the reference's drivers that this image lacks
sys.path.insert(0, %(root)r); sys.path.insert(0, %(ref)r)
import dm_nerf_amd.dropin as D
D.install()
import networks.render, networks.helpers, networks.dm_nerf, networks.penalizer, networks.evaluator, config
import networks.tester, networks.manipulator                # reference modules that copy the names at import (tester.py:11-13)
import dm_nerf_amd.networks.render as R, dm_nerf_amd.networks.helpers as H, dm_nerf_amd.networks.dm_nerf as M
import dm_nerf_amd.networks.manipulator as MA, dm_nerf_amd.config as C, dm_nerf_amd.networks.evaluator as E
assert networks.render.dm_nerf is R.dm_nerf and networks.render.render_train is R.render_train
assert networks.tester.dm_nerf is R.dm_nerf and networks.tester.get_rays_k is H.get_rays_k and networks.tester.z_val_sample is H.z_val_sample
assert networks.helpers.sample_pdf is H.sample_pdf and networks.helpers.get_select_crop is H.get_select_crop
assert networks.manipulator.manipulator is MA.manipulator and networks.manipulator.exchanger is MA.exchanger
assert networks.manipulator.sample_pdf is H.sample_pdf
assert networks.dm_nerf.DM_NeRF is M.DM_NeRF and config.DM_NeRF is M.DM_NeRF and config.create_nerf is C.create_nerf
assert networks.evaluator.ins_criterion is E.ins_criterion
# not on the hot path: still the reference's own code
assert networks.evaluator.calculate_ap.__module__ == "networks.evaluator" and networks.helpers.get_rays.__module__ == "networks.helpers"
assert config.initial.__module__ == "config" and networks.tester.render_test.__module__ == "networks.tester"
# this package's own modules are never patched
assert not hasattr(C, "__dm_nerf_amd_patched__")
print("DROPIN_OK", sorted(networks.helpers.__dm_nerf_amd_patched__))
'''


def test_reference_modules_are_rebound_without_edits(tmp_path):
    ref = REF or _stand_in_checkout(str(tmp_path))
    p = subprocess.run([sys.executable, "-c", PROBE % {"root": ROOT, "ref": ref}], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DROPIN_OK" in p.stdout, p.stderr[-2000:]


def test_patch_table_names_exist_in_this_package():
    import dm_nerf_amd.dropin as D
    for mod, names in D.PATCHES.items():
        for name, ref in names.items():
            assert callable(D._resolve(ref)) or isinstance(D._resolve(ref), type), (mod, name)
