"""GPU tests (-m gpu) of the kernel-layout copies of the weights behind ``DM_NeRF``'s accessors (``flat``, the seven blobs,
``blob_f16_density``): every copy bit for bit what it was when ``tests/golden/packed_layouts.json`` was recorded (SHA-256 of its
bytes; the packers are gathers and fixed-order conversions, so the digests are a property of the device type), the refresh rules
of the cache, and the refusals.  Only the public accessors are used.

``python tests/test_gpu_packed_layouts.py [out.json]`` records the digests (default: the golden file)."""
import copy
import hashlib
import json
import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pytest
import torch

import _gpu
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_layouts.json")
BLOBS = ("blob", "blob_t", "blob_fused", "blob_split", "blob_f16", "blob_t_split", "blob_t_f16")
OPT_IN = BLOBS[2:] + ("blob_f16_density",)             # what install_packed does not install
ACCESSORS = ("flat",) + BLOBS + ("blob_f16_density",)
# 1: C = 2, one 32-logit block; 13: the benchmark's; 93: three blocks, packed as four; 120: four blocks
INS_NUMS = (1, 13, 93, 120)
IN_EVERY_LAYOUT = "mlps.3.weight"                      # (mlps.0 has no W^T: the first layer's input gets no data gradient)


def make_model(ins_num, seed=5):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return _gpu.model_from(O.make_weights(seed, ins_num, gain=1.7, sigma_bias=0.3), ins_num)


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digests(m):
    return {name: digest(getattr(m, name)()) for name in ACCESSORS}


def get_all(m, names=ACCESSORS):
    return {name: getattr(m, name)() for name in names}


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("ins_num", INS_NUMS)
def test_every_layout_is_bit_identical_to_the_recorded_one(want, ins_num):
    got = digests(make_model(ins_num))
    assert set(want[str(ins_num)]) == set(ACCESSORS)
    assert got == want[str(ins_num)], [k for k in ACCESSORS if got[k] != want[str(ins_num)][k]]


def test_same_object_until_a_parameter_changes():
    m = make_model(13)
    first = get_all(m)
    for name, t in get_all(m).items():
        assert t is first[name], name


def test_version_bump_gives_a_new_tensor_and_leaves_the_old_one_alone():
    m = make_model(13)
    old = get_all(m)
    kept = {name: t.clone() for name, t in old.items()}
    with torch.no_grad():
        dict(m.named_parameters())[IN_EVERY_LAYOUT].add_(0)
    for name, t in get_all(m).items():
        assert t is not old[name] and t.data_ptr() != old[name].data_ptr(), name
        assert torch.equal(old[name], kept[name]), name
        assert torch.equal(t, kept[name]), name                     # (+ 0: the same weights, packed again)


def test_data_update_is_seen_after_invalidate_blobs_only():
    m = make_model(13)
    old = get_all(m)
    dict(m.named_parameters())[IN_EVERY_LAYOUT].data.mul_(2)
    for name, t in get_all(m).items():
        assert t is old[name], name
    m.invalidate_blobs()
    for name, t in get_all(m).items():
        assert t is not old[name] and not torch.equal(t, old[name]), name


def test_install_packed_installs_three_and_drops_the_rest():
    m = make_model(13)
    old = get_all(m)
    f, b, bt = old["flat"].clone(), old["blob"].clone(), old["blob_t"].clone()
    m.install_packed(f, b, bt)
    assert m.flat() is f and m.blob() is b and m.blob_t() is bt
    for name, t in get_all(m, OPT_IN).items():
        assert t is not old[name] and t.data_ptr() != old[name].data_ptr(), name
        assert torch.equal(t, old[name]), name
    assert m.flat() is f and m.blob() is b and m.blob_t() is bt      # packing the others did not replace them


def test_deepcopy_renders_the_same():
    from dm_nerf_amd.networks import render as R
    m = make_model(13)
    get_all(m)                                                      # a warm cache travels with the copy and must not be used by it
    m2 = copy.deepcopy(m)
    g = torch.Generator().manual_seed(2)
    rays_o, rays_d = torch.randn(24, 3, generator=g).cuda(), torch.nn.functional.normalize(torch.randn(24, 3, generator=g), dim=-1).cuda()
    z = torch.linspace(4.0, 15.0, 16).expand(24, 16).contiguous().cuda()
    with torch.no_grad():
        a, b = R.run_network(m, rays_o, rays_d, z), R.run_network(m2, rays_o, rays_d, z)
    assert m2.blob() is not m.blob() and torch.equal(a, b)


def test_module_without_the_cache_attribute_packs_on_first_use(want):
    m = make_model(13)
    m.__dict__.pop("_packed", None)                                 # a module pickled whole before the cache was one dict
    assert digests(m) == want["13"]


def test_other_shapes_are_refused_by_every_blob_accessor_but_flat():
    from dm_nerf_amd.networks import dm_nerf as M
    m = M.DM_NeRF(D=4, W=64, input_ch_pts=63, input_ch_views=27, skips=[2], ins_num=13).cuda()
    for name in BLOBS + ("blob_f16_density",):
        with pytest.raises(NotImplementedError, match=r"the packed weight blobs exist for the fused kernels' shape only \(D=8, W=256"):
            getattr(m, name)()
    flat = m.flat()
    assert flat.dtype == torch.float32 and flat.numel() == sum(p.numel() for p in m.parameters())
    assert torch.equal(flat, torch.cat([p.detach().reshape(-1) for p in m.parameters()]))


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {str(n): digests(make_model(n)) for n in INS_NUMS}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in rec.values())} digests -> {out}")
