"""CPU tests of the touch chart predictor: module tree, the torch path against the fixture, the BatchNorm fold, the dataset
class on a miniature dataset, the synthetic batch, and the argument checks of the four ``a3vt_conv5f_*`` entry points."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_util as gu
import touch_util as tu


@pytest.fixture(scope="module")
def z():
    return gu.load(tu.FIXTURE)


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def test_state_dict_keys_and_shapes(z):
    net = tu.load_encoder(z)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == json.loads(str(z["keys"]))
    for name in ("predict_verts", "transform_verts", "forward"):
        assert callable(getattr(net, name))


def test_cpu_forward_against_fixture(z):
    net = tu.load_encoder(z, fused_stem=True)            # the knob is inert on the CPU
    x = torch.from_numpy(z["img"]).float() / 255.0
    ref = {"rot": torch.from_numpy(z["rot"]), "pos": torch.from_numpy(z["pos"])}
    verts = torch.from_numpy(z["template"]).unsqueeze(0).repeat(2, 1, 1)
    with torch.no_grad():
        stem, out = net.stem(x), net(x, ref, verts)
    d_stem = (stem.double() - torch.from_numpy(z["eval64:stem"])).abs().max().item()
    d_out = (out.double() - torch.from_numpy(z["eval64:out"])).abs().max().item()
    assert d_stem <= 4 * float(z["e_stem"]) and d_out <= 4 * float(z["e_out"]), (d_stem, d_out)


def test_transform_verts_leaves_its_inputs_alone(z):
    net = tu.load_encoder(z)
    g = torch.Generator().manual_seed(0)
    verts = torch.randn(3, 25, 3, generator=g)
    rot, pos = tu.frames(3, 1)
    kept = verts.clone(), rot.clone(), pos.clone()
    out = net.transform_verts(verts, {"rot": rot, "pos": pos})
    assert torch.equal(verts, kept[0]) and torch.equal(rot, kept[1]) and torch.equal(pos, kept[2])
    want = torch.einsum("bij,bvj->bvi", rot.double(), verts.double()) + pos.double()[:, None]
    assert (out.double() - want).abs().max().item() < 1e-6
    template = torch.from_numpy(z["template"])
    net(torch.zeros(1, 3, 121, 121), {"rot": rot[:1], "pos": pos[:1]}, template[None])
    assert torch.equal(template, torch.from_numpy(z["template"]))


def test_batchnorm_fold_against_torch_fp64():
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(3, 16, 5, padding=2, stride=2).double()
    bn = torch.nn.BatchNorm2d(16).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(16, generator=g, dtype=torch.float64))
        bn.bias.copy_(torch.randn(16, generator=g, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(16, generator=g, dtype=torch.float64))
        bn.running_var.copy_(0.1 + torch.rand(16, generator=g, dtype=torch.float64))
    bn.eval()
    x = torch.randn(2, 3, 13, 11, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = bn(conv(x))
        scale, shift = ops.bn_fold(conv.bias, bn)
        got = torch.nn.functional.conv2d(x, conv.weight, None, stride=2, padding=2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        assert (got - want).abs().max().item() <= 1e-13 * want.abs().max().item()
        scale0, shift0 = ops.bn_fold(None, bn)
        assert torch.equal(scale0, scale) and (shift0 + scale * conv.bias - shift).abs().max().item() < 1e-13


def test_mesh_loader_touch_on_a_miniature_dataset(tmp_path):
    from a3vt_amd.pterotactyl.utility import data_loaders
    root = str(tmp_path)
    tu.write_mini_touch_dataset(root, short_points=37)
    args = SimpleNamespace(data_root=root, limit_data=False, num_samples=100)
    np.random.seed(0)
    torch.manual_seed(0)
    train = data_loaders.mesh_loader_touch(args, set_type="recon_train")
    valid = data_loaders.mesh_loader_touch(args, set_type="valid")
    assert len(train) == 8 and len(valid) == 4                        # objects x 2 grasps x 2 fingers; "3" has no grasps, "4" is in no set
    assert sorted(map(tuple, valid.object_names)) == [("2", "0", "0"), ("2", "0", "2"), ("2", "7", "0"), ("2", "7", "2")]
    items = [valid[i] for i in range(len(valid))]
    batch = valid.collate(items)
    assert batch["names"] == [it["names"] for it in items] and len(batch["names"][0]) == 3
    assert tuple(batch["samples"].shape) == (4, 100, 3) and batch["samples"].dtype == torch.float32
    assert tuple(batch["sim_touch"].shape) == (4, 3, 121, 121) and batch["sim_touch"].dtype == torch.float32
    assert 0.0 <= batch["sim_touch"].min().item() and batch["sim_touch"].max().item() <= 1.0 and batch["sim_touch"].max().item() > 0.9
    assert set(batch["ref"]) == {"rot", "pos"} and tuple(batch["ref"]["rot"].shape) == (4, 3, 3) and tuple(batch["ref"]["pos"].shape) == (4, 3)
    for i, (obj, grasp, finger) in enumerate(batch["names"]):
        d = tmp_path / "grasp_info" / obj / grasp
        touch = np.load(d / f"{finger}_touch.npy")
        assert np.array_equal(batch["sim_touch"][i].numpy(), (touch.transpose(2, 0, 1) / 255.0).astype(np.float32))
        frame = np.load(d / f"{finger}_ref_frame.npy", allow_pickle=True).item()
        assert np.allclose(batch["ref"]["rot"][i].numpy(), frame["rot"]) and np.allclose(batch["ref"]["pos"][i].numpy(), frame["pos"])
        points = np.load(d / f"{finger}_points.npy").astype(np.float32)
        rows = {tuple(r) for r in points.tolist()}
        got = batch["samples"][i].numpy()
        assert all(tuple(r) in rows for r in got.tolist())              # every sample is a row of the file
        if finger == "0":       # 37 rows < 100: repeated x 4 to 148, 100 drawn without replacement: no row more than 4 times
            assert points.shape[0] == 37
            _, counts = np.unique(got, axis=0, return_counts=True)
            assert counts.max() <= 4 and counts.sum() == 100 and len(counts) >= 25
        else:                   # long enough: a subset without repetition
            assert len(np.unique(got, axis=0)) == 100
    # the repetition itself: 37 -> 148 rows before the draw
    pts = 0.1 * np.arange(37 * 3, dtype=np.float64).reshape(37, 3)
    args.num_samples = 148
    out = valid.standerdize_point_size(pts.copy())
    _, counts = np.unique(out.numpy(), axis=0, return_counts=True)
    assert tuple(out.shape) == (148, 3) and (counts == 4).all() and len(counts) == 37


def test_synthetic_touch_batch():
    from a3vt_amd import synthetic
    b = synthetic.touch_batch(3, 64, seed=5)
    b2 = synthetic.touch_batch(3, 64, seed=5)
    assert tuple(b["sim_touch"].shape) == (3, 3, 121, 121) and 0.0 <= b["sim_touch"].min() and b["sim_touch"].max() <= 1.0
    assert tuple(b["samples"].shape) == (3, 64, 3) and len(b["names"]) == 3
    rot, pos = b["ref"]["rot"], b["ref"]["pos"]
    assert (rot @ rot.transpose(1, 2) - torch.eye(3)).abs().max().item() < 1e-5
    assert (torch.linalg.det(rot) - 1).abs().max().item() < 1e-5
    assert torch.equal(b["samples"], b2["samples"]) and torch.equal(b["sim_touch"], b2["sim_touch"])
    assert ((b["samples"] - pos[:, None]).norm(dim=-1) < 0.05).all()      # near the chart (1.7 cm wide) in the finger's frame


FAKE = ctypes.c_void_p(0x7F0000001000)       # a "device pointer": 16-byte aligned, never mapped on the host
FAKE_ODD = ctypes.c_void_p(0x7F0000001008)   # 8 mod 16
SHAPES = [(3, 16, 2), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 32, 2)]


def test_conv5f_supported_and_image_bytes(L):
    for cin in (1, 3, 4, 16, 32, 64):
        for cout in (3, 16, 32, 64):
            for stride in (1, 2, 3):
                assert L.a3vt_conv5f_supported(cin, cout, stride) == int((cin, cout, stride) in SHAPES)
    for cin, cout, _ in SHAPES:
        n = L.a3vt_conv5f_image_bytes(cin, cout)
        assert n >= cout * cin * 25 * 4 and n % 16 == 0          # at least the weights themselves
    for cin, cout in ((3, 32), (16, 3), (32, 16), (64, 64), (0, 16), (16, 0), (-3, 16)):
        assert L.a3vt_conv5f_image_bytes(cin, cout) == 0


def test_conv5f_argument_checks(L):
    """Every invalid call returns < 0 with a message before anything is launched (the pointers are never dereferenced)."""
    err = lambda: L.a3vt_last_error().decode()       # noqa: E731
    assert L.a3vt_conv5f_weight_image(None, 16, 16, FAKE, None) < 0 and "argument check" in err()
    assert L.a3vt_conv5f_weight_image(FAKE, 16, 16, None, None) < 0
    assert L.a3vt_conv5f_weight_image(FAKE, 16, 32, FAKE, None) < 0          # 32 -> 16 is not taken
    assert L.a3vt_conv5f_weight_image(FAKE, 16, 16, FAKE_ODD, None) < 0
    ok = dict(x=FAKE, batch=2, h=17, w=16, cin=16, cout=16, stride=1, pad=2, image=FAKE, scale=FAKE, shift=FAKE, relu=1, y=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return L.a3vt_conv5f_nhwc(a["x"], a["batch"], a["h"], a["w"], a["cin"], a["cout"], a["stride"], a["pad"], a["image"], a["scale"],
                                  a["shift"], a["relu"], a["y"], None)

    for bad in (dict(x=None), dict(image=None), dict(y=None), dict(batch=0), dict(batch=-1), dict(pad=-1), dict(pad=5),
                dict(stride=2), dict(cin=32, cout=16), dict(cin=3, cout=16, stride=1), dict(cin=8, cout=8),
                dict(h=0), dict(w=0), dict(h=4, pad=0), dict(w=2, pad=1),              # an empty output
                dict(relu=2), dict(y=FAKE_ODD), dict(x=FAKE_ODD), dict(image=FAKE_ODD), dict(batch=1 << 20, h=1 << 10, w=1 << 10)):
        assert call(**bad) < 0, bad
        assert "argument check" in err(), bad
