"""GPU tests of the touch-chart bake: the encoder's channels-last entry, ``scoring.touch_slots`` with the one-launch head, and
``utility.data_making.save_touch_info`` through the real renderer on two icospheres.

The cap of the comparisons between the head on and off is the one of ``test_gpu_chart_head.py``: both forms take the SAME fp32
features (the convolutions are the same calls), so both are compared with the fp64 head (``chart_head_util.rows64``) of those
features, and the one-launch head's largest error may be 4 x the torch tail's: two equally valid fp32 evaluations."""
import os

import numpy as np
import pytest
import torch

import touch_util as tu
from chart_head_util import (BAKE_OBJECTS as OBJECTS, bake_scene, parent_predict_verts, rows64, seeded_encoder, write_bake_tree,
                             write_touch_checkpoint)

pytestmark = pytest.mark.gpu

A = 3


@pytest.fixture(scope="module")
def net(cuda):
    return seeded_encoder(cuda, fused_stem=True)


@pytest.fixture(scope="module")
def template(cuda):
    from a3vt_amd import mesh
    return torch.from_numpy(mesh.load_asset("touch_chart")[0]).float().to(cuda)


def held(on, off, want, what):
    """The 4 x rule on (n, 25, 4) rows; the mask columns and every row without a rounded sum must agree exactly."""
    on, off = on.double().cpu().reshape(want.shape), off.double().cpu().reshape(want.shape)
    e_on, e_off = (on - want).abs().max().item(), (off - want).abs().max().item()
    print(f"{what}: head on {e_on:.3e}, head off {e_off:.3e}: {e_on / e_off:.2f} x")
    assert e_off > 0 and e_on <= 4 * e_off, f"{what}: {e_on:.3e} > 4 x {e_off:.3e}"
    assert torch.equal(on[..., 3], off[..., 3]) and torch.equal(on[..., 3], want[..., 3])
    plain = want[:, 0, 3] != 2
    assert torch.equal(on[plain], off[plain]) and torch.equal(on[plain], want[plain])


@pytest.mark.parametrize("n", [1, 5])
def test_the_channels_last_entry_is_the_same_bits(net, cuda, n):
    from a3vt_amd import ops
    x = (tu.images(n, 30 + n).float() / 255.0).to(cuda)                        # (n, 3, 121, 121)
    last = x.movedim(-3, -1).contiguous()                                      # as the samplers deliver them
    with torch.no_grad():
        assert net.takes_fused_stem(last)
        before = ops.STATS.get("conv5f", 0)
        got = net.predict_features_nhwc(last)
        assert ops.STATS.get("conv5f", 0) == before + 9                        # the fused stem ran
        want = net.predict_features(last.movedim(-1, -3))
        assert got.shape == (n, 512) and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(net.predict_verts(x), parent_predict_verts(net, x))  # the split left predict_verts' bits as they were
        plain = seeded_encoder(cuda, fused_stem=False)                         # without the fused stem: permuted once, torch's stem
        assert torch.equal(plain.predict_features_nhwc(last), plain.predict_features(x))
        assert torch.equal(plain.predict_verts(x), parent_predict_verts(plain, x))


def test_touch_slots_with_the_head_on_and_off(net, template, cuda):
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies import scoring
    E, F = 2, 4
    touch = (tu.images(E * F, 41).float() / 255.0).to(cuda).view(E, F, 3, 121, 121)
    rot, pos = tu.frames(E * F, 42)
    ref = {"rot": rot.view(E, F, 3, 3), "pos": pos.view(E, F, 3)}              # on the host, as a sampler leaves them
    status = [["touch", "no_touch", "touch", "no_intersection"], ["touch", "touch", "nothing", "touch"]]
    code = torch.tensor([2, 1, 2, 0, 2, 2, 0, 2])
    ops.chart_head_launches(reset=True)
    off = scoring.touch_slots(net, touch, ref, status, template, fused_head=False)
    default = scoring.touch_slots(net, touch, ref, status, template)
    assert ops.chart_head_launches() == {"calls": 0}
    assert torch.equal(default[0], off[0]) and torch.equal(default[1], off[1])  # None is off: today's path, bit for bit
    on = scoring.touch_slots(net, touch, ref, status, template, fused_head=True)
    assert ops.chart_head_launches() == {"calls": 1}
    for got in (on, off):
        assert got[0].shape == (E, F, 25, 3) and got[1].shape == (E, F, 25, 1) and got[0].is_contiguous() and got[1].is_contiguous()
    with torch.no_grad():
        features = net.predict_features(touch.view(E * F, 3, 121, 121))
    want = rows64(features, net.fc, template, rot, pos, code)
    held(torch.cat(on, dim=-1), torch.cat(off, dim=-1), want, "touch_slots, 8 views")


def test_a_two_object_bake_through_the_renderer(net, template, cuda, tmp_path, monkeypatch):
    from a3vt_amd.pterotactyl.policies import rendered
    from a3vt_amd.pterotactyl.utility import data_making
    geometry, frames = bake_scene()
    root = write_bake_tree(str(tmp_path / "data"), geometry, frames)
    # the call a user makes: the tree rendered (sampler="rendered"), the pretrained model found by the environment's rule
    write_touch_checkpoint(str(tmp_path / "pretrained" / "reconstruction" / "touch" / "best"), net)
    monkeypatch.setenv("PTEROTACTYL_PRETRAINED", str(tmp_path / "pretrained"))
    counts = data_making.save_touch_info(root, num_actions=A)
    sampler = rendered.RenderedSampler(frames, geometry, to_host=False)        # the same scene from mappings, for the comparisons
    baked = torch.from_numpy(np.stack([np.load(os.path.join(root, "touch_charts", obj, "touch_charts.npy")) for obj in OBJECTS]))
    assert baked.shape == (2, A, 4, 25, 4) and baked.dtype == torch.float32
    names = [os.path.join(root, "object_info", obj) for obj in OBJECTS]
    on = data_making.touch_charts_batch(sampler, net, template, names, num_actions=A, fused_head=True)
    off = data_making.touch_charts_batch(sampler, net, template, names, num_actions=A, fused_head=False)
    assert on.is_cuda and torch.equal((on if data_making.BAKE_FUSED_HEAD else off).cpu(), baked)   # the files hold the default form
    table = sampler.sample_table(A, to_host=False)                             # the same views once more, for the fp64 head
    code = table["touch_code"].reshape(-1)
    assert sorted(code.unique().tolist()) == [0, 1, 2]
    assert counts == dict(written=2, skipped_existing=0, skipped_no_grasps=0, views=2 * A * 4, touch=int((code == 2).sum()),
                          no_touch=int((code == 1).sum()), no_intersection=int((code == 0).sum()))
    with torch.no_grad():
        images = table["touch_signal"].reshape(-1, 121, 121, 3).to(torch.uint8).float() / 255.0
        features = net.predict_features_nhwc(images)
    want = rows64(features, net.fc, template, table["finger_transform_rot_M"].reshape(-1, 3, 3),
                  table["finger_transfrom_pos"].reshape(-1, 3), code)
    held(on.reshape(-1, 25, 4), off.reshape(-1, 25, 4), want, f"bake of two icospheres, {code.numel()} views")
    assert torch.equal(on[..., 3].cpu(), table["touch_code"].cpu().float()[..., None].expand(2, A, 4, 25))
