"""CPU tests of the touch-chart bake (no GPU): ``utility.data_making.touch_charts_batch`` / ``save_touch_info`` with a CPU ``Encoder``
and a ``RecordedSampler`` on seeded records (the recipe of ``env_util``) or on a synthetic tree (``touch_util``); ``ops.touch_chart_head``
on CPU tensors against the lines of ``Encoder.forward`` and ``scoring.touch_slots`` it replaces; the encoder's new entry points."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import env_util as eu
import touch_util as tu
from chart_head_util import parent_predict_verts, write_touch_checkpoint
from a3vt_amd import mesh, ops
from a3vt_amd.pterotactyl.policies import recorded, rendered, scoring
from a3vt_amd.pterotactyl.reconstruction.touch import model
from a3vt_amd.pterotactyl.utility import data_loaders, data_making

A = 3
SEED = 4100


@pytest.fixture(scope="module")
def template():
    return torch.from_numpy(mesh.load_asset("touch_chart")[0].astype(np.float32))


@pytest.fixture(scope="module")
def encoder():
    torch.manual_seed(0)
    net = model.Encoder()
    tu.seed_batchnorm(net)
    return net.eval()


class CheapEncoder(model.Encoder):
    """The encoder's ``fc`` behind 512 pixels of the image: for the tests that are about files, not about the network."""

    def predict_features_nhwc(self, signal):
        return signal.reshape(signal.shape[0], -1)[:, 1000:1000 + 512 * 7:7].contiguous()


@pytest.fixture(scope="module")
def cheap():
    torch.manual_seed(1)
    return CheapEncoder().eval()


@pytest.fixture(scope="module")
def table():
    return eu.status_table(SEED, A)                        # (2, A, 4) codes: all three occur (asserted below)


@pytest.fixture(scope="module")
def sampler(table):
    return recorded.RecordedSampler(eu.records(eu.OBJECTS, A, table, SEED))


def tree(root, objects, without_grasps=()):
    for obj in objects:
        os.makedirs(os.path.join(root, "object_info"), exist_ok=True)
        np.save(os.path.join(root, "object_info", f"{obj}_verts.npy"), np.zeros((3, 3), np.float32))
        np.save(os.path.join(root, "object_info", f"{obj}_faces.npy"), np.zeros((1, 3), np.int64))
        if obj not in without_grasps:
            os.makedirs(os.path.join(root, "grasp_info", obj), exist_ok=True)
    return str(root)


@pytest.fixture(scope="module")
def bake(tmp_path_factory, encoder, sampler):
    """One bake of the two objects (and one without grasps) with the real CPU encoder: (root, counts)."""
    root = tree(tmp_path_factory.mktemp("bake"), eu.OBJECTS + ("lonely",), without_grasps=("lonely",))
    counts = data_making.save_touch_info(root, encoder=encoder, sampler=sampler, batch=8, num_actions=A)
    return root, counts


def load(root, obj):
    return np.load(os.path.join(root, "touch_charts", obj, "touch_charts.npy"))


def test_files_counts_and_mask_columns(bake, table):
    root, counts = bake
    assert sorted(np.unique(table)) == [0, 1, 2]                                            # a view of each code is in the table
    assert counts == dict(written=2, skipped_existing=0, skipped_no_grasps=1, views=2 * A * 4, touch=int((table == 2).sum()),
                          no_touch=int((table == 1).sum()), no_intersection=int((table == 0).sum()))
    assert not os.path.exists(os.path.join(root, "touch_charts", "lonely"))
    for e, obj in enumerate(eu.OBJECTS):
        assert os.listdir(os.path.join(root, "touch_charts", obj)) == ["touch_charts.npy"]  # no temporary file is left behind
        charts = load(root, obj)
        assert charts.shape == (A, 4, 25, 4) and charts.dtype == np.float32
        assert np.array_equal(charts[..., 3], np.broadcast_to(table[e][:, :, None].astype(np.float32), (A, 4, 25)))
        assert not charts[table[e] == 0].any() and np.isfinite(charts).all()


def test_entries_are_touch_slots_of_the_samplers_answers(bake, sampler, encoder, template):
    """(e, a, f) order and the arithmetic: entry [a, f] of object e's file is ``touch_slots`` on finger f of element e of
    ``sampler.sample([a, a])`` with the image truncated through uint8 — all views in one ``touch_slots`` call, as the bake makes
    one encoder call, so that the comparison is bit for bit."""
    root, _ = bake
    sampler.load_objects([f"/data/object_info/{o}" for o in eu.OBJECTS])
    answers = [sampler.sample([a, a]) for a in range(A)]
    stack = lambda key: torch.stack([r[key] for r in answers], dim=1)                        # noqa: E731  (E, A, 4, ...)
    touch = (stack("touch_signal").to(torch.uint8).float().movedim(-1, -3) / 255.0).contiguous()
    status = [[answers[a]["touch_status"][e] for a in range(A)] for e in range(2)]
    charts, masks = scoring.touch_slots(encoder, touch, {"rot": stack("finger_transform_rot_M"), "pos": stack("finger_transfrom_pos")},
                                        status, template)
    want = torch.cat((charts, masks), dim=-1).numpy()
    for e, obj in enumerate(eu.OBJECTS):
        got = load(root, obj)
        for a in range(A):
            for f in range(4):
                assert np.array_equal(got[a, f].view(np.uint32), want[e, a, f].view(np.uint32)), (obj, a, f)
    code1 = np.argwhere(np.asarray(status, dtype=object) == "no_touch")[0]
    e, a, f = code1
    assert np.array_equal(load(root, eu.OBJECTS[e])[a, f, :, :3], np.tile(answers[a]["finger_transfrom_pos"][e, f].numpy(), (25, 1)))


def test_truncation_shows_and_chunks_are_the_same_views(bake, sampler, encoder, template, table):
    root, _ = bake
    names = [os.path.join(root, "object_info", o) for o in eu.OBJECTS]
    plain = data_making.touch_charts_batch(sampler, encoder, template, names, num_actions=A, truncate=False, encode_chunk=5)
    assert plain.shape == (2, A, 4, 25, 4) and plain.dtype == torch.float32 and plain.device.type == "cpu"
    baked = np.stack([load(root, o) for o in eu.OBJECTS])
    touched = table == 2
    assert (np.abs(plain.numpy() - baked)[touched].reshape(touched.sum(), -1).max(axis=1) > 0).all()   # every fractional image shows
    assert np.array_equal(plain.numpy()[~touched], baked[~touched])                                    # no image is in the others


def test_the_head_knob_and_the_action_count(sampler, cheap, template):
    names = [f"/data/object_info/{o}" for o in eu.OBJECTS]
    on = data_making.touch_charts_batch(sampler, cheap, template, names, num_actions=A, fused_head=True)
    off = data_making.touch_charts_batch(sampler, cheap, template, names, num_actions=A, fused_head=False)
    default = data_making.touch_charts_batch(sampler, cheap, template, names, num_actions=A)
    assert torch.equal(on, off) and torch.equal(on, default)                 # on the CPU one torch formulation serves both
    assert torch.equal(data_making.touch_charts_batch(sampler, cheap, template, names, num_actions=A, encode_chunk=5), on)
    two = data_making.touch_charts_batch(sampler, cheap, template, names[::-1], num_actions=2, encode_chunk=3)
    assert two.shape == (2, 2, 4, 25, 4) and torch.equal(two[:, :, :, :, 3], on.flip(0)[:, :2, :, :, 3])


def test_a_recorded_tree_fifty_actions_and_the_loader(tmp_path, cheap):
    """``sampler="recorded"`` on a dataset tree, the default 50 actions, and ``mesh_loader_vision.get_touch_info`` reading the file
    back in both ``finger`` modes; existing files are skipped, ``overwrite`` writes them again."""
    root = str(tmp_path)
    ids = tu.write_mini_touch_dataset(root)                                   # grasps 0 and 7, fingers 0 and 2; "3" has no grasps
    tree(root, ids, without_grasps=ids)
    for obj in ids:
        for grasp in ("0", "7"):
            d = os.path.join(root, "grasp_info", obj, grasp)
            if os.path.isdir(d):                                              # finger 1: a frame and no image is "no_touch"
                np.save(os.path.join(d, "1_ref_frame.npy"), {"rot": np.eye(3), "pos": np.array([0.1, 0.2, 0.3]) * (1 + int(obj))})
    counts = data_making.save_touch_info(root, encoder=cheap, sampler="recorded", batch=2)
    assert counts == dict(written=4, skipped_existing=0, skipped_no_grasps=1, views=4 * 50 * 4, touch=16, no_touch=8,
                          no_intersection=4 * 200 - 24)
    charts = load(root, "2")
    assert charts.shape == (50, 4, 25, 4) and charts.dtype == np.float32
    assert sorted(np.flatnonzero(charts[:, :, 0, 3].any(axis=1))) == [0, 7]
    assert charts[7, :, 0, 3].tolist() == [2.0, 1.0, 2.0, 0.0]
    loader = data_loaders.mesh_loader_vision.__new__(data_loaders.mesh_loader_vision)
    loader.touch_dir = os.path.join(root, "touch_charts")
    loader.args = SimpleNamespace(use_touch=True, num_grasps=5, finger=False)
    got = loader.get_touch_info("2", [7, 3, 0])
    assert got.shape == (5, 4, 25, 4) and torch.equal(got[:3], torch.from_numpy(charts[[7, 3, 0]])) and not got[3:].any()
    loader.args.finger = True
    got = loader.get_touch_info("2", [7, 0])
    assert got.shape == (5, 25, 4) and torch.equal(got[:2], torch.from_numpy(charts[[7, 0], 1])) and not got[2:].any()
    assert torch.equal(got[0], torch.tensor([0.3, 0.6, 0.9, 1.0]).expand(25, 4))
    before = os.stat(os.path.join(root, "touch_charts", "2", "touch_charts.npy")).st_mtime_ns
    again = data_making.save_touch_info(root, encoder=cheap, sampler="recorded", batch=2)
    assert again == dict(written=0, skipped_existing=4, skipped_no_grasps=1, views=0, touch=0, no_touch=0, no_intersection=0)
    assert os.stat(os.path.join(root, "touch_charts", "2", "touch_charts.npy")).st_mtime_ns == before
    os.remove(os.path.join(root, "touch_charts", "0", "touch_charts.npy"))
    third = data_making.save_touch_info(root, encoder=cheap, sampler="recorded", batch=3, overwrite=True)
    assert third == counts and np.array_equal(load(root, "2"), charts)
    assert all(os.listdir(os.path.join(root, "touch_charts", o)) == ["touch_charts.npy"] for o in ("0", "1", "2", "4"))


def test_the_encoder_is_loaded_from_a_checkpoint(tmp_path, encoder, monkeypatch):
    """``encoder=None``: the model of ``touch_location``, or without one the pretrained model by the environment's rule
    (``<pretrained root>/reconstruction/touch/best``) — the same files as with the encoder passed in."""
    root = str(tmp_path / "data")
    ids = tu.write_mini_touch_dataset(root)
    tree(root, ids, without_grasps=ids)
    path = lambda obj: os.path.join(root, "touch_charts", obj, "touch_charts.npy")             # noqa: E731
    want_counts = data_making.save_touch_info(root, encoder=encoder, sampler="recorded", num_actions=1)
    want = {obj: np.load(path(obj)) for obj in ("0", "1", "2", "4")}
    assert want_counts["written"] == 4 and want_counts["touch"] == 8 and want["2"][0, :, 0, 3].tolist() == [2.0, 0.0, 2.0, 0.0]
    location = write_touch_checkpoint(str(tmp_path / "mine"), encoder) + "/"
    monkeypatch.delenv("PTEROTACTYL_PRETRAINED", raising=False)
    with pytest.raises(FileNotFoundError, match="PTEROTACTYL_PRETRAINED"):
        data_making.save_touch_info(root, sampler="recorded", num_actions=1, overwrite=True, device="cpu")
    write_touch_checkpoint(str(tmp_path / "pretrained" / "reconstruction" / "touch" / "best"), encoder)
    for kw in (dict(touch_location=location), dict()):
        for obj in want:
            os.remove(path(obj))
        if not kw:
            monkeypatch.setenv("PTEROTACTYL_PRETRAINED", str(tmp_path / "pretrained"))
        assert data_making.save_touch_info(root, sampler="recorded", num_actions=1, device="cpu", **kw) == want_counts
        for obj, charts in want.items():
            assert np.array_equal(np.load(path(obj)).view(np.uint32), charts.view(np.uint32)), (kw, obj)


def test_refusals(tmp_path, cheap):
    root = tree(tmp_path, ("a",))
    with pytest.raises(ValueError, match=f"{400 * 50 * 4} views.*{rendered.MAX_VIEWS}"):
        data_making.save_touch_info(root, encoder=cheap, sampler="recorded", batch=400)
    with pytest.raises(ValueError, match="sampler"):
        data_making.save_touch_info(root, encoder=cheap, sampler=object())
    assert not os.path.exists(os.path.join(root, "touch_charts"))


def head_inputs(n, seed, fc):
    g = torch.Generator().manual_seed(seed)
    features = torch.randn(n, 512, generator=g).abs()
    rot = torch.randn(n, 3, 3, generator=g)                                   # no symmetry: a transposed product would show
    pos = torch.randn(n, 3, generator=g)
    code = torch.arange(n, dtype=torch.int32) % 3
    return features, fc, rot, pos, code


def test_the_cpu_head_is_the_lines_it_replaces(encoder, template):
    features, fc, rot, pos, code = head_inputs(7, 5, encoder.fc)
    code[6] = 5                                                                # no code of the environment's: zeros and mask 0
    features[1, 3] = float("nan")                                              # a "no_touch" row
    features[3, 0] = float("nan")                                              # a "no_intersection" row
    rows, charts, masks = ops.touch_chart_head(features, fc, template, rot, pos, code, want_slots=True)
    with torch.no_grad():                                                      # Encoder.forward + touch_slots, as they stand
        verts = template.view(1, -1, 3).repeat(7, 1, 1)
        pred = encoder.transform_verts(verts + fc(features).view(-1, 25, 3), {"rot": rot, "pos": pos})
        c = torch.where(code > 2, torch.zeros_like(code), code).float().view(7, 1, 1)
        want = torch.where(c == 2, pred, torch.where(c == 1, pos.view(7, 1, 3).expand_as(pred), torch.zeros_like(pred)))
    assert rows.shape == (7, 25, 4) and charts.shape == (7, 25, 3) and masks.shape == (7, 25, 1)
    assert torch.equal(charts.view(torch.int32), want.view(torch.int32)) and torch.equal(masks, c.expand(7, 25, 1))
    assert torch.equal(rows[..., :3], charts) and torch.equal(rows[..., 3:], masks) and torch.isfinite(rows).all()
    assert torch.equal(ops.touch_chart_head(features, fc, template, rot, pos, code.long()), rows)
    assert not rows.requires_grad
    features[2, 9] = float("nan")                                              # a "touch" row: poisoned, alone
    poisoned = ops.touch_chart_head(features, fc, template, rot, pos, code)
    assert torch.isnan(poisoned[2, :, :3]).all() and torch.equal(poisoned[[0, 1, 3, 4, 5, 6]], rows[[0, 1, 3, 4, 5, 6]])
    for bad, match in (((features[:, :500], fc, template, rot, pos, code), "features"), ((features, fc, template[:24], rot, pos, code), "template"),
                       ((features, fc, template, rot[:6], pos, code), "views"), ((features, fc, template, rot, pos, code.float()), "code"),
                       ((features, fc, template, rot, pos, code[:6]), "code"), ((features.double(), fc, template, rot, pos, code), "features"),
                       ((features, torch.nn.Sequential(fc[1], fc[0], fc[2]), template, rot, pos, code), "Linear")):
        with pytest.raises(ValueError, match=match):
            ops.touch_chart_head(*bad)


def test_the_encoders_entry_points(encoder):
    x = tu.images(2, 9).float() / 255.0
    with torch.no_grad():
        features = encoder.predict_features(x)
        assert features.shape == (2, 512)
        assert torch.equal(encoder.predict_verts(x), parent_predict_verts(encoder, x))     # the bits it had before the split
        assert torch.equal(encoder.predict_verts(x), encoder.fc(features))
        assert torch.equal(encoder.predict_features_nhwc(x.movedim(-3, -1).contiguous()), features)


def test_the_knob_of_touch_slots(encoder, template):
    """Off by default; on the CPU the knob changes nothing (the torch lines run)."""
    assert scoring.FUSED_HEAD_DEFAULT is False
    net = encoder
    touch = tu.images(3, 4).float() / 255.0
    rot, pos = tu.frames(3, 5)
    status = ["touch", "no_touch", "no_intersection"]
    plain = scoring.touch_slots(net, touch, {"rot": rot, "pos": pos}, status, template)
    for knob in (None, False, True):
        got = scoring.touch_slots(net, touch, {"rot": rot, "pos": pos}, status, template, fused_head=knob)
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
