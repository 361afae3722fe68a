"""CPU tests of ``policies/rendered.py::RenderedSampler``'s host logic (no GPU): the class runs with ``render=`` set to the NumPy
emulation ``touch_render_ref.render``; keys, shapes and dtypes are compared with ``RecordedSampler``'s for the same records."""
import os

import numpy as np
import pytest
import torch

import env_util as eu
import touch_render_ref as tr
import touch_render_util as tu
from a3vt_amd import mesh
from a3vt_amd.pterotactyl.policies import environment, recorded, rendered

OBJECTS = ("ball", "pebble")
NAMES = [f"/data/object_info/{o}" for o in OBJECTS]


def sphere(level, radius, ahead):
    v, f = mesh.icosphere(level, radius)
    return (v.astype(np.float64) + tu.POS + ahead * tu.ROT[:, 0]).astype(np.float32), f.astype(np.int32)


def geometry():
    """Two meshes of different size ahead of the scenes' finger frame (few faces: the emulation casts every ray at every face)."""
    return {"ball": sphere(0, 0.004, 0.015), "pebble": sphere(1, 0.006, 0.02)}


def frame_table():
    """{(id, action): (pos, rot, present)}: action 0 all four fingers at the scenes' frame (finger 2 turned away: "no_touch"),
    action 1 with finger 3 missing, action 2 unknown for "pebble"."""
    pos, rot = np.tile(tu.POS, (4, 1)), np.tile(tu.ROT, (4, 1, 1))
    away = rot.copy()
    away[2] = tu.ROT @ tr.euler_xyz(np.array([0.0, 0.0, np.pi]))                  # finger 2 looks the other way
    some = np.array([True, True, True, False])
    table = {(o, 0): (pos, away, np.ones(4, bool)) for o in OBJECTS}
    table.update({(o, 1): (pos + 0.0005 * np.arange(4)[:, None], rot, some) for o in OBJECTS})
    table[("ball", 2)] = (pos, rot, np.ones(4, bool))
    return table


@pytest.fixture(scope="module")
def sampler():
    s = rendered.RenderedSampler(frame_table(), geometry(), render=tr.render)
    s.load_objects(NAMES)
    return s


@pytest.fixture(scope="module")
def first(sampler):
    return sampler.sample([0, 1], touch_point_cloud=True)


def test_the_result_has_the_recorded_samplers_keys_shapes_and_dtypes(first):
    frames = frame_table()
    records = {key: {"touch": np.zeros((4, 121, 121, 3), np.float32), "pos": p, "rot": r, "status": ["touch"] * 4}
               for key, (p, r, _) in frames.items()}
    rec = recorded.RecordedSampler(records)
    rec.load_objects(NAMES)
    want = rec.sample([0, 1], touch_point_cloud=True)
    assert set(want) <= set(first) and set(first) - set(want) == {"depths", "touch_point_cloud"}
    for key, value in want.items():
        if key == "touch_status":
            assert [len(row) for row in first[key]] == [len(row) for row in value] and all(isinstance(s, str) for row in first[key] for s in row)
        else:
            assert first[key].shape == value.shape and first[key].dtype == value.dtype and first[key].device == value.device, key
    assert first["depths"].shape == (2, 4, 121, 121) and first["depths"].dtype == torch.float32
    assert torch.equal(first["finger_transfrom_pos"][0], torch.as_tensor(frames[("ball", 0)][0], dtype=torch.float32))


def test_statuses_signals_and_clouds(first):
    assert first["touch_status"][0] == ["touch", "touch", "no_touch", "touch"]          # ball, action 0: finger 2 looks away
    assert first["touch_status"][1] == ["touch", "touch", "touch", "no_intersection"]   # pebble, action 1: finger 3 has no frame
    for key in ("touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"):
        assert not first[key][1, 3].any(), key                                           # ... and is all zeros
    assert not first["depths"][0, 2].any() and first["touch_signal"][0, 2].any()         # nothing seen, yet a (flat) gel image
    clouds = first["touch_point_cloud"]
    assert [len(row) for row in clouds] == [4, 4]
    for e in range(2):
        for f in range(4):
            cloud = clouds[e][f]
            assert isinstance(cloud, np.ndarray) and cloud.dtype == np.float32 and cloud.ndim == 2 and cloud.shape[1] == 3
            assert (len(cloud) > 0) == (first["touch_status"][e][f] == "touch")
    # the signals are the emulation's for that view
    pos32, rot32 = tu.frame32()                          # (the sampler hands the frames on as float32)
    d = tr.cast(*geometry()["ball"], pos32, rot32)[0].astype(np.float32)
    status, touch, points = tr.finish_one(d, pos32, rot32)
    assert np.array_equal(first["depths"][0, 0].numpy(), d)
    assert np.array_equal(first["touch_signal"][0, 0].numpy(), touch.astype(np.float32))
    assert np.array_equal(clouds[0][0], points.astype(np.float32))
    # a contact point lies on the object: between the icosahedron's inscribed sphere (0.795 r) and its circumscribed one
    centre = tu.POS + 0.015 * tu.ROT[:, 0]
    radius = np.linalg.norm(clouds[0][0] - centre, axis=1)
    assert radius.max() <= 0.004 * (1 + 1e-4) and radius.min() >= 0.004 * 0.79


def test_unknown_grasp_is_no_intersection(sampler):
    got = sampler.sample([2, 2], touch_point_cloud=True)
    assert got["touch_status"][0] == ["touch"] * 4 and got["touch_status"][1] == ["no_intersection"] * 4
    for key in ("touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"):
        assert not got[key][1].any()
    assert all(len(c) == 0 for c in got["touch_point_cloud"][1])
    nothing = sampler.sample([7, 7])
    assert nothing["touch_status"] == [["no_intersection"] * 4] * 2 and not nothing["touch_signal"].any()
    assert "touch_point_cloud" not in nothing and nothing["touch_signal"].shape == (2, 4, 121, 121, 3)
    assert sampler.sample([0, 0], touch=False) == {}
    with pytest.raises(ValueError, match="actions for 2 loaded"):
        sampler.sample([0])


def test_sample_many_equals_its_sample_calls(sampler, first):
    lists = [[0, 1], [2, 2], [1, 0]]
    many = sampler.sample_many(lists, touch_point_cloud=True)
    assert len(many) == 3
    for got, actions in zip(many, lists):
        want = first if actions == [0, 1] else sampler.sample(actions, touch_point_cloud=True)
        assert got["touch_status"] == want["touch_status"]
        for key in ("touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"):
            assert torch.equal(got[key], want[key]), key
        for a, b in zip(got["touch_point_cloud"], want["touch_point_cloud"]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_one_render_call_per_sample_many():
    calls = []

    def counting(*a, **k):
        calls.append((a[3].numel(), k["want_points"]))
        return tr.render(*a, **k)
    s = rendered.RenderedSampler(frame_table(), geometry(), render=counting)
    s.load_objects(NAMES)
    s.sample_many([[1, 1], [2, 2]])
    assert calls == [(2 * 3 + 4, False)]                    # the live views only: 3 + 3 fingers of action 1, "ball"'s four of action 2
    s.sample([7, 7])
    assert len(calls) == 1                                  # nothing to render: no call


def test_both_source_kinds_agree(tmp_path, first):
    """A dataset tree (``<name>_verts.npy`` / ``_faces.npy`` beside the names, ``grasp_info/<id>/<action>/<f>_ref_frame.npy``)
    against the mappings."""
    root = tmp_path / "data"
    (root / "object_info").mkdir(parents=True)
    for obj, (v, f) in geometry().items():
        np.save(root / "object_info" / f"{obj}_verts.npy", v)
        np.save(root / "object_info" / f"{obj}_faces.npy", f)
    for (obj, action), (pos, rot, present) in frame_table().items():
        d = root / "grasp_info" / obj / str(action)
        d.mkdir(parents=True)
        for f in np.flatnonzero(present):
            np.save(d / f"{f}_ref_frame.npy", {"pos": pos[f], "rot": rot[f]}, allow_pickle=True)
    s = rendered.RenderedSampler(str(root), render=tr.render)
    s.load_objects([str(root / "object_info" / o) for o in OBJECTS], from_dataset=True, scale=3.1)
    got = s.sample([0, 1], touch_point_cloud=True)
    assert got["touch_status"] == first["touch_status"]
    for key in ("touch_signal", "depths", "finger_transfrom_pos", "finger_transform_rot_M"):
        assert torch.equal(got[key], first[key]), key
    s.disconnect()
    with pytest.raises(ValueError, match="neither a mapping"):
        rendered.RenderedSampler(str(tmp_path / "nowhere"), render=tr.render)
    with pytest.raises(KeyError, match="no geometry"):
        rendered.RenderedSampler(frame_table(), {}, render=tr.render).load_objects(NAMES)


def test_active_touch_accepts_it():
    """``ActiveTouch`` takes the class as it takes any sampler (``env_util``'s construction; the models are not loaded here: the
    sampler check and ``_signals`` are what concerns a sampler)."""
    s = rendered.RenderedSampler(frame_table(), geometry(), render=tr.render)
    assert environment.ActiveTouch._factory_of(s) is None                      # an instance, not a factory: accepted as it is
    env = environment.ActiveTouch.__new__(environment.ActiveTouch)
    env.args, env.device, env.sampler = eu.env_args("a", finger=False), torch.device("cpu"), s
    s.load_objects(NAMES)
    touch, pos, rot, status = env._signals(s.sample([0, 1], touch_point_cloud=True))
    assert touch.shape == (2, 4, 3, 121, 121) and 0.0 <= float(touch.min()) and float(touch.max()) <= 1.0
    assert pos.shape == (2, 4, 3) and rot.shape == (2, 4, 3, 3) and status[1][3] == "no_intersection"
    env.args = eu.env_args("a", finger=True)
    touch, pos, rot, status = env._signals(s.sample([0, 1], touch_point_cloud=True))
    assert touch.shape == (2, 1, 3, 121, 121) and status == [["touch"], ["touch"]]
