"""CPU tests of the placement without a hull: ``ops.hull_place`` on CPU tensors (the float64 NumPy form of the rule in
``include/a3vt.h``) against ``grasping.place_hand`` on SciPy's hull (``hull_place_ref``), and the layers above it —
``KinematicGrasp(placement="device")`` with its fallback for undecided pairs, and ``data_making.save_simulation(placement=)``.

On decided pairs the status equals the reference's, the simplex spans the reference facet's plane (normal to 1e-12, t to 1e-12
relative) and the float64 pose lies within 1e-12 of ``place_hand``'s: both sides form the same float64 expressions from the same
plane, and ``place_hand``'s quaternion round trips move R by about 1e-16.  Measured here: no status 2 on any shape, 0 undecided
pairs of 50 on every shape but ``sym`` (2 of 50), and about two thirds of the pose elements differ at all, by some 1e-16."""
import os

import numpy as np
import pytest
import torch

import grasp_ref as gr
import hull_place_ref as hr


def place(verts, offsets=None, **kw):
    from a3vt_amd import ops
    offsets = [0, len(verts)] if offsets is None else offsets
    out = ops.hull_place(torch.from_numpy(np.array(verts, np.float32)), offsets, hr.directions(), **kw)
    return {k: v.numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def singles():
    """Every shape's single-mesh result, computed once."""
    return {name: place(hr.shape(name)) for name in hr.SHAPES}


@pytest.fixture(scope="module")
def hand():
    return gr.hand()


@pytest.mark.parametrize("name", hr.SHAPES)
def test_numpy_form_against_place_hand(singles, name):
    out = singles[name]
    assert out["status"].dtype == np.int32 and out["simplex"].dtype == np.int32 and out["t"].dtype == np.float64
    assert out["base_pos"].shape == (1, 50, 3) and out["base_rot"].shape == (1, 50, 3, 3) and out["base_pos"].dtype == np.float64
    compared, differing, undecided = hr.check(name, {k: v[0] for k, v in out.items()}, exact64=True, allow_undecided=name == "sym")
    print(f"{name}: {compared} pose elements compared, {differing} differ at all, {undecided} pairs of status 2")
    ref = hr.reference(name)
    if name == "far":
        assert ref["present"].sum() == 1 and (out["status"][0] == 1).sum() == 49
    elif name != "sym":
        assert compared == 12 * 50


def test_batch_rows_equal_single_calls(singles):
    names = ("tetra", "cloud257", "far")
    verts = np.concatenate([hr.shape(n) for n in names])
    offsets = np.cumsum([0] + [len(hr.shape(n)) for n in names])
    out = place(verts, offsets)
    for m, name in enumerate(names):
        for key, value in singles[name].items():
            assert np.array_equal(out[key][m], value[0]), (name, key)


def test_meshes_place_hand_refuses():
    v = hr.shape("ico2").copy()
    assert (place(v[:3])["status"] == 1).all() and (place(v[:0])["status"] == 1).all()
    v[7, 1] = np.nan
    out = place(v)
    assert (out["status"] == 1).all() and not out["base_pos"].any() and (out["simplex"] == -1).all()
    v[7, 1] = np.inf
    assert (place(v)["status"] == 1).all()
    # an empty mesh between two others
    both = np.concatenate([hr.shape("tetra"), hr.shape("box")])
    out = place(both, [0, 4, 4, 12])
    assert (out["status"][1] == 1).all() and (out["status"][[0, 2]] == 0).all()


def flat_square():
    return (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32) * 0.1 - np.float32(0.05)) + np.array([0, 0, 0.07], np.float32)


def test_a_flat_hull_is_left_to_the_host(hand):
    """Four coplanar points: no pair is placed; a ray that crosses the square ahead of the origin ends in the flatness check (status
    2), and ``grasp_table`` then finds no hull on the host: ``present`` is False, as with the host placement."""
    from a3vt_amd.pterotactyl.simulator.physics.grasping import KinematicGrasp
    v = flat_square()
    out = place(v)
    d = hr.directions()
    t = 0.02 / np.where(d[:, 2] > 0, d[:, 2], np.nan)                     # the square lies in z = 0.02
    crosses = (np.abs(d[:, 0] * t) < 0.049) & (np.abs(d[:, 1] * t) < 0.049)
    assert crosses.sum() >= 3 and (out["status"][0][crosses] == 2).all() and (out["status"] != 0).all()
    geometry = {"flat": (v, np.array([[0, 1, 2], [0, 2, 3]]))}
    grasper = KinematicGrasp(hand, steps=2, device="cpu", placement="device")
    table = grasper.grasp_table(geometry, ["flat"], 50, want_base=True)
    assert not table["present"].any() and not table["pos"].any() and not table["base_pos"].any() and grasper.undecided >= 3


def geometry_two():
    return {"ico2": (hr.shape("ico2"), gr.icosphere(2)[1]), "box": (hr.shape("box"), gr.box_mesh()[1])}


def one_ulp(got, want):
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()


def test_device_placement_against_host_placement(hand):
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    assert grasping.DEVICE_PLACEMENT_DEFAULT is False
    geometry = geometry_two()
    want = dict(want_q=True, want_blocked_step=True, want_base=True, want_hand_pose=True)
    host = grasping.KinematicGrasp(hand, steps=2, device="cpu", placement="host")
    assert grasping.KinematicGrasp(hand, steps=2, device="cpu").placement == "host"
    device = grasping.KinematicGrasp(hand, steps=2, device="cpu", placement="device")
    a, b = host.grasp_table(geometry, ["ico2", "box"], 50, **want), device.grasp_table(geometry, ["ico2", "box"], 50, **want)
    assert device.undecided == 0 and device.placement_seconds > 0
    assert np.array_equal(a["present"], b["present"]) and a["present"].all()
    assert a["base_pos"].dtype == np.float32 and b["base_rot"].shape == (2, 50, 3, 3)
    assert one_ulp(b["base_pos"], a["base_pos"]) and one_ulp(b["base_rot"], a["base_rot"])
    same = (a["base_pos"] == b["base_pos"]).all(axis=-1) & (a["base_rot"] == b["base_rot"]).all(axis=(-1, -2))
    print(f"{int(same.sum())} of {same.size} base poses are bit-equal")
    assert same.any()
    for key in ("pos", "rot", "q", "blocked_step"):
        assert np.array_equal(a[key][same], b[key][same]), key
    assert np.allclose(a["pos"], b["pos"], atol=1e-6) and len(b["hand_pose"][1][7]) == 28
    with pytest.raises(ValueError, match="placement"):
        grasping.KinematicGrasp(hand, placement="gpu")
    empty = device.grasp_table(geometry, [], 50, want_base=True)
    assert empty["present"].shape == (0, 50, 4) and empty["base_pos"].shape == (0, 50, 3)


def test_undecided_pairs_fall_back_to_place_hand(hand, monkeypatch):
    """``ops.hull_place`` wrapped so that chosen pairs come back as status 2 (zeros, simplex -1): ``grasp_table`` must return the
    host's ``present`` and base poses for them, and build a hull only for the objects that need one."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    geometry = geometry_two()
    geometry["far"] = (hr.shape("far"), gr.icosphere(2)[1])
    ids = ["ico2", "box", "far"]
    forced = [(0, 3), (0, 49), (2, 0), (2, 1), (2, 30)] + [(2, int(np.flatnonzero(hr.reference("far")["present"])[0]))]
    real = ops.hull_place

    def wrapped(*args, **kw):
        out = real(*args, **kw)
        for e, a in forced:
            out["status"][e, a] = 2
            out["base_pos"][e, a], out["base_rot"][e, a], out["simplex"][e, a], out["t"][e, a] = 0, 0, -1, 0
        return out
    monkeypatch.setattr(ops, "hull_place", wrapped)
    hulls = []
    facets_of = grasping.hull_facets
    monkeypatch.setattr(grasping, "hull_facets", lambda v: hulls.append(len(v)) or facets_of(v))
    device = grasping.KinematicGrasp(hand, steps=2, device="cpu", placement="device")
    b = device.grasp_table(geometry, ids, 50, want_base=True)
    assert device.undecided == len(set(forced)) and sorted(hulls) == [162, 162]            # ico2 and far; never the box
    monkeypatch.undo()
    a = grasping.KinematicGrasp(hand, steps=2, device="cpu", placement="host").grasp_table(geometry, ids, 50, want_base=True)
    assert np.array_equal(a["present"], b["present"]) and a["present"][2].any(axis=-1).sum() == 1
    for e, a_ in set(forced):
        assert np.array_equal(a["base_pos"][e, a_], b["base_pos"][e, a_]) and np.array_equal(a["base_rot"][e, a_], b["base_rot"][e, a_])
        assert np.array_equal(a["pos"][e, a_], b["pos"][e, a_])
    assert one_ulp(b["base_pos"], a["base_pos"]) and one_ulp(b["base_rot"], a["base_rot"])


def test_wrapper_refuses_bad_arguments():
    from a3vt_amd import ops
    v = torch.from_numpy(hr.shape("tetra").copy())
    d = hr.directions()
    for bad in (dict(vert_offset=[0, 5]), dict(vert_offset=[2, 1]), dict(vert_offset=[-1, 4]), dict(directions=np.zeros((0, 3))),
                dict(directions=np.ones((129, 3))), dict(directions=np.array([[0.0, 0.0, 0.0]])), dict(directions=np.array([[np.nan, 0, 1]])),
                dict(hand_distance=np.inf), dict(tip_offset=(0, np.nan, 0)), dict(directions=np.ones((3, 2))), dict(vert_offset=[0])):
        args = dict(vert_offset=[0, 4], directions=d)
        args.update(bad)
        with pytest.raises(ValueError):
            ops.hull_place(v, **args)
    with pytest.raises(ValueError):
        ops.hull_place(v.reshape(-1), [0, 4], d)


def test_save_simulation_with_device_placement(hand, tmp_path):
    from a3vt_amd.pterotactyl.utility import data_making
    geometry = {"ball": (hr.shape("ico2"), gr.icosphere(2)[1]), "flat": (flat_square(), np.array([[0, 1, 2], [0, 2, 3]]))}
    listing = {}
    for placement in (None, "device"):
        root = str(tmp_path / str(placement))
        os.makedirs(os.path.join(root, "object_info"))
        for name, (v, f) in geometry.items():
            np.save(os.path.join(root, "object_info", f"{name}_verts.npy"), v)
            np.save(os.path.join(root, "object_info", f"{name}_faces.npy"), f)
        counts = data_making.save_simulation(root, hand, batch=2, num_actions=50, steps=2, device="cpu", signals=False, placement=placement)
        assert counts == dict(written=2, skipped_existing=0, grasps=100, placed=50)
        listing[placement] = sorted(os.path.relpath(os.path.join(d, f), root) for d, _, files in os.walk(root) for f in files)
    assert listing[None] == listing["device"] and len(listing[None]) == 4 + 50 * 4
    for rel in listing[None]:
        if rel.endswith("_ref_frame.npy"):
            a = np.load(os.path.join(str(tmp_path / "None"), rel), allow_pickle=True).item()
            b = np.load(os.path.join(str(tmp_path / "device"), rel), allow_pickle=True).item()
            assert np.allclose(a["pos"], b["pos"], atol=1e-6) and np.allclose(a["rot"], b["rot"], atol=1e-6)
