"""``a3vt_hull_place`` (csrc/hull_place.hip) on the GPU against ``grasping.place_hand`` on SciPy's hull (``hull_place_ref``), and
``KinematicGrasp(placement="device")`` end to end.

On decided pairs (margin >= 1e-4 in the float64 reference; at most 10 % of a shape's pairs may be undecided) the status equals the
reference's, the simplex spans the reference facet's plane (normal to 1e-12, t to 1e-12 relative), and every element of the
float32 pose lies within one float32 ulp of ``place_hand``'s pose cast to float32: the kernel forms the same float64 expressions
from the same plane, so only the last rounding can differ.  A status 2 on a decided pair is a failure on every shape but ``sym``.
Each test prints how many pose elements differ at all.  Measured on an MI355X: of 6 588 pose elements compared over the twelve
shapes none differs, no pair comes back status 2 (``sym`` included: its two undecided pairs are answered), and the kernel's
statuses and simplices equal the float64 NumPy form's on every pair.

Shapes (``hull_place_ref.shape``): V = 4 and 8 (below a wave), 162, 344 with duplicate vertices, 642 = 2 x 256 + 130 (a ragged last
stride), a cloud with interior points cut at 255 / 256 / 257 (the workgroup's edge) and whole (1000), an object off the origin (one
hit, 49 misses), a 10 242-vertex sphere (50 workgroups on one mesh) and a sphere symmetric about the origin."""
import numpy as np
import pytest
import torch

import grasp_ref as gr
import hull_place_ref as hr

pytestmark = pytest.mark.gpu
BATCHED = tuple(name for name in hr.SHAPES if name != "ico5")


def place(cuda, verts, offsets=None):
    from a3vt_amd import ops
    offsets = [0, len(verts)] if offsets is None else offsets
    out = ops.hull_place(torch.from_numpy(np.array(verts, np.float32)).to(cuda), offsets, hr.directions())
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def cuda():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def singles(cuda):
    """Every shape's single-mesh result, computed once."""
    return {name: place(cuda, hr.shape(name)) for name in hr.SHAPES}


@pytest.mark.parametrize("name", hr.SHAPES)
def test_kernel_against_place_hand(singles, name):
    out = singles[name]
    assert out["status"].dtype == np.int32 and out["simplex"].dtype == np.int32 and out["t"].dtype == np.float64
    assert out["base_pos"].shape == (1, 50, 3) and out["base_rot"].shape == (1, 50, 3, 3) and out["base_pos"].dtype == np.float32
    compared, differing, undecided = hr.check(name, {k: v[0] for k, v in out.items()}, exact64=False, allow_undecided=name == "sym")
    print(f"{name}: {compared} pose elements compared, {differing} differ at all, {undecided} pairs of status 2")
    if name == "far":
        assert (out["status"][0] == 1).sum() == 49
    elif name != "sym":
        assert compared == 12 * 50


def test_kernel_equals_the_numpy_form_in_status_and_simplex(singles):
    """The NumPy form states the kernel's operations in the kernel's order: the integers agree on every pair, decided or not."""
    from a3vt_amd import ops
    for name in ("tetra", "box", "cloud257", "dumbbell", "far", "sym"):
        host = ops.hull_place(torch.from_numpy(hr.shape(name).copy()), [0, len(hr.shape(name))], hr.directions())
        assert np.array_equal(host["status"].numpy(), singles[name]["status"]), name
        assert np.array_equal(host["simplex"].numpy(), singles[name]["simplex"]), name


def test_batched_call_two_calls_and_launch_count(cuda, singles):
    from a3vt_amd import ops
    verts = np.concatenate([hr.shape(n) for n in BATCHED])
    offsets = np.cumsum([0] + [len(hr.shape(n)) for n in BATCHED])
    ops.hull_place_launches(reset=True)
    first = place(cuda, verts, offsets)
    assert ops.hull_place_launches() == {"calls": 1, "launches": 1}
    second = place(cuda, verts, offsets)
    assert ops.hull_place_launches(reset=True) == {"calls": 2, "launches": 2}
    for key, value in first.items():
        assert value.tobytes() == second[key].tobytes(), key
        for m, name in enumerate(BATCHED):
            assert value[m].tobytes() == singles[name][key][0].tobytes(), (name, key)


def test_meshes_place_hand_refuses(cuda):
    v = hr.shape("ico3").copy()
    v[641, 2] = np.nan                                    # the last vertex: the ragged stride's last lane
    both = np.concatenate([hr.shape("tetra"), v, hr.shape("box")[:3]])
    out = place(cuda, both, [0, 4, 4, 646, 649])
    assert (out["status"][0] == 0).all() and (out["status"][1:] == 1).all()
    assert not out["base_pos"][1:].any() and not out["base_rot"][1:].any() and (out["simplex"][1:] == -1).all() and not out["t"][1:].any()


def one_ulp(got, want):
    return (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()


def tables(cuda, geometry, ids, monkeypatch=None, forced=()):
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.simulator.physics import grasping
    hand = gr.hand()
    want = dict(want_q=True, want_blocked_step=True, want_base=True)
    host = grasping.KinematicGrasp(hand, steps=16, device=cuda, placement="host").grasp_table(geometry, ids, 50, **want)
    if forced:
        real = ops.hull_place

        def wrapped(*args, **kw):
            out = real(*args, **kw)
            for e, a in forced:
                out["status"][e, a] = 2
                out["base_pos"][e, a], out["base_rot"][e, a], out["simplex"][e, a], out["t"][e, a] = 0, 0, -1, 0
            return out
        monkeypatch.setattr(ops, "hull_place", wrapped)
    grasper = grasping.KinematicGrasp(hand, steps=16, device=cuda, placement="device")
    ops.hull_place_launches(reset=True)
    ops.grasp_launches(reset=True)
    device = grasper.grasp_table(geometry, ids, 50, **want)
    assert ops.hull_place_launches() == {"calls": 1, "launches": 1} and ops.grasp_launches()["calls"] == 1
    return host, device, grasper


def test_sym_answers_and_fallback(cuda, singles, monkeypatch):
    """``sym``: every status 0 or 1 answer on a decided pair is right (``check`` above, status 2 allowed), and ``grasp_table``
    returns the host's base poses for the pairs the kernel leaves undecided — and for three more that are forced to status 2
    here, so that the path runs whatever the kernel decides."""
    status = singles["sym"]["status"][0]
    hr.check("sym", {k: v[0] for k, v in singles["sym"].items()}, exact64=False, allow_undecided=True)
    forced = sorted(set(np.flatnonzero(status == 2).tolist()) | {0, 21, 49})
    geometry = {"sym": (hr.shape("sym"), gr.icosphere(3)[1])}
    host, device, grasper = tables(cuda, geometry, ["sym"], monkeypatch, [(0, a) for a in forced])
    assert grasper.undecided == len(forced)
    assert np.array_equal(host["present"], device["present"])
    for a in forced:
        assert np.array_equal(host["base_pos"][0, a], device["base_pos"][0, a]) and np.array_equal(host["base_rot"][0, a], device["base_rot"][0, a])
        assert np.array_equal(host["pos"][0, a], device["pos"][0, a]) and np.array_equal(host["q"][0, a], device["q"][0, a])


def test_end_to_end_device_against_host_placement(cuda):
    geometry = {"ico3": (hr.shape("ico3"), gr.icosphere(3)[1]), "box": (hr.shape("box"), gr.box_mesh()[1])}
    host, device, grasper = tables(cuda, geometry, ["ico3", "box"])
    assert grasper.undecided == 0
    assert np.array_equal(host["present"], device["present"]) and host["present"].all()
    assert one_ulp(device["base_pos"], host["base_pos"]) and one_ulp(device["base_rot"], host["base_rot"])
    same = (host["base_pos"] == device["base_pos"]).all(axis=-1) & (host["base_rot"] == device["base_rot"]).all(axis=(-1, -2))
    print(f"{int(same.sum())} of {same.size} base poses are bit-equal")
    assert same.any()
    for key in ("pos", "rot", "q", "blocked_step"):
        assert np.array_equal(host[key][same], device[key][same]), key
