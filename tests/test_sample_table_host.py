"""CPU tests of the per-episode touch table's host side (no GPU): ``sample_table`` of ``RenderedSampler`` (driven by the NumPy
emulation ``touch_render_ref.render``, as ``test_rendered_sampler_host.py`` drives the class) and of ``RecordedSampler`` against their
own ``sample``, bit for bit; ``ops.touch_assemble`` on CPU tensors against the NumPy loop of ``touch_assemble_util``; the knob's
refusals in ``ActiveTouch``."""
import numpy as np
import pytest
import torch

import env_util as eu
import touch_assemble_util as ta
import touch_render_ref as tr
from a3vt_amd import ops
from a3vt_amd.pterotactyl.policies import environment, recorded, rendered
from test_rendered_sampler_host import NAMES, OBJECTS, frame_table, geometry

A = 4                                   # actions 0..2 of ``frame_table`` ("pebble" has no action 2) and action 3, which nobody has
KEYS = ("touch_signal", "finger_transfrom_pos", "finger_transform_rot_M")
CODES = {"touch": 2, "no_touch": 1, "no_intersection": 0}


def stacked(sampler, fingers=(0, 1, 2, 3)):
    """The table that ``sample([a] * E)`` for every a spells: the four keys, (E, A, Fs, ...)."""
    per_action = [sampler.sample([a] * len(OBJECTS)) for a in range(A)]
    fingers = list(fingers)
    want = {key: torch.stack([r[key][:, fingers] for r in per_action], dim=1) for key in KEYS}
    want["touch_code"] = torch.tensor([[[CODES[r["touch_status"][e][f]] for f in fingers] for r in per_action]
                                       for e in range(len(OBJECTS))], dtype=torch.int32)
    return want


def same(got, want):
    assert set(got) == set(KEYS) | {"touch_code"}
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key], want[key]), key
    assert got["touch_code"].dtype == torch.int32 and got["touch_signal"].dtype == torch.float32


class Counting:
    def __init__(self):
        self.calls = []

    def __call__(self, *a, **k):
        self.calls.append((a[3].numel(), k["want_points"], k["want_touch"]))
        return tr.render(*a, **k)


@pytest.fixture(scope="module")
def sampler():
    s = rendered.RenderedSampler(frame_table(), geometry(), render=Counting())
    s.load_objects(NAMES)
    return s


@pytest.fixture(scope="module")
def full(sampler):
    """(the full table, the render calls it took, the table its ``sample`` calls spell): computed once."""
    del sampler.render.calls[:]
    table = sampler.sample_table(A)
    calls = list(sampler.render.calls)
    return table, calls, stacked(sampler)


def test_rendered_table_equals_its_sample_calls(full):
    table, calls, want = full
    assert table["touch_signal"].shape == (2, A, 4, 121, 121, 3) and table["finger_transform_rot_M"].shape == (2, A, 4, 3, 3)
    same(table, want)
    assert len(np.unique(table["touch_code"].numpy())) == 3 and table["touch_signal"].any()       # all three codes are in it
    # ONE render call: the live views alone (4 + 3 + 4 of "ball", 4 + 3 of "pebble"), no contact points
    assert calls == [(18, False, True)]


def test_a_missing_frame_and_an_unknown_grasp_are_code_0_and_zeros(full):
    table = full[0]
    assert table["touch_code"][:, 1, 3].tolist() == [0, 0]                   # action 1: finger 3 has no frame
    assert table["touch_code"][1, 2].tolist() == [0] * 4                     # "pebble" has no action 2
    assert not table["touch_code"][:, 3].any()                               # nobody has action 3
    for key in KEYS:
        assert not table[key][:, 1, 3].any() and not table[key][1, 2].any() and not table[key][:, 3].any(), key
    assert table["touch_code"][0, 0].tolist() == [2, 2, 1, 2]                # "ball", action 0: finger 2 looks away


def test_only_the_fingers_asked_for_are_rendered(sampler, full):
    del sampler.render.calls[:]
    one = sampler.sample_table(A, fingers=[1])
    assert sampler.render.calls == [(5, False, True)]                        # finger 1 of the five grasps that exist
    same(one, {key: value[:, :, 1:2] for key, value in full[0].items()})
    del sampler.render.calls[:]
    two = sampler.sample_table(A, fingers=(3, 0))                            # any order; finger 3 is missing in action 1
    assert sampler.render.calls == [(5 + 3, False, True)]
    same(two, {key: value[:, :, [3, 0]] for key, value in full[0].items()})
    same(two, stacked(sampler, fingers=(3, 0)))
    for bad in ([], [4], [-1], [0, 7]):
        with pytest.raises(ValueError, match="fingers"):
            sampler.sample_table(A, fingers=bad)


def test_nothing_to_render_is_no_call_and_too_many_views_are_refused(sampler):
    del sampler.render.calls[:]
    none = sampler.sample_table(2, fingers=[3], to_host=False)               # (to_host is accepted; the fake renderer is on the host)
    assert sampler.render.calls == [(2, False, True)] and none["touch_signal"].shape == (2, 2, 1, 121, 121, 3)
    empty = rendered.RenderedSampler({}, geometry(), render=sampler.render)
    empty.load_objects(NAMES)
    del sampler.render.calls[:]
    got = empty.sample_table(3)
    assert sampler.render.calls == [] and not got["touch_code"].any() and not got["touch_signal"].any()
    assert got["touch_signal"].shape == (2, 3, 4, 121, 121, 3) and got["touch_code"].dtype == torch.int32
    with pytest.raises(ValueError, match="65537 views"):
        one = rendered.RenderedSampler({}, geometry(), render=sampler.render)
        one.load_objects(NAMES[:1])
        one.sample_table(65537, fingers=[0])
    assert sampler.render.calls == []
    with pytest.raises(RuntimeError, match="load_objects"):
        rendered.RenderedSampler({}, geometry(), render=sampler.render).sample_table(2)


def test_a_tree_reads_every_grasp_once(tmp_path, monkeypatch, full):
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
    read = []
    real = rendered.tree_frames
    monkeypatch.setattr(rendered, "tree_frames", lambda root, obj, action: read.append((obj, action)) or real(root, obj, action))
    s = rendered.RenderedSampler(str(root), render=tr.render)
    s.load_objects([str(root / "object_info" / o) for o in OBJECTS])
    same(s.sample_table(A), full[0])
    assert sorted(read) == sorted((o, a) for o in OBJECTS for a in range(A))


def records():
    table = eu.status_table(77, A)
    recs = eu.records(OBJECTS, A, table, 770)
    del recs[("pebble", 2)]                                                   # an unknown grasp
    return recs


def test_recorded_table_equals_its_sample_calls():
    s = recorded.RecordedSampler(records())
    s.load_objects(NAMES)
    table = s.sample_table(A)
    same(table, stacked(s))
    assert all(not t.is_cuda for t in table.values()) and len(np.unique(table["touch_code"].numpy())) == 3
    assert not table["touch_code"][1, 2].any() and not table["touch_signal"][1, 2].any()
    same(s.sample_table(A, fingers=[1]), {key: value[:, :, 1:2] for key, value in table.items()})
    same(s.sample_table(A, fingers=[2, 0], to_host=False), stacked(s, fingers=(2, 0)))
    with pytest.raises(ValueError, match="fingers"):
        s.sample_table(A, fingers=[4])


SHAPES = [(1, 1, 1, 1, 1, 1), (3, 2, 5, 4, 5, 25), (7, 3, 4, 1, 5, 25)]


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_touch_assemble_on_cpu_tensors_is_the_numpy_loop(shape):
    arrays = ta.inputs(*shape, seed=5)
    G = shape[4]
    tensors = [torch.from_numpy(a.copy()) for a in arrays]
    for slot in sorted({0, G // 2, G - 1}):
        want_c, want_m = ta.reference(*arrays, slot)
        for cand in (tensors[4], arrays[4], arrays[4].tolist(), tensors[4].long()):
            charts, masks = ops.touch_assemble(*tensors[:4], cand, slot)
            assert charts.shape == want_c.shape and masks.shape == want_m.shape and charts.dtype == masks.dtype == torch.float32
            assert np.array_equal(charts.numpy().view(np.uint32), want_c) and np.array_equal(masks.numpy().view(np.uint32), want_m)
        flat_masks = tensors[3].squeeze(-1)                                   # (E, F, G, C) is taken as well
        assert torch.equal(ops.touch_assemble(tensors[0], tensors[1], tensors[2], flat_masks, cand, slot)[1].view(torch.int32),
                           masks.view(torch.int32))
    assert all(np.array_equal(t.numpy().view(np.uint32), a.view(np.uint32)) for t, a in zip(tensors, arrays))   # inputs as they were


def test_touch_assemble_refuses_on_the_host():
    K, E, A_, F, G, C = 3, 2, 5, 4, 5, 25
    t = [torch.from_numpy(a) for a in ta.inputs(K, E, A_, F, G, C, seed=6)]
    for bad in (-1, A_):
        cand = t[4].clone()
        cand[2, 1] = bad
        with pytest.raises(ValueError, match=rf"candidates outside \[0, {A_}\)"):
            ops.touch_assemble(*t[:4], cand, 0)
        with pytest.raises(ValueError, match="candidates outside"):
            ops.touch_assemble(*t[:4], cand.tolist(), 0)
    for slot in (-1, G):
        with pytest.raises(ValueError, match=f"slot={slot}"):
            ops.touch_assemble(*t, slot)
    with pytest.raises(ValueError, match="table_codes"):
        ops.touch_assemble(t[0], t[1][:, :-1], t[2], t[3], t[4], 0)
    with pytest.raises(ValueError, match="table_codes"):
        ops.touch_assemble(t[0], t[1].long(), t[2], t[3], t[4], 0)
    with pytest.raises(ValueError, match="state_charts"):
        ops.touch_assemble(t[0], t[1], t[2][:, :-1], t[3], t[4], 0)
    with pytest.raises(ValueError, match="state_masks"):
        ops.touch_assemble(t[0], t[1], t[2], t[3][:, :, :-1], t[4], 0)
    with pytest.raises(ValueError, match="candidates"):
        ops.touch_assemble(*t[:4], t[4][:, :1], 0)
    with pytest.raises(ValueError, match="candidates"):
        ops.touch_assemble(*t[:4], t[4].float(), 0)


def bare_env(sampler, **knobs):
    env = environment.ActiveTouch.__new__(environment.ActiveTouch)
    env.args, env.device, env.sampler = eu.env_args("a", **knobs), torch.device("cpu"), sampler
    return env


def test_the_knob():
    """``args.touch_table``: off by default and when None; on with a sampler without ``sample_table`` is a ``ValueError`` that names
    both."""
    class Plain:
        load_objects = sample = disconnect = lambda self, *a, **k: None

    assert environment.TOUCH_TABLE_DEFAULT is False
    s = recorded.RecordedSampler(records())
    assert bare_env(s)._use_table() is False and bare_env(s, touch_table=None)._use_table() is False
    assert bare_env(s, touch_table=False)._use_table() is False and bare_env(Plain(), touch_table=None)._use_table() is False
    assert bare_env(s, touch_table=True)._use_table() is True
    with pytest.raises(ValueError, match="touch_table.*Plain.*sample_table"):
        bare_env(Plain(), touch_table=True)._use_table()


@pytest.mark.parametrize("finger", [True, False])
def test_signals_and_the_table_share_one_image_arithmetic(finger):
    """``_signals`` of a ``sample`` result and ``_images`` of the table's signals are the same numbers: ``/ 255.0`` in fp32, under
    ``finger`` after the truncation through uint8."""
    s = recorded.RecordedSampler(records())
    s.load_objects(NAMES)
    env = bare_env(s, finger=finger)
    fingers = [1] if finger else [0, 1, 2, 3]
    images = env._images(s.sample_table(A, fingers=fingers)["touch_signal"])
    assert images.shape == (2, A, len(fingers), 3, 121, 121)
    for a in range(A):
        raw = s.sample([a, a])["touch_signal"][:, fingers]
        touch = env._signals(s.sample([a, a]))[0]
        assert torch.equal(images[:, a], touch)
        want = (torch.from_numpy(raw.numpy().astype(np.uint8)).float() if finger else raw).permute(0, 1, 4, 2, 3) / 255.0
        assert torch.equal(touch, want)
