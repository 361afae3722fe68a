"""The end-to-end GPU test of the data-set bake: from ``object_info`` and finger frames (``chart_head_util.write_bake_tree``: two
icospheres, three actions) through ``save_point_info`` -> ``save_image_info`` -> ``save_touch_signals`` -> ``save_touch_info`` ->
``make_data_split`` to a tree that ``data_loaders.py``'s three loaders read, with every stored signal held bit for bit against
what ``RenderedSampler`` answers for the same scene from mappings."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from chart_head_util import BAKE_OBJECTS as OBJECTS, bake_scene, seeded_encoder, write_bake_tree

pytestmark = pytest.mark.gpu

A = 3
EMPTY = dict(written=0, skipped_existing=2, skipped_no_grasps=0, views=0, touch=0, no_touch=0, no_intersection=0)


def records(root):
    """{relative path: bytes} of every touch record of a tree."""
    return {os.path.relpath(f, root): open(f, "rb").read() for kind in ("touch", "points")
            for f in glob.glob(os.path.join(root, "grasp_info", "*", "*", f"*_{kind}.npy"))}


@pytest.fixture(scope="module")
def baked(cuda, tmp_path_factory):
    from a3vt_amd.pterotactyl.utility import data_making
    geometry, frames = bake_scene()
    root = write_bake_tree(str(tmp_path_factory.mktemp("tree") / "data"), geometry, frames)
    np.random.seed(0)                                                          # (save_point_info draws from NumPy's generator)
    counts = {"points": data_making.save_point_info(os.path.join(root, "object_info"), os.path.join(root, "point_cloud_info"), dim=32,
                                                    num_points=2000),
              "images": data_making.save_image_info(root),
              "signals": data_making.save_touch_signals(root, num_actions=A),
              "charts": data_making.save_touch_info(root, encoder=seeded_encoder(cuda), num_actions=50),   # (the loader reads 50 actions)
              "split": data_making.make_data_split(root, sizes=(1, 0, 0, 1, 0))}
    return root, counts


@pytest.fixture(scope="module")
def sampler(cuda):
    from a3vt_amd.pterotactyl.policies import rendered
    geometry, frames = bake_scene()
    s = rendered.RenderedSampler(frames, geometry, pack_points=False)          # the same scene from mappings, read the padded way
    s.load_objects([f"/data/object_info/{o}" for o in OBJECTS])
    return s


@pytest.fixture(scope="module")
def answers(sampler):
    return [sampler.sample([a, a], touch_point_cloud=True, vision=(a == 0)) for a in range(A)]


def loader_args(root, **kw):
    return SimpleNamespace(data_root=root, limit_data=False, num_grasps=2, number_points=500, use_img=True, use_touch=True, finger=False,
                           eval=False, val_grasps=-1, num_samples=64, env_batch_size=1, **kw)


def test_the_counts_of_the_chain(baked, answers):
    root, counts = baked
    status = np.array([[answers[a]["touch_status"][e] for a in range(A)] for e in range(2)])
    assert sorted(np.unique(status)) == ["no_intersection", "no_touch", "touch"]
    assert counts["points"] == sorted(OBJECTS) and counts["images"] == dict(written=2, skipped_existing=0, skipped_no_surface=0)
    assert counts["signals"] == dict(written=2, skipped_existing=0, skipped_no_grasps=0, views=2 * A * 4, touch=int((status == "touch").sum()),
                                     no_touch=int((status == "no_touch").sum()), no_intersection=int((status == "no_intersection").sum()))
    assert counts["charts"]["written"] == 2 and counts["charts"]["touch"] == counts["signals"]["touch"]
    split = counts["split"]
    assert sorted(split["recon_train"] + split["valid"]) == sorted(OBJECTS) and not split["auto_train"] + split["RL_train"] + split["test"]
    assert not glob.glob(os.path.join(root, "grasp_info", "*", ".baking")) and not glob.glob(os.path.join(root, "*", "*", "*", ".*"))


def test_the_vision_and_active_loaders_find_their_objects(baked, answers):
    from a3vt_amd.pterotactyl.utility import data_loaders
    root, counts = baked
    args = loader_args(root)
    for set_type in ("recon_train", "valid"):
        obj = counts["split"][set_type][0]
        ds = data_loaders.mesh_loader_vision(args, set_type)
        assert [n for n, _ in ds.object_names] == [obj] * (1 if set_type == "recon_train" else 5)
        item = ds[0]
        img = item["img"]
        assert img.shape == (3, 256, 256) and img.dtype == torch.float32 and 0.0 <= float(img.min()) and float(img.max()) <= 1.0
        stored = np.load(os.path.join(root, "images_colourful", f"{obj}.npy"))
        assert stored.shape == (256, 256, 3) and stored.dtype == np.uint8
        vision = answers[0]["vision"][OBJECTS.index(obj)]
        assert np.array_equal(stored, vision) and torch.equal(img, torch.from_numpy(vision).float().permute(2, 0, 1) / 255.0)
        assert item["gt_points"].shape == (500, 3) and item["touch_charts"].shape == (2, 4, 25, 4)
        active = data_loaders.mesh_loader_active(args, set_type)
        assert active.object_names == [obj] and len(active) == 1 and active[0]["names"] == os.path.join(root, "object_info", obj)
        assert torch.equal(active[0]["img"], img)
    assert data_loaders.mesh_loader_active(args, "RL_train").object_names == []


def test_the_touch_loader_reads_the_samplers_signals(baked, answers):
    from a3vt_amd.pterotactyl.utility import data_loaders
    root, counts = baked
    args = loader_args(root)
    seen = 0
    for set_type in ("recon_train", "valid"):
        obj = counts["split"][set_type][0]
        e = OBJECTS.index(obj)
        ds = data_loaders.mesh_loader_touch(args, set_type)
        want = sorted([obj, str(a), str(f)] for a in range(A) for f in range(4) if answers[a]["touch_status"][e][f] == "touch")
        assert sorted(ds.object_names) == want and len(want) > 0               # exactly the "touch" views of the status table
        for index, (_, a, f) in enumerate(ds.object_names):
            a, f = int(a), int(f)
            item = ds[index]
            signal = answers[a]["touch_signal"][e, f]
            assert torch.equal(item["sim_touch"], signal.to(torch.uint8).float().permute(2, 0, 1) / 255.0), (obj, a, f)
            stored = np.load(os.path.join(root, "grasp_info", obj, str(a), f"{f}_touch.npy"))
            assert stored.dtype == np.uint8 and np.array_equal(stored, signal.numpy().astype(np.uint8))
            points = np.load(os.path.join(root, "grasp_info", obj, str(a), f"{f}_points.npy"))
            cloud = answers[a]["touch_point_cloud"][e][f]
            assert points.dtype == np.float32 and len(cloud) > 0 and np.array_equal(points.view(np.uint32), cloud.view(np.uint32)), (obj, a, f)
            assert item["samples"].shape == (64, 3) and torch.equal(item["pos"], answers[a]["finger_transfrom_pos"][e, f])
            seen += 1
    assert seen == counts["signals"]["touch"]


def test_a_second_run_a_planted_marker_and_both_read_paths(baked, cuda, tmp_path):
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.utility import data_making
    root, counts = baked
    first = records(root)
    stamps = {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in first}
    assert data_making.save_touch_signals(root, num_actions=A) == EMPTY        # a second run writes nothing
    assert data_making.save_image_info(root) == dict(written=0, skipped_existing=2, skipped_no_surface=0)
    assert {f: os.stat(os.path.join(root, f)).st_mtime_ns for f in first} == stamps
    # the other read path on a tree of its own: the same bytes, file for file
    geometry, frames = bake_scene()
    other = write_bake_tree(str(tmp_path / "data"), geometry, frames)
    ops.touch_pack_launches(reset=True)
    again = data_making.save_touch_signals(other, num_actions=A, pack_points=not data_making.BAKE_PACK_POINTS)
    assert ops.touch_pack_launches() == {"calls": 0 if data_making.BAKE_PACK_POINTS else 1}   # one pack launch for the whole batch
    assert again == counts["signals"] and records(other) == first
    # a planted marker: the object counts as not yet written and is written again
    victim = sorted(f for f in first if f.startswith(os.path.join("grasp_info", "ball")))[0]
    with open(os.path.join(other, victim), "wb") as f:
        f.write(b"half a file")
    open(os.path.join(other, "grasp_info", "ball", ".baking"), "w").close()
    third = data_making.save_touch_signals(other, num_actions=A, pack_points=True)
    assert third["written"] == 1 and third["skipped_existing"] == 1 and third["views"] == A * 4
    assert records(other) == first and not os.path.exists(os.path.join(other, "grasp_info", "ball", ".baking"))
