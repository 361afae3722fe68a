"""GPU tests of the ground-truth point-cloud kernels (csrc/voxel.hip) through ``ops.voxel_surface`` / ``ops.voxel_points`` /
``ops.voxel_depth_maps``: every stage bit-equal to the reference's results in ``g24_points.npz`` (0.obj at 128: ``g6_chamfer.npz``),
to the exact emulation ``points_ref`` where no fixture exists; batch invariance, workspace hygiene, launch counts.  Every comparison
is integer or bit equality."""
import functools

import numpy as np
import pytest
import torch

import points_ref
from points_util import CASES, abc, case, cells_of, special_meshes

pytestmark = pytest.mark.gpu


def _batch(meshes, dev):
    verts = torch.from_numpy(np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1, 3) for v, _ in meshes])).to(dev)
    faces = torch.from_numpy(np.concatenate([np.asarray(f, dtype=np.int32).reshape(-1, 3) for _, f in meshes])).to(dev)
    off = lambda k: torch.tensor(np.concatenate(([0], np.cumsum([len(m[k]) for m in meshes]))), dtype=torch.int32, device=dev)  # noqa: E731
    return verts, faces, off(0), off(1)


def _run(meshes, dim, dev, index=None):
    """Every stage of a batch -> a list with one dict(occ, odm, surface, aligned[, cloud]) of host arrays per mesh."""
    from a3vt_amd import ops
    state = ops.voxel_surface(*_batch(meshes, dev), dim, want_occupancy=True, want_depth_maps=True)
    out = ops.voxel_points(state, index=None if index is None else torch.from_numpy(np.asarray(index, dtype=np.int64)).to(dev),
                           want_aligned=True)
    assert out["offset"][-1] == out["surface"].shape[0]
    res = []
    for m in range(len(meshes)):
        rows = slice(out["offset"][m], out["offset"][m + 1])
        res.append(dict(occ=cells_of(state.occupancy[m].cpu().numpy()), odm=state.depth_maps[m].cpu().numpy(),
                        surface=out["surface"][rows].cpu().numpy(), aligned=out["aligned"][rows].cpu().numpy()))
        if index is not None:
            res[-1]["cloud"] = out["cloud"][m].cpu().numpy()
    return res


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _check_stages(got, want):
    assert _same(got["occ"], want["occ"]), "occupancy"
    assert _same(got["odm"], want["odm"]), "depth maps"
    assert _same(got["surface"], want["surface"]), "surface list or its order"
    assert _same_bits(got["aligned"], want["aligned"]), "realigned cloud"


@functools.lru_cache(maxsize=None)
def _emulated(name):
    verts, faces, dim = special_meshes()[name]
    return points_ref.pipeline(verts, faces, dim)


@pytest.mark.parametrize("tag", CASES)
def test_fixture_case_equals_the_reference(cuda, tag):
    c = case(tag)
    got = _run([(c["verts"], c["faces"])], c["dim"], cuda, index=c["choices"][None])[0]
    _check_stages(got, c)
    assert _same_bits(got["cloud"], c["cloud"]), "gathered cloud"


def test_abc_object_at_128_equals_g6(cuda):
    c = abc()
    got = _run([(c["verts"], c["faces"])], 128, cuda)[0]
    assert got["aligned"].shape == (2176, 3) and _same_bits(got["aligned"], c["aligned"])


@pytest.mark.parametrize("name", sorted(special_meshes()))
def test_special_mesh_equals_the_emulation(cuda, name):
    verts, faces, dim = special_meshes()[name]
    want = _emulated(name)
    index = (np.arange(777, dtype=np.int64) * 7919) % (want["surface"].shape[0] * 4)
    got = _run([(verts, faces)], dim, cuda, index=index[None])[0]
    _check_stages(got, want)
    assert _same_bits(got["cloud"], points_ref.gather(want["aligned"], index))


def test_batch_equals_the_meshes_alone(cuda):
    """Three meshes of different sizes with an empty one in the middle; vertex and face offsets (360, 360, 364 faces) are no
    multiples of 64.  A mesh's results do not depend on what else is in the batch."""
    a, b = case("obj1_32"), case("tetra24")
    empty = (np.zeros((5, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32))
    meshes = [(a["verts"], a["faces"]), empty, (b["verts"], b["faces"])]
    index = np.stack([(np.arange(400, dtype=np.int64) * (31 + m)) % 1000 for m in range(3)])
    batch = _run(meshes, 32, cuda, index=index)
    _check_stages(batch[0], a)
    assert batch[1]["occ"].shape[0] == 0 and batch[1]["surface"].shape[0] == 0 and not batch[1]["cloud"].any()
    assert (batch[1]["odm"] == 32).all()
    for m in (0, 2):
        alone = _run([meshes[m]], 32, cuda, index=index[m][None])[0]
        _check_stages(batch[m], alone)
        assert _same_bits(batch[m]["cloud"], alone["cloud"])


def test_repeatable_and_the_workspace_does_not_leak(cuda):
    """A dim-128 call, a dim-16 call on another mesh in the same (larger) workspace, the first again."""
    big, small = case("obj1_128"), case("tetra16")
    first = _run([(big["verts"], big["faces"])], 128, cuda, index=big["choices"][None])[0]
    second = _run([(small["verts"], small["faces"])], 16, cuda, index=small["choices"][None])[0]
    third = _run([(big["verts"], big["faces"])], 128, cuda, index=big["choices"][None])[0]
    _check_stages(second, small)
    assert _same_bits(second["cloud"], small["cloud"])
    _check_stages(third, first)
    assert _same_bits(third["cloud"], first["cloud"]) and _same_bits(first["cloud"], big["cloud"])


def test_depth_maps_of_a_given_grid(cuda):
    from a3vt_amd import ops
    g = torch.Generator().manual_seed(3)
    grids = (torch.rand(2, 21, 21, 21, generator=g) > 0.97).to(torch.uint8)
    grids[1, :, 4, :] = 0                                                   # some empty columns
    got = ops.voxel_depth_maps(grids.to(cuda)).cpu().numpy()
    for m in range(2):
        assert _same(got[m], points_ref.depth_maps(cells_of(grids[m].numpy()), 21))
    assert _same(got, ops.voxel_depth_maps(grids).numpy())


def test_points_call_must_follow_its_surface_call(cuda):
    from a3vt_amd import ops
    c = case("tetra8")
    state = ops.voxel_surface(*_batch([(c["verts"], c["faces"])], cuda), 8)
    ops.voxel_surface(*_batch([(c["verts"], c["faces"])], cuda), 16)
    with pytest.raises(RuntimeError, match="voxel_points: M=1 dim=8"):
        ops.voxel_points(state)


def test_launches_do_not_depend_on_the_batch_or_the_depth(cuda):
    """One ``extract_points_batch`` call enqueues the same operations for M = 1 and M = 3, for a mesh that is never subdivided and
    for one subdivided many levels deep; and between the inputs being on the device and the outputs being there, nothing but the read of
    the M counts synchronises the host (torch's sync debug mode raises on any other)."""
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.utility import data_making
    deep, shallow = special_meshes()["wide"], special_meshes()["wide"]
    deep, shallow = (deep[0][:3], deep[1][:1]), (shallow[0][3:], shallow[1][1:] - 3)
    other = case("tetra24")
    counted = []
    for meshes in ([shallow], [deep], [deep, shallow, (other["verts"], other["faces"])]):
        ops.voxel_launches(reset=True)
        clouds = data_making.extract_points_batch(meshes, dim=64, num_points=500, choices=[np.arange(500)] * len(meshes), device=cuda)
        assert all(c is not None and c.shape == (500, 3) for c in clouds)
        counted.append(ops.voxel_launches())
    assert counted[0] == counted[1] == counted[2] and counted[0]["surface"] == 8 and counted[0]["points"] == 2, counted
    # the same two calls under torch's sync detector, the counts known beforehand
    args = _batch([deep, shallow], cuda)
    index = torch.arange(1000, device=cuda).reshape(2, 500)
    counts = ops.voxel_surface(*args, 64).counts.tolist()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        state = ops.voxel_surface(*args, 64)
        out = ops.voxel_points(state, counts=counts, index=index)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = points_ref.pipeline(deep[0], deep[1], 64)
    assert _same_bits(out["cloud"][0].cpu().numpy(), points_ref.gather(want["aligned"], np.arange(500)))


def test_utils_and_extract_points_on_gpu_tensors(cuda):
    from a3vt_amd.pterotactyl.utility import data_making, utils
    c = case("obj1_32")
    verts, faces = torch.from_numpy(c["verts"]).to(cuda), torch.from_numpy(c["faces"]).long().to(cuda)
    voxel = utils.mesh_to_voxel(verts, faces, 32)
    assert voxel.is_cuda and voxel.dtype == torch.float32 and _same(cells_of(voxel.cpu().numpy()), c["occ"])
    odm = utils.extract_ODMs(voxel)
    assert isinstance(odm, np.ndarray) and odm.dtype == np.float64 and _same(odm, c["odm"])
    carved = utils.apply_ODMs(odm, 32)
    assert carved.is_cuda and int(carved.sum()) == c["carved"]
    cells = utils.voxel_to_pointcloud(carved)
    assert _same(cells.cpu().numpy(), c["surface"])
    assert _same_bits(utils.realign_points(cells, verts).cpu().numpy(), c["aligned"])
    np.random.seed(c["seed"])
    cloud = data_making.extract_points(verts, faces, dim=32, num_points=c["cloud"].shape[0])
    assert cloud.is_cuda and _same_bits(cloud.cpu().numpy(), c["cloud"])
