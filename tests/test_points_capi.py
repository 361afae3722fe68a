"""CPU tests (no GPU, no compute): ``a3vt_voxel_surface``, ``a3vt_voxel_depth_maps`` and ``a3vt_voxel_points`` refuse what the contract
in ``include/a3vt.h`` excludes with an error code and a message that names the argument, before anything is launched or allocated —
every call below passes fake device addresses that must never be dereferenced on the host (the manner of
``test_touch_render_capi.py``)."""
import pytest

FAKE = 0x7F0000001000        # a "device pointer": 16-byte aligned, never mapped on the host
SURFACE = dict(verts=FAKE, V=42, faces=FAKE + 0x1000, F=80, vert_offset=FAKE + 0x2000, face_offset=FAKE + 0x3000, M=2, dim=32,
               occupancy=FAKE + 0x4000, depth_maps=FAKE + 0x5000, counts=FAKE + 0x6000, stream=None)
SURFACE_ORDER = ("verts", "V", "faces", "F", "vert_offset", "face_offset", "M", "dim", "occupancy", "depth_maps", "counts", "stream")
MAPS = dict(voxels=FAKE, M=2, dim=32, depth_maps=FAKE + 0x1000, stream=None)
MAPS_ORDER = ("voxels", "M", "dim", "depth_maps", "stream")
POINTS = dict(M=2, dim=32, total=500, surface=FAKE, aligned=FAKE + 0x1000, index=FAKE + 0x2000, num_points=300, cloud=FAKE + 0x3000,
              stream=None)
POINTS_ORDER = ("M", "dim", "total", "surface", "aligned", "index", "num_points", "cloud", "stream")
CALLS = {"voxel_surface": (SURFACE, SURFACE_ORDER), "voxel_depth_maps": (MAPS, MAPS_ORDER), "voxel_points": (POINTS, POINTS_ORDER)}


@pytest.fixture(scope="module")
def L():
    from a3vt_amd import lib
    return lib.load()


def call(L, who, **changes):
    good, order = CALLS[who]
    a = dict(good, **changes)
    return getattr(L, "a3vt_" + who)(*(a[name] for name in order)), L.a3vt_last_error().decode()


@pytest.mark.parametrize("who", sorted(CALLS))
def test_dim_and_mesh_count_outside(L, who):
    for v in (3, 0, -8, 257):
        rc, msg = call(L, who, dim=v)
        assert rc != 0 and who in msg and f"dim={v}" in msg and "4..256" in msg, (v, msg)
    for v in (0, -1, 4097):
        rc, msg = call(L, who, M=v)
        assert rc != 0 and who in msg and f"M={v}" in msg, (v, msg)
    rc, msg = call(L, who, M=65, dim=256)                                   # 65 * 2^24 voxels > 2^30
    assert rc != 0 and "M=65" in msg and "dim=256" in msg, msg


def test_counts_outside(L):
    for name in ("V", "F"):
        for v in (-1, (1 << 28) + 1):
            rc, msg = call(L, "voxel_surface", **{name: v})
            assert rc != 0 and "voxel_surface" in msg and f"{name}={v}" in msg, (name, v, msg)
    for v in (-1, (1 << 30) + 1):
        rc, msg = call(L, "voxel_points", total=v)
        assert rc != 0 and f"total={v}" in msg, (v, msg)
    for v in (0, -30000, (1 << 28) + 1):
        rc, msg = call(L, "voxel_points", num_points=v)
        assert rc != 0 and f"num_points={v}" in msg, (v, msg)


@pytest.mark.parametrize("who,name", [("voxel_surface", n) for n in ("verts", "faces", "vert_offset", "face_offset", "counts")] +
                         [("voxel_depth_maps", "voxels"), ("voxel_depth_maps", "depth_maps"), ("voxel_points", "surface")])
def test_required_pointers(L, who, name):
    rc, msg = call(L, who, **{name: None})
    assert rc != 0 and who in msg and f"{name}=NULL" in msg, msg


def test_pointers_that_go_together(L):
    rc, msg = call(L, "voxel_points", index=None)
    assert rc != 0 and "index=NULL" in msg and "together" in msg, msg
    rc, msg = call(L, "voxel_points", cloud=None)
    assert rc != 0 and "cloud=NULL" in msg and "together" in msg, msg


@pytest.mark.parametrize("who,name,align", [("voxel_surface", n, 4) for n in ("verts", "faces", "vert_offset", "face_offset", "depth_maps",
                                                                             "counts")] +
                         [("voxel_depth_maps", "depth_maps", 4), ("voxel_points", "surface", 4), ("voxel_points", "aligned", 4),
                          ("voxel_points", "cloud", 4), ("voxel_points", "index", 8)])
def test_alignment(L, who, name, align):
    for off in (1, 2) + ((4,) if align == 8 else ()):
        rc, msg = call(L, who, **{name: CALLS[who][0][name] + off})
        assert rc != 0 and who in msg and f"{name}=0x" in msg and f"{align}-byte aligned" in msg, (name, off, msg)


def test_empty_tables_need_no_pointer(L):
    """``verts`` may be NULL when V == 0, ``faces`` when F == 0, ``surface`` when total == 0: such a call gets past those (and is
    refused here for a reason of its own, so that nothing is launched)."""
    rc, msg = call(L, "voxel_surface", verts=None, V=0, faces=None, F=0, counts=None)
    assert rc != 0 and "counts=NULL" in msg, msg
    rc, msg = call(L, "voxel_points", surface=None, total=0, index=None)
    assert rc != 0 and "index=NULL" in msg, msg


def test_the_voxeliser_is_in_the_build():
    from a3vt_amd import lib
    assert "voxel.hip" in lib.SOURCES and "-ffp-contract=off" in lib.EXTRA_FLAGS["voxel.hip"]
    for who, (_, order) in CALLS.items():
        assert len(lib.SIGNATURES["a3vt_" + who][1]) == len(order)
    assert "a3vt_voxel_launches" in lib.SIGNATURES
