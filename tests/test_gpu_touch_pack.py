"""GPU tests of ``ops.touch_pack`` (``a3vt_touch_pack``, csrc/touch_pack.hip) on synthetic ``touch`` / ``points`` / ``count`` /
``status`` tensors — no rendering but in the last test.  Every expected value is NumPy slicing on the host; everything is compared
bit for bit (the points as uint32, so NaN payloads count).

The sizes I = 1, 2, 65, 257, 1030 cross a wave and a workgroup of the prefix sum and the kernel's ways of slicing a view's rows
(16 chunks per view at 1, 2 and 65 views, 7 at 257, 1 at 1 030).  Above 2 048 views a workgroup owns a span of views, which
``test_a_span_of_views`` reaches with small counts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PIX = 121 * 121
SENTINEL = 0x7FC12345            # a NaN with a payload: no input below holds it
EDGE_COUNTS = (0, 1, 2, PIX - 1, PIX)


def inputs(I, seed, big=None, with_touch=True):
    """Host arrays: counts from the edge values plus random ones (``big``: how many views may be large; the rest stay <= 64),
    random status in {0, 1} (and a few other values, which are not "touch"), points as random bit patterns, a small random image."""
    g = np.random.default_rng(seed)
    count = g.choice(np.array(EDGE_COUNTS + tuple(g.integers(3, PIX, 3))), I)
    if big is not None:
        small = g.choice(np.array((0, 1, 2, 7, 63, 64)), I)
        keep = np.zeros(I, bool)
        keep[g.choice(I, min(big, I), replace=False)] = True
        count = np.where(keep, count, small)
    status = g.choice(np.array((0, 1, 1, 1, 2, -1)), I)
    if I >= 4:
        status[g.choice(I, 2, replace=False)] = 1             # at least two views are kept whatever the draw
    # (cheap to make at I = 1030, 180 MB each: a multiplicative hash of the index, no two neighbours alike; a random image repeated)
    points = ((np.arange(I * PIX * 3, dtype=np.uint32) + np.uint32(seed)) * np.uint32(2654435761)).reshape(I, PIX, 3)
    touch = np.resize(g.random(min(I, 3) * PIX * 3 + 17, dtype=np.float32) * np.float32(255), (I, 121, 121, 3)) if with_touch else None
    return dict(count=count.astype(np.int32), status=status.astype(np.int32), points=points, touch=touch)


def expected(host):
    n = np.where(host["status"] == 1, host["count"], 0).astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(n)))
    rows = [host["points"][i, :n[i]] for i in range(len(n))]
    return offsets.astype(np.int32), np.concatenate(rows) if rows else np.zeros((0, 3), np.uint32)


def on_device(host, cuda):
    out = {"count": torch.from_numpy(host["count"]).to(cuda), "status": torch.from_numpy(host["status"]).to(cuda),
           "points": torch.from_numpy(host["points"].view(np.int32)).to(cuda).view(torch.float32)}
    if host["touch"] is not None:
        out["touch"] = torch.from_numpy(host["touch"]).to(cuda)
    return out


def run(out, capacity, want_touch):
    """One launch into a sentinel-filled cloud of ``capacity`` rows -> (offsets, cloud as uint32, touch_u8 or None) on the host."""
    from a3vt_amd import ops
    I = out["status"].shape[0]
    cloud = torch.full((capacity, 3), SENTINEL, dtype=torch.int32, device=out["status"].device).view(torch.float32)
    offsets = torch.full((I + 1,), -7, dtype=torch.int32, device=cloud.device)
    small = torch.full((I, 121, 121, 3), 99, dtype=torch.uint8, device=cloud.device) if want_touch else None
    got = ops._touch_pack_into(out["touch"] if want_touch else None, out["points"], out["count"], out["status"], I, small, offsets, cloud,
                               bounded=False)
    assert got["cloud"] is cloud and got["offsets"] is offsets
    return offsets.cpu().numpy(), cloud.view(torch.int32).cpu().numpy().view(np.uint32), None if small is None else small.cpu().numpy()


@pytest.mark.parametrize("I,big", [(1, None), (2, None), (65, 6), (257, 5), (1030, 4)])
def test_offsets_rows_images_and_the_rows_beyond(cuda, I, big):
    from a3vt_amd import ops
    for seed in ((0, 1, 2) if I <= 2 else (0,)):                              # (I = 1, 2: a kept, a dropped and an empty view turn up)
        host = inputs(I, 100 * I + seed, big)
        want_offsets, want_rows = expected(host)
        total = int(want_offsets[-1])
        out = on_device(host, cuda)
        ops.touch_pack_launches(reset=True)
        offsets, cloud, small = run(out, total + 5, want_touch=True)
        assert ops.touch_pack_launches() == {"calls": 1}
        print(f"I={I} seed={seed}: {total} rows of {int(np.where(host['status'] == 1, 1, 0).sum())} kept views")
        assert np.array_equal(offsets, want_offsets)
        assert np.array_equal(cloud[:total], want_rows)
        assert (cloud[total:] == SENTINEL).all()                             # rows from offsets[I] on are not written
        assert np.array_equal(small, host["touch"].astype(np.uint8))         # in-range values: NumPy's own truncation
        again = run(out, total + 5, want_touch=True)                         # two calls give equal bits
        assert np.array_equal(again[0], offsets) and np.array_equal(again[1], cloud) and np.array_equal(again[2], small)
    assert I <= 2 or (np.diff(want_offsets) == 0).any() and (host["count"][host["status"] != 1] > 0).any()   # dropped views with points


def test_a_span_of_views(cuda):
    """Above 2 048 views a workgroup owns several views: 2 101 views (spans of 2, the last one short) with counts <= 64 but four."""
    host = inputs(2101, 7, big=4, with_touch=False)
    want_offsets, want_rows = expected(host)
    total = int(want_offsets[-1])
    offsets, cloud, _ = run(on_device(host, cuda), total + 3, want_touch=False)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(cloud[:total], want_rows) and (cloud[total:] == SENTINEL).all()


def test_the_truncation_rule(cuda):
    """Clamp to [0, 255], then toward zero; NaN gives 0 — on a plane that holds the edge values at every position of a 16-byte
    group and in the scalar tail (I * 43 923 = 3 mod 4 for I = 1)."""
    from a3vt_amd import ops
    values = np.array([0.0, 0.5, 0.99999994, 1.0, 127.5, 254.99998, 255.0, -0.0, 300.0, -3.0, np.nan, np.inf, -np.inf, 1e-40, 255.00002],
                      np.float32)
    want = np.array([0, 0, 0, 1, 127, 254, 255, 0, 255, 0, 0, 255, 0, 0, 255], np.uint8)
    touch = np.resize(values, 121 * 121 * 3).reshape(1, 121, 121, 3)           # 15 values: every value meets every lane position
    touch[0, -1, -1] = (np.nan, 254.99998, 300.0)                              # the last three floats: the scalar tail
    want_plane = np.resize(want, 121 * 121 * 3).reshape(1, 121, 121, 3)
    want_plane[0, -1, -1] = (0, 254, 255)
    out = {"touch": torch.from_numpy(touch).to(cuda), "status": torch.zeros(1, dtype=torch.int32, device=cuda)}
    got = ops.touch_pack(out, want_touch=True, want_points=False)
    assert set(got) == {"touch_u8"} and got["touch_u8"].dtype == torch.uint8 and got["touch_u8"].shape == (1, 121, 121, 3)
    assert np.array_equal(got["touch_u8"].cpu().numpy(), want_plane)
    in_range = np.isfinite(touch) & (touch >= 0) & (touch <= 255)
    assert np.array_equal(want_plane[in_range], touch[in_range].astype(np.uint8))            # NumPy's .astype, where it is defined
    assert torch.equal(got["touch_u8"][torch.from_numpy(in_range)], out["touch"].to(torch.uint8)[torch.from_numpy(in_range)])
    off = torch.zeros(121 * 121 * 3 + 1, device=cuda)[1:].view(1, 121, 121, 3)               # a view 4 bytes off a 16-byte boundary
    off.copy_(out["touch"])
    assert off.data_ptr() % 16 == 4
    assert torch.equal(ops.touch_pack({"touch": off, "status": out["status"]}, want_points=False)["touch_u8"], got["touch_u8"])


def test_all_counts_zero_and_all_views_dropped(cuda):
    host = inputs(65, 3, with_touch=False)
    for change in (dict(count=np.zeros(65, np.int32)), dict(status=np.zeros(65, np.int32))):
        offsets, cloud, _ = run(on_device(dict(host, **change), cuda), 4, want_touch=False)
        assert not offsets.any() and (cloud == SENTINEL).all()


def test_a_capacity_one_row_short(cuda):
    from a3vt_amd import ops
    host = inputs(65, 11, big=6, with_touch=False)
    want_offsets, want_rows = expected(host)
    total = int(want_offsets[-1])
    out = on_device(host, cuda)
    offsets, cloud, _ = run(out, total - 1, want_touch=False)
    assert np.array_equal(offsets, want_offsets) and (cloud == SENTINEL).all()                # offsets complete, no row written
    with pytest.raises(RuntimeError, match=f"{total} contact points.*capacity={total - 1}"):
        ops.touch_pack(out, want_touch=False, capacity=total - 1)
    exact = ops.touch_pack(out, want_touch=False, capacity=total)                            # the bound itself is enough
    assert set(exact) == {"offsets", "cloud"} and exact["cloud"].shape == (total, 3)
    assert np.array_equal(exact["cloud"].view(torch.int32).cpu().numpy().view(np.uint32), want_rows)
    unbounded = ops.touch_pack(out, want_touch=False)
    assert unbounded["cloud"].shape == (65 * PIX, 3) and torch.equal(unbounded["offsets"], exact["offsets"])
    assert torch.equal(unbounded["cloud"][:total].view(torch.int32), exact["cloud"].view(torch.int32))


def test_counts_the_renderer_cannot_produce_stay_in_bounds(cuda):
    """A count outside 0..14 641 is clamped into it: no read outside the view's points, and the capacity rule holds."""
    host = inputs(5, 13, with_touch=False)
    host["count"][:] = (PIX + 1, -5, 1 << 30, 3, -(1 << 31))
    host["status"][:] = 1
    clamped = dict(host, count=np.clip(host["count"], 0, PIX))
    want_offsets, want_rows = expected(clamped)
    offsets, cloud, _ = run(on_device(host, cuda), int(want_offsets[-1]) + 2, want_touch=False)
    assert np.array_equal(offsets, want_offsets) and np.array_equal(cloud[:-2], want_rows) and (cloud[-2:] == SENTINEL).all()


def test_wrapper_refusals(cuda):
    from a3vt_amd import ops
    out = on_device(inputs(2, 5), cuda)
    with pytest.raises(ValueError, match="neither"):
        ops.touch_pack(out, want_touch=False, want_points=False)
    with pytest.raises(ValueError, match="without want_points"):
        ops.touch_pack({k: v for k, v in out.items() if k != "points"})
    with pytest.raises(ValueError, match="without want_touch"):
        ops.touch_pack({k: v for k, v in out.items() if k != "touch"})
    with pytest.raises(ValueError, match="touch_pack wants points"):
        ops.touch_pack(dict(out, points=out["points"][:, :100].contiguous()))
    with pytest.raises(ValueError, match="negative"):
        ops.touch_pack(out, capacity=-1)


def test_through_the_renderer(cuda):
    """``ops.touch_render`` on the bake scene's live views, then the pack, against per-view slicing of the render's own buffers."""
    from chart_head_util import bake_scene
    from a3vt_amd import ops
    from a3vt_amd.pterotactyl.policies import rendered
    geometry, frames = bake_scene()
    calls = []

    def keeping(*a, **k):
        calls.append(ops.touch_render(*a, **k))
        return calls[-1]
    sampler = rendered.RenderedSampler(frames, geometry, to_host=False, render=keeping, device=cuda, pack=ops.touch_pack)
    sampler.load_objects(["/data/object_info/ball", "/data/object_info/pebble"])
    sampler.sample([0, 1], touch_point_cloud=True)
    out = calls[0]
    I = out["status"].shape[0]
    assert I == 7                                                              # four fingers of ("ball", 0), three of ("pebble", 1)
    got = ops.touch_pack(out)
    count, status = out["count"].cpu().numpy(), out["status"].cpu().numpy()
    n = np.where(status == 1, count, 0)
    assert (n > 0).sum() >= 5 and (status == 0).any()                          # finger 2 of action 0 looks away
    offsets = got["offsets"].cpu().numpy()
    assert np.array_equal(offsets, np.concatenate(([0], np.cumsum(n))))
    for i in range(I):
        assert torch.equal(got["cloud"][offsets[i]:offsets[i + 1]].view(torch.int32), out["points"][i, :n[i]].view(torch.int32)), i
    assert torch.equal(got["touch_u8"], out["touch"].to(torch.uint8))
