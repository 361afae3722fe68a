#!/usr/bin/env python
"""Generate ``g23_touch_render.npz`` by running the REAL reference's ``Scene.render_depth`` (for the statuses),
``Scene.depth_to_touch`` and ``Scene.depth_to_points`` on the CPU on prepared float32 depth maps
(``python tests/golden/make_golden_touch_render.py``, build container only; see ``make_golden.py`` and ``oracle.ref_shim``).

The three methods are called unbound on a stand-in ``self`` whose ``touch_renderer`` hands out the prepared maps instead of
rendering and whose ``get_pose`` returns the scenes' finger frame: nothing of pybullet or pyrender runs.  The maps
(``touch_render_util``): the fp64 emulation's ray-cast depth of the scenes in ``CAST_MAPS``, rounded to float32, and the hand-made
``HAND_MAPS``.  Stored:
  names                 the maps' names, in order
  depth                 (n, 121, 121) float32, the inputs
  pos, rot, euler       the finger frame (float64; ``rot`` is SciPy's matrix of ``euler``, what ``*_ref_frame.npy`` stores)
  status                (n,) int8, 1 = "touch"
  touch                 (n, len(ROWS), 121, 3) float64: rows ``touch_render_util.ROWS`` of ``depth_to_touch`` (the first and last
                        8 rows, every third between; every column of each)
  count, points         (n,) int32, the clouds' sizes, and the concatenated float64 clouds of ``depth_to_points`` in the reference's
                        order, of each the points ``touch_render_util.stored_points(count)``"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save  # noqa: E402  (installs the import shim; defines no fixture when imported)
import touch_render_ref as tr  # noqa: E402
import touch_render_util as tu  # noqa: E402


class Handout:
    """The stand-in ``touch_renderer``: ``render`` returns the next prepared map."""

    def __init__(self, maps):
        self.maps = list(maps)

    def update_camera_pose(self, position, orientation):
        pass

    def render(self):
        return self.maps.pop(0).copy()


def main():
    from scipy.spatial.transform import Rotation
    scene_module = importlib.import_module("pterotactyl.simulator.scene.instance")
    Scene = scene_module.Scene
    names = list(tu.CAST_MAPS) + list(tu.HAND_MAPS)
    maps = [tr.cast(*tu.scene(n), tu.POS, tu.ROT)[0].astype(np.float32) for n in tu.CAST_MAPS] + [tu.hand_map(n) for n in tu.HAND_MAPS]
    rot = Rotation.from_euler("xyz", tu.EULER, degrees=False).as_matrix()
    assert np.abs(rot - tu.ROT).max() < 1e-15
    status, touch, count, points = [], [], [], []
    for g0 in range(0, len(maps), 4):                       # the reference handles four fingers at a time
        group = maps[g0:g0 + 4]
        group = group + [np.zeros_like(maps[0])] * (4 - len(group))
        me = SimpleNamespace(max_depth=tr.MAX_DEPTH, TACTO=False, hand=0, touch_cameras=[6, 13, 20, 27],
                             touch_renderer=Handout(group), get_pose=lambda obj, link: (tuple(tu.POS), tuple(tu.EULER)))
        st = Scene.render_depth(me)
        clouds = Scene.depth_to_points(me)
        for i in range(min(4, len(maps) - g0)):
            status.append(st[i] == "touch")
            touch.append(Scene.depth_to_touch(me, group[i].copy())[tu.ROWS])
            cloud = np.asarray(clouds[i], np.float64).reshape(-1, 3)
            count.append(len(cloud))
            points.append(cloud[tu.stored_points(len(cloud))])
    for n, s, c in zip(names, status, count):
        print(f"{n}: status {int(s)}, {c} points")
    save(tu.FIXTURE, names=np.array(names), depth=np.stack(maps), pos=tu.POS, rot=rot, euler=np.array(tu.EULER),
         status=np.array(status, np.int8), touch=np.stack(touch), count=np.array(count, np.int32), points=np.concatenate(points))


if __name__ == "__main__":
    main()
