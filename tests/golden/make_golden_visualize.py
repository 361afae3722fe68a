#!/usr/bin/env python
"""Generate ``g25_visualize.npz``: what the REFERENCE's visualisation helpers of ``utility/utils.py`` give, run on the CPU through
``oracle.ref_shim``.

Run in the build container only:  ``python tests/golden/make_golden_visualize.py``  (a second).  The file holds
  ``circle<n>``            ``get_circle(n).points`` fp32 (n, 3), for every n of ``circle_sizes`` the reference accepts
  ``circle_sizes``, ``circle_exits``   the sizes asked for, and 1 where the reference printed its mismatch and called ``exit()``
                           (10 is one: its rings hold 3 + 5 + 3 = 11 points) — ``circle<n>`` is absent there
  ``faces7``, ``faces7_added``         a 7-face table and ``add_faces`` of it
  ``pose_camera``          ``euler2matrix`` for the render camera (xyz, [45, 0, 180] degrees, at [0, 0.6, 0.6]), fp64 (4, 4)
  ``pose_lights``          the same for the four lights' poses (zero angles, radians), fp64 (4, 4, 4)
  ``pose_general``, ``pose_general_angles``   one pose of three non-trivial angles in radians, and those angles
  ``actions``, ``num_actions``, ``projection``   a fixed action list and ``visualize_actions``' ``sphere_projection.png`` for it
                           with ``use_img=False``, read back as the uint8 array that was written
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

ref = ref_shim.load_reference()
assert ref is not None, "needs the reference"

CIRCLE_SIZES = (10, 12, 50)
ACTIONS = [3, 3, 17, 49, 0, 21, 21, 21, 8, 30, 44, 12, 3]
GENERAL = [0.3, -0.7, 1.1]
LIGHTS = ([0, -0.8, 0.3], [0, 0.8, 0.3], [-1, 0, 1], [1, 0, 1])


def main():
    from PIL import Image
    out = {"circle_sizes": np.array(CIRCLE_SIZES, np.int32)}
    exits = []
    for n in CIRCLE_SIZES:
        try:
            out[f"circle{n}"] = ref.utils.get_circle(n).points.numpy().astype(np.float32)
            exits.append(0)
        except SystemExit:
            exits.append(1)
    out["circle_exits"] = np.array(exits, np.int32)
    faces7 = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 2], [5, 6, 7], [7, 6, 0], [3, 5, 1], [8, 2, 6]], np.int64)
    out.update(faces7=faces7, faces7_added=ref.utils.add_faces(faces7))
    out["pose_camera"] = ref.utils.euler2matrix(xyz="xyz", angles=[45.0, 0, 180.0], translation=[0, 0.6, 0.6], degrees=True)
    out["pose_lights"] = np.stack([ref.utils.euler2matrix(angles=[0, 0, 0], translation=t, xyz="xyz", degrees=False) for t in LIGHTS])
    out["pose_general"] = ref.utils.euler2matrix(angles=GENERAL, translation=[0.1, -0.2, 0.3])
    out["pose_general_angles"] = np.array(GENERAL)
    args = SimpleNamespace(num_actions=50, use_img=False)
    with tempfile.TemporaryDirectory() as tmp:
        ref.utils.visualize_actions(tmp, torch.tensor(ACTIONS), args)
        out["projection"] = np.array(Image.open(os.path.join(tmp, "sphere_projection.png")))
    out.update(actions=np.array(ACTIONS, np.int32), num_actions=np.int32(50))
    path = os.path.join(HERE, "g25_visualize.npz")
    np.savez_compressed(path, **out)
    print(f"g25_visualize.npz: {os.path.getsize(path) / 1024:.1f} KiB; get_circle exits at {[n for n, e in zip(CIRCLE_SIZES, exits) if e]}; "
          f"projection {out['projection'].shape} {out['projection'].dtype}")


if __name__ == "__main__":
    main()
