#!/usr/bin/env python
"""Generate ``allegro_hand.npz``: the NUMBERS of the reference's Allegro hand (``objects/hand/allegro_hand.urdf`` and the binary STL
collision meshes beside it), read through this package's own ``HandModel.load`` and stored by ``HandModel.save``
(``python tests/golden/make_golden_hand.py [path/to/allegro_hand.urdf]``; build container only).

Stored (one row per link, the base excluded, in ``HandModel``'s depth-first order): ``names``, ``parent``, ``origin_xyz``,
``origin_rpy``, ``axis``, ``revolute``, ``lower``, ``upper``, ``has_box``, ``box_centre``, ``box_half`` and the rest pose ``q0``.  No
program text, no mesh: the URDF, STL and OBJ files themselves are not committed.  The GPU tests and the ``save_simulation`` tests load
this file; ``test_grasp_host.py`` compares it with a live parse where the reference is present."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    import a3vt_amd  # noqa: F401
    from oracle.ref_shim import REFERENCE_ROOT
    DEFAULT_URDF = os.path.join(REFERENCE_ROOT, "pterotactyl", "objects", "hand", "allegro_hand.urdf")
    from a3vt_amd.pterotactyl.simulator.hand import HandModel
    urdf = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_URDF
    hand = HandModel.load(urdf)
    out = os.path.join(HERE, "allegro_hand.npz")
    hand.save(out)
    print(f"{out}: {hand.num_links} links, {int(hand.has_box.sum())} boxes, {os.path.getsize(out)} bytes")
    for i in range(hand.num_links):
        print(i, hand.names[i], int(hand.parent[i]), bool(hand.revolute[i]), hand.box_centre[i].round(4), hand.box_half[i].round(4))


if __name__ == "__main__":
    main()
