#!/usr/bin/env python
"""Generate ``allegro_hand_visual.npz``: the NUMBERS of the hand's visual meshes (the reference's ``objects/hand/meshes_obj/*.obj``),
read through this package's own ``HandVisual.load`` and stored by ``HandVisual.save``
(``python tests/golden/make_golden_hand_visual.py [path/to/meshes_obj]``; build container only).

Stored: per distinct part (``0_base`` .. ``9_thumb``) the float32 vertices and int32 faces, and the node table (part, link row, RGB)
of the reference's 21 hand nodes.  Arrays only — no program text; the OBJ and MTL files themselves are not committed.  The posed-render
tests load this file; ``test_posed_render_host.py`` compares it with a live load where the reference is present."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    import a3vt_amd  # noqa: F401
    from oracle.ref_shim import REFERENCE_ROOT
    from a3vt_amd.pterotactyl.simulator.hand import VISUAL_PARTS, HandVisual
    folder = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REFERENCE_ROOT, "pterotactyl", "objects", "hand", "meshes_obj")
    visual = HandVisual.load(folder)
    out = os.path.join(HERE, "allegro_hand_visual.npz")
    visual.save(out)
    print(f"{out}: {len(visual.parts)} parts, {len(visual.nodes)} nodes, {visual.num_faces} faces drawn, {os.path.getsize(out)} bytes")
    for name, (v, f) in zip(VISUAL_PARTS, visual.parts):
        print(name, len(v), "vertices", len(f), "faces", v.min(axis=0).round(4), v.max(axis=0).round(4))


if __name__ == "__main__":
    main()
