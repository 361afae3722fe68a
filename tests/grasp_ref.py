"""The tests' own float64 statement of the closing rule of ``a3vt_grasp_close`` (``include/a3vt.h``), loop by loop: test
infrastructure, independent of ``ops.grasp_close``'s vectorised host path and of ``HandModel.table()`` (it reads the model's arrays).

``close(...)`` walks steps, joints and boxes in Python loops exactly as the rule is worded (a joint's angle grows by ``q + delta``
per accepted step) and takes only the triangles of one box at a time through NumPy.  Beside the rule's outputs it returns every
query's SIGNED SEPARATION: per (box, triangle) pair the largest gap over the 13 axes, each normalised to unit length (negative: the
depth by which the pair penetrates along its shallowest axis), then the smallest over the pairs.  A pair overlaps iff its separation
is <= 0 (touching counts).  ``margin[g, c]`` is the smallest |separation| over the queries of grasp g, finger c: the pair
(g, c) is *decided* for a float32 implementation when ``margin >= DECIDED`` (1e-5 m).

Pairs whose world-axis bounding boxes are more than ``FAR`` (1 mm) apart are not tested: they are separated by at least 1 mm, their
13-axis separation is then at least 1 mm / sqrt(3), far above ``DECIDED``, so they can change neither a boolean nor a verdict.

Also here: the meshes and placements the grasp tests share."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DECIDED = 1e-5
FAR = 1e-3
MIN_AXIS2 = 1e-24


def hand():
    from a3vt_amd.pterotactyl.simulator.hand import HandModel
    return HandModel.load(os.path.join(GOLDEN, "allegro_hand.npz"))


def _rpy(r, p, y):
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return rz @ ry @ rx


def _turn(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def chain_poses(model, c, base_pos, base_rot, angles):
    """World poses of chain c's links for the chain's 7 ``angles`` (fixed joints ignore theirs)."""
    n = model.chain
    pos, rot = [None] * n, [None] * n
    for k in range(n):
        i = c * n + k
        parent = int(model.parent[i])
        p, R = (base_pos, base_rot) if parent < 0 else (pos[parent - c * n], rot[parent - c * n])
        pos[k] = p + R @ model.origin_xyz[i]
        rot[k] = R @ _rpy(*model.origin_rpy[i])
        if model.revolute[i]:
            rot[k] = rot[k] @ _turn(model.axis[i], angles[k])
    return pos, rot


def pair_separation(centre, R, half, tri):
    """(n,) signed separations of one box against the triangles (n, 3, 3)."""
    p = (tri - centre) @ R                                         # rows: R^T (v - c)
    best = np.full(len(tri), -np.inf)
    for i in range(3):                                             # the box's axes
        best = np.maximum(best, np.maximum(p[:, :, i].min(axis=1) - half[i], -p[:, :, i].max(axis=1) - half[i]))
    edges = [p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]]
    axes = [np.cross(edges[0], edges[1])]
    for e in edges:
        for u in np.eye(3):
            axes.append(np.cross(u, e))
    for a in axes:
        length2 = (a * a).sum(-1)
        use = length2 >= MIN_AXIS2
        d = np.einsum("ni,nki->nk", a, p)
        r = np.abs(a) @ half
        with np.errstate(divide="ignore", invalid="ignore"):
            gap = np.maximum(d.min(axis=1) - r, -d.max(axis=1) - r) / np.sqrt(length2)
        best = np.where(use, np.maximum(best, gap), best)
    return best


def close(verts, faces, face_offset, grasp_mesh, base_pos, base_rot, model, steps, near_faces=None):
    """-> ``q`` (G, 16), ``blocked_step`` (G, 16) int, ``margin`` (G, 4), ``link_pos`` (G, 28, 3), ``link_rot`` (G, 28, 3, 3).
    ``near_faces``: a set that receives the global index of every face that came within ``FAR`` of a box in any query (the
    faces outside it can be taken out of the mesh without changing any query's verdict)."""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    G, n = len(grasp_mesh), model.chain
    q_out, blocked, margin = np.zeros((G, 16)), np.zeros((G, 16), np.int64), np.full((G, 4), np.inf)
    link_pos, link_rot = np.zeros((G, 4 * n, 3)), np.zeros((G, 4 * n, 3, 3))
    for g in range(G):
        m = int(grasp_mesh[g])
        f = faces[int(face_offset[m]):int(face_offset[m + 1])]
        tri = verts[f].reshape(-1, 3, 3)
        lo, hi = tri.min(axis=1), tri.max(axis=1)
        bp, br = np.asarray(base_pos[g], np.float64), np.asarray(base_rot[g], np.float64).reshape(3, 3)
        for c in range(4):
            joints = [k for k in range(n) if model.revolute[c * n + k]]
            q = np.array(model.q0[c * n:(c + 1) * n], np.float64)
            delta = {j: (model.upper[c * n + j] - q[j]) / steps for j in joints}
            frozen, took = set(), {j: steps for j in joints}
            for step in range(1, steps + 1):
                for j in joints:
                    if j in frozen:
                        continue
                    tentative = q.copy()
                    tentative[j] = q[j] + delta[j]
                    pos, rot = chain_poses(model, c, bp, br, tentative)
                    separation = np.inf
                    for k in range(j, n):                           # link j and every link distal to it
                        i = c * n + k
                        if not model.has_box[i] or len(tri) == 0:
                            continue
                        centre = pos[k] + rot[k] @ model.box_centre[i]
                        extent = np.abs(rot[k]) @ model.box_half[i]
                        near = (np.maximum(lo - (centre + extent), (centre - extent) - hi).max(axis=1) < FAR)
                        if near_faces is not None:
                            near_faces.update((int(face_offset[m]) + np.flatnonzero(near)).tolist())
                        if near.any():
                            separation = min(separation, pair_separation(centre, rot[k], model.box_half[i], tri[near]).min())
                    margin[g, c] = min(margin[g, c], abs(separation))
                    if separation <= 0:
                        frozen.add(j)
                        took[j] = step - 1
                    else:
                        q = tentative
            pos, rot = chain_poses(model, c, bp, br, q)
            q_out[g, 4 * c:4 * c + 4] = [q[j] for j in joints]
            blocked[g, 4 * c:4 * c + 4] = [took[j] for j in joints]
            link_pos[g, c * n:(c + 1) * n], link_rot[g, c * n:(c + 1) * n] = np.array(pos), np.array(rot)
    return q_out, blocked, margin, link_pos, link_rot


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------
def icosphere(level, radius=0.08, scale=(1.0, 1.0, 1.0), centre=(0.0, 0.0, 0.0)):
    from a3vt_amd import mesh as amesh
    v, f = amesh.icosphere(level)
    v = np.asarray(v, np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * radius * np.asarray(scale) + np.asarray(centre)
    return v.astype(np.float32), np.asarray(f, np.int64)


def box_mesh(half=(0.05, 0.04, 0.03)):
    """A 12-face box about the origin."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * np.asarray(half)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int64)
    return v.astype(np.float32), f


def blocking_triangle(model, c, fraction, base_pos=(0.0, 0.0, 0.0), base_rot=np.eye(3), size=0.012):
    """One triangle (verts (3, 3) float32, faces (1, 3)) through the centre of chain c's tip box at the pose where the chain's four
    joints have all gone ``fraction`` of their way from ``q0`` to their upper limits: it lies in that finger's path."""
    n = model.chain
    q = np.array(model.q0[c * n:(c + 1) * n], np.float64)
    q[:4] += fraction * (model.upper[c * n:c * n + 4] - q[:4])
    pos, rot = chain_poses(model, c, np.asarray(base_pos, np.float64), np.asarray(base_rot, np.float64), q)
    tip = c * n + 4
    centre = pos[4] + rot[4] @ model.box_centre[tip]
    offsets = np.array([[1.0, 0.2, -0.3], [-0.6, 0.9, 0.25], [-0.4, -0.8, 0.5]]) * size
    return (centre + offsets @ rot[4].T).astype(np.float32), np.array([[0, 1, 2]], np.int64)


def batch(meshes):
    """``[(verts, faces), ...]`` -> verts, faces (global indices), face_offset."""
    verts, faces, offsets, base = [], [], [0], 0
    for v, f in meshes:
        verts.append(np.asarray(v, np.float32).reshape(-1, 3))
        faces.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += len(verts[-1])
        offsets.append(offsets[-1] + len(faces[-1]))
    return np.concatenate(verts), np.concatenate(faces), offsets


def placements(meshes, picks, num_actions=50):
    """``picks``: (mesh, action) pairs -> grasp_mesh, base_pos (G, 3), base_rot (G, 3, 3) float32 of those that can be placed."""
    from a3vt_amd.pterotactyl.simulator.physics.grasping import place_hand
    which, pos, rot = [], [], []
    for m, a in picks:
        pose = place_hand(meshes[m][0], a, num_actions)
        if pose is not None:
            which.append(m)
            pos.append(pose[0])
            rot.append(pose[1])
    return which, np.array(pos, np.float32).reshape(-1, 3), np.array(rot, np.float32).reshape(-1, 3, 3)
