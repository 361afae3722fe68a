"""An exact host emulation of the ground-truth point-cloud pipeline (``a3vt_voxel_surface`` / ``a3vt_voxel_points``), written in
NumPy from the contract in ``include/a3vt.h`` and independent of ``ops.py``'s CPU path: where no fixture of the reference exists,
the GPU tests compare against this, bit for bit.  Every fp32 step is one NumPy operation on float32 operands, so each is rounded on
its own, as the contract demands."""
import numpy as np

F32 = np.float32
MAX_DEPTH = 12          # a sub-triangle of this depth is never split


def normalise(verts):
    """(v - lo) / (hi - lo) - 0.5 with lo / hi over the finite coordinates; NaN rows where that cannot be formed."""
    verts = np.asarray(verts, dtype=F32).reshape(-1, 3)
    flat = verts.ravel()
    flat = flat[np.isfinite(flat)]
    if flat.size == 0:
        return np.full(verts.shape, np.nan, dtype=F32)
    lo, hi = flat.min(), flat.max()
    with np.errstate(all="ignore"):
        return np.subtract(np.divide(np.subtract(verts, lo), np.subtract(hi, lo)), F32(0.5))


def occupied(verts, faces, dim):
    """Sorted (n, 3) int64 voxel coordinates the subdivision of every face marks."""
    norm = normalise(verts)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tri = [norm[f] for f in faces if (f >= 0).all() and (f < norm.shape[0]).all() and np.isfinite(norm[f]).all()]
    tri = np.asarray(tri, dtype=F32).reshape(-1, 3, 3)            # [triangle][corner][axis]
    thr = F32((1.0 / dim) ** 2)
    marked = set()

    def mark(points):
        scaled = np.multiply(np.add(points.reshape(-1, 3), F32(0.5)), F32(dim - 1))
        cell = np.trunc(scaled).astype(np.int64)
        good = ((cell >= 0) & (cell < dim)).all(axis=1)
        marked.update(np.unique((cell[good, 0] * dim + cell[good, 1]) * dim + cell[good, 2]).tolist())

    def longest(t):
        worst = np.zeros(t.shape[0], dtype=F32)
        for p, q in ((0, 1), (1, 2), (2, 0)):
            sq = np.square(np.subtract(t[:, p], t[:, q]))
            worst = np.maximum(worst, np.add(np.add(sq[:, 0], sq[:, 1]), sq[:, 2]))
        return worst

    mark(tri)
    for _ in range(MAX_DEPTH):
        tri = tri[longest(tri) > thr]
        if tri.shape[0] == 0:
            break
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ac = np.divide(np.add(a, b), F32(2)), np.divide(np.add(b, c), F32(2)), np.divide(np.add(a, c), F32(2))
        mark(np.stack((ab, bc, ac)))
        tri = np.concatenate([np.stack(t, axis=1) for t in ((a, ac, ab), (ab, b, bc), (ab, ac, bc), (ac, c, bc))])
    flat = np.array(sorted(marked), dtype=np.int64)
    return np.stack((flat // (dim * dim), flat // dim % dim, flat % dim), axis=1).reshape(-1, 3)


def depth_maps(cells, dim):
    """The six maps (6, dim, dim) int64 of a list of occupied cells: walk the cells, keep first and last per column."""
    first = np.full((3, dim, dim), dim, dtype=np.int64)
    last = np.full((3, dim, dim), -1, dtype=np.int64)
    for i, j, k in np.asarray(cells, dtype=np.int64).reshape(-1, 3):
        for axis, (p, q, x) in enumerate(((i, j, k), (i, k, j), (j, k, i))):
            first[axis, p, q] = min(first[axis, p, q], x)
            last[axis, p, q] = max(last[axis, p, q], x)
    odm = np.empty((6, dim, dim), dtype=np.int64)
    odm[0::2] = np.where(last >= 0, dim - 1 - last, dim)
    odm[1::2] = first
    return odm


def carve(odm):
    """The kept grid, bool (dim, dim, dim): inside the column's interval along every axis."""
    dim = odm.shape[1]
    i, j, k = np.indices((dim, dim, dim))
    return ((odm[1][i, j] <= k) & (k <= dim - 1 - odm[0][i, j]) & (odm[3][i, k] <= j) & (j <= dim - 1 - odm[2][i, k]) &
            (odm[5][j, k] <= i) & (i <= dim - 1 - odm[4][j, k]))


def surface(kept):
    """Kept cells with fewer than 27 kept cells in their 3 x 3 x 3 neighbourhood, (n, 3) int64 in lexicographic order."""
    dim = kept.shape[0]
    padded = np.zeros((dim + 2,) * 3, dtype=np.int64)
    padded[1:-1, 1:-1, 1:-1] = kept
    around = np.zeros((dim,) * 3, dtype=np.int64)
    for di in range(3):
        for dj in range(3):
            for dk in range(3):
                around += padded[di:di + dim, dj:dj + dim, dk:dk + dim]
    return np.argwhere(kept & (around < 27))


def realign(cells, verts):
    """fp32 (n, 3): per axis centre on (max + min) / 2, divide by the centred values' max + 1 - min, times the vertices' extent."""
    cells = np.asarray(cells).reshape(-1, 3)
    verts = np.asarray(verts, dtype=F32).reshape(-1, 3)
    out = np.zeros(cells.shape, dtype=F32)
    if cells.shape[0] == 0:
        return out
    for axis in range(3):
        x = cells[:, axis].astype(F32)
        centred = np.subtract(x, np.divide(np.add(x.max(), x.min()), F32(2)))
        extent = np.subtract(np.add(centred.max(), F32(1)), centred.min())
        col = verts[:, axis][np.isfinite(verts[:, axis])]
        with np.errstate(all="ignore"):
            spread = np.subtract(col.max(), col.min()) if col.size else F32(np.nan)
            out[:, axis] = np.divide(np.multiply(centred, spread), extent)
    return out


def pipeline(verts, faces, dim):
    """Every stage of one mesh: dict(occ, odm, surface, aligned)."""
    occ = occupied(verts, faces, dim)
    odm = depth_maps(occ, dim)
    cells = surface(carve(odm))
    return dict(occ=occ, odm=odm, surface=cells, aligned=realign(cells, verts))


def gather(aligned, index):
    """Rows ``index`` of the cloud doubled as often as needed: row r of a doubled cloud is row r mod n."""
    return aligned[np.asarray(index, dtype=np.int64) % aligned.shape[0]]
