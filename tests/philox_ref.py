"""Host emulations of csrc/sample.hip for the tests (plain module, no fixtures): Philox4x32-10 in numpy uint64 arithmetic
vectorised over the counter, the Philox branch of sample_fwd_kernel in numpy float32 (emulate_draws), and the fp32
summation order of face_cdf_kernel (emulate_cdf), in the order the kernel has now and in the one it had before."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # Salmon et al., SC'11: the two multipliers ...
W0, W1 = 0x9E3779B9, 0xBB67AE85                            # ... and the key schedule's Weyl increments
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4), key (2,) or (..., 2), words < 2^32 -> the ten-round output (..., 4) as uint64 words < 2^32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = int(k[..., 0].flat[0]), int(k[..., 1].flat[0])
    assert (k[..., 0] == k0).all() and (k[..., 1] == k1).all(), "one key per call"
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                           # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1)


def u01(x):
    """sample.hip's u01: the top 24 bits as a float32 in [0, 1) (both the conversion and the scaling are exact)."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def counters(offset, n):
    """The n counters {lo32(offset + i), hi32(offset + i), 0, 0}, i < n, the sum wrapping at 2^64."""
    start = int(offset) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        ctr = np.uint64(start) + np.arange(n, dtype=np.uint64)     # uint64 addition wraps as the kernel's does
    out = np.zeros((n, 4), dtype=np.uint64)
    out[:, 0], out[:, 1] = ctr & MASK, ctr >> S32
    return out


def emulate_draws(cdf, seed, offset, draws, batch, num):
    """The Philox branch of sample_fwd_kernel on the host: cdf (batch, F) float32, monotone ->
    (face (draws, batch, num) int32, u, v (draws, batch, num) float32).  Sample i = (draw, b, s) flat takes counter
    offset + i and key {lo32(seed), hi32(seed)}; tgt = min(f32(u01(c0) * tot), f32(tot * f32(1 - 2^-24))) with
    tot = cdf[b][F - 1]; face = the first f with cdf[b][f] > tgt; u = u01(c1), v = u01(c2)."""
    cdf = np.ascontiguousarray(cdf, dtype=np.float32)
    assert cdf.shape[0] == batch and (np.diff(cdf, axis=1) >= 0).all(), "the search is defined on a monotone CDF"
    seed = int(seed) & (2 ** 64 - 1)
    total = draws * batch * num
    r = philox4x32_10(counters(offset, total), (seed & 0xFFFFFFFF, seed >> 32))
    b = (np.arange(total) // num) % batch
    tot = cdf[b, -1]
    tgt = np.minimum(u01(r[:, 0]) * tot, tot * np.float32(1.0 - 2.0 ** -24))
    assert tgt.dtype == np.float32
    face = np.empty(total, dtype=np.int32)
    for m in range(batch):
        sel = b == m
        face[sel] = np.minimum(np.searchsorted(cdf[m], tgt[sel], side="right"), cdf.shape[1] - 1)
    shape = (draws, batch, num)
    return face.reshape(shape), u01(r[:, 1]).reshape(shape), u01(r[:, 2]).reshape(shape)


def chunk_size(n_faces):
    """Faces per thread of face_cdf_kernel's 256 threads."""
    return (n_faces + 255) // 256


def emulate_cdf(p, old=False):
    """face_cdf_kernel's scan of the fp32 probabilities p (F,) in its own order of fp32 additions.  Thread t sums its chunk
    from 0 (part[t]); the bases are the serial exclusive sums of the parts; a chunk is scanned serially from its base,
    cdf[f] = ((base + p1) + p2) + ...  ``old`` stops there, as the kernel once did.  The kernel now joins the chunks: carry =
    the entry written for the last face before the chunk; a chunk whose first p is 0 is scanned from 0 and written as
    carry + local sum, every other chunk keeps its scan from the base, raised to carry where it lies below."""
    p = np.asarray(p, dtype=np.float32)
    F, per = p.size, chunk_size(p.size)
    q = np.zeros(256 * per, dtype=np.float32)
    q[:F] = p
    q = q.reshape(256, per)
    n = np.clip(F - per * np.arange(256), 0, per)             # faces of each chunk
    s = np.zeros(256, dtype=np.float32)
    for j in range(per):
        s = s + q[:, j]
    base = np.zeros(256, dtype=np.float32)
    run = np.float32(0)
    for t in range(256):
        base[t] = run
        run = run + s[t]
    add = np.zeros(256, dtype=bool) if old else (q[:, 0] == 0) | (n == 0)
    out = np.empty((256, per), dtype=np.float32)
    s = np.where(add, np.float32(0), base)
    for j in range(per):
        s = s + q[:, j]
        out[:, j] = s
    if not old:
        carry = np.float32(0)
        for t in range(256):
            if add[t]:
                out[t] = carry + out[t]
            else:
                out[t] = np.maximum(out[t], carry)
            if n[t]:
                carry = out[t, n[t] - 1]
    assert out.dtype == np.float32
    return out.reshape(-1)[:F]
