"""Shared by the ``touch_assemble`` tests (host and GPU): seeded inputs with the values a copy must not change, and the contract of
``a3vt_touch_assemble`` (``include/a3vt.h``) as a NumPy loop over the blocks, moving uint32 words."""
import numpy as np

# NaNs with payloads (quiet and signalling, both signs), the infinities, -0.0, a subnormal
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF80BEEF, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001],
                    dtype=np.uint32)


def _floats(g, shape):
    """Seeded float32 values of ``shape`` with ``SPECIALS`` at seeded places (all of them where the array has room)."""
    a = g.standard_normal(shape).astype(np.float32)
    words = a.reshape(-1).view(np.uint32)
    where = g.permutation(words.size)[:len(SPECIALS)]
    words[where] = SPECIALS[:len(where)]
    return a


def inputs(K, E, A, F, G, C, seed):
    """``(table_charts, table_codes, state_charts, state_masks, candidates)`` as NumPy arrays.  The codes run over -3..5 (the
    kernel clamps into 0..2); candidate 1 repeats candidate 0, and within a candidate the elements share actions where A < E."""
    g = np.random.default_rng(seed)
    table_charts, state_charts, state_masks = _floats(g, (E, A, F, C, 3)), _floats(g, (E, F, G, C, 3)), _floats(g, (E, F, G, C, 1))
    table_codes = g.integers(-3, 6, (E, A, F)).astype(np.int32)
    candidates = g.integers(0, A, (K, E)).astype(np.int32)
    if K > 1:
        candidates[1] = candidates[0]
    return table_charts, table_codes, state_charts, state_masks, candidates


def reference(table_charts, table_codes, state_charts, state_masks, candidates, slot):
    """-> ``(charts (K, E, F * G * C, 3), masks (K, E, F * G * C, 1))`` as uint32 words."""
    E, A, F, C, _ = table_charts.shape
    G = state_charts.shape[2]
    K = candidates.shape[0]
    tc, sc = table_charts.view(np.uint32), state_charts.view(np.uint32)
    sm = np.ascontiguousarray(state_masks).reshape(E, F, G, C).view(np.uint32)
    charts, masks = np.empty((K, E, F, G, C, 3), np.uint32), np.empty((K, E, F, G, C), np.uint32)
    for k in range(K):
        for e in range(E):
            a = int(candidates[k, e])
            for f in range(F):
                for g in range(G):
                    if g != slot:
                        charts[k, e, f, g], masks[k, e, f, g] = sc[e, f, g], sm[e, f, g]
                    elif 0 <= a < A:
                        charts[k, e, f, g] = tc[e, a, f]
                        masks[k, e, f, g] = np.float32(min(max(int(table_codes[e, a, f]), 0), 2)).view(np.uint32)
                    else:
                        charts[k, e, f, g], masks[k, e, f, g] = 0, 0
    return charts.reshape(K, E, F * G * C, 3), masks.reshape(K, E, F * G * C, 1)
