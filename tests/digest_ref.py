"""The geometry digest (include/linr_hip.h "geometry digests") restated in numpy: uint64 arrays that wrap, nothing else.
   G = 0x9E3779B97F4A7C15;  m(v): v ^= v >> 30; v *= 0xBF58476D1CE4E5B9; v ^= v >> 27; v *= 0x94D049BB133111EB; v ^= v >> 31
   r(x, y, z) = m(m(u32(x) | u32(y) << 32) + u32(z) + G), (x, y, z) = row + origin in int32;  D = m(sum r ^ m(n + G))"""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
_C1, _C2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)

# the issue's known answers, computed with plain Python integers: (rows, origin, D)
KNOWN = [
    ([], (0, 0, 0), 0x48218226ff3cd4bf),
    ([(0, 0, 0)], (0, 0, 0), 0x8e58975f6d0dc556),
    ([(1, 2, 3), (-1, 2 ** 31 - 1, -2 ** 31)], (0, 0, 0), 0x2fb051dd12d1e535),
    ([(1, 2, 3), (4, 5, 6)], (10, -20, 30), 0xf2be1d4320cbd4c0),
    ([(1, 2, 3), (1, 2, 3)], (0, 0, 0), 0x49e80c0367870be3),
]


def mix(v):
    v = np.asarray(v, dtype=np.uint64).copy()
    with np.errstate(over='ignore'):
        v ^= v >> np.uint64(30)
        v *= _C1
        v ^= v >> np.uint64(27)
        v *= _C2
        v ^= v >> np.uint64(31)
    return v


def row_terms(rows, origin=None):
    """r of every row: uint64 [n]."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    org = np.zeros(3, dtype=np.int64) if origin is None else np.asarray(origin, dtype=np.int64).reshape(3)
    u = ((rows + org) & 0xFFFFFFFF).astype(np.uint64)              # int32 addition that wraps = the sum's low 32 bits
    with np.errstate(over='ignore'):
        return mix(mix(u[:, 0] | (u[:, 1] << np.uint64(32))) + u[:, 2] + G)


def digest(rows, origin=None):
    """D of the rows (anything that reshapes to int [n, 3]) as a Python int."""
    terms = row_terms(rows, origin)
    with np.errstate(over='ignore'):
        s = np.add.reduce(terms, dtype=np.uint64) if terms.size else np.uint64(0)
        return int(mix(np.uint64(s) ^ mix(np.uint64(terms.size) + G)))


def digest_segments(coords, seg_off, origins=None):
    """[D of rows seg_off[j] .. seg_off[j + 1]) for every j], origins: per segment or None."""
    coords = np.asarray(coords).reshape(-1, 3)
    return [digest(coords[int(seg_off[j]):int(seg_off[j + 1])], None if origins is None else origins[j]) for j in range(len(seg_off) - 1)]
