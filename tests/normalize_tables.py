"""Tables and the witness for the normalisation tests (the CPU host form and the device path share them) -- no test in here.  The witness
(``restate``) is a dict walk in pure Python floats, one group and one member at a time, rounded to fp32 through ``struct``: it shares no code and no
numpy reduction with ensemble.normalize_members.  Member scores are multiples of 1/64 in [-1, 1] (joint_tables.members), so every sum of the z-score
is exact and ties, -0.0 and constant groups happen all the time."""
import math
import struct

import numpy as np

MODES = ("minmax", "zscore", "rank")
EDGE_GROUPS = (1, 2, 63, 64, 65, 200)          # rows per query: below, at and beyond one wavefront


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def restate(query_id, members, mode):
    """The definition of include/mmscore.h, read literally: float32 [M, n]."""
    groups = {}
    for r, q in enumerate(np.asarray(query_id).tolist()):
        groups.setdefault(q, []).append(r)                                   # ascending row index
    out = np.zeros(np.shape(members), np.float32)
    for m, row in enumerate(np.asarray(members, np.float32).tolist()):
        for rows in groups.values():
            xs = [row[r] + 0.0 for r in rows]
            c = len(xs)
            if mode == "minmax":
                lo, hi = min(xs), max(xs)
                vals = [0.0 if hi == lo else (x - lo) / (hi - lo) for x in xs]
            elif mode == "zscore":
                s1 = 0.0
                for x in xs:
                    s1 = s1 + x
                mean = s1 / float(c)
                s2 = 0.0
                for x in xs:
                    d = x - mean
                    s2 = s2 + d * d
                sd = math.sqrt(s2 / float(c))
                vals = [(x - mean) / sd if sd > 0 else 0.0 for x in xs]
            else:
                vals = [0.0 if c == 1 else float(c - 1 - sum(1 for y in xs if y > x)) / float(c - 1) for x in xs]
            for r, v in zip(rows, vals):
                out[m, r] = f32(v)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def edge_table(M=4, shuffled=False, seed=0):
    """-> (query_id int64 [395], members float32 [M, 395]): queries of EDGE_GROUPS rows with unrelated ids (one negative, one beyond 2^32), adjacent
    unless ``shuffled``.  Multiples of 1/64 with -0.0 among them; member 0 is constant inside the 64-row query, the last member is +-0.0 inside the
    2-row query."""
    rng = np.random.default_rng(9100 + seed)
    ids = [7, 3, 900, -5, 12, 1 << 40]
    q = np.repeat(np.array(ids, np.int64), EDGE_GROUPS)
    n = len(q)
    mem = (rng.integers(-64, 65, (M, n)) / 64).astype(np.float32)
    mem[rng.random((M, n)) < 0.04] = -0.0
    mem[0, q == -5] = 0.375
    mem[M - 1, q == 3] = (0.0, -0.0)
    if shuffled:
        perm = rng.permutation(n)
        q, mem = q[perm], np.ascontiguousarray(mem[:, perm])
    return q, mem
