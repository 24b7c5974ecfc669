"""The table of the fit-family tests (the CPU host forms and the device path share it) -- no test in here.  Five key queries of 1, 4, 5, 7 and 9 rows,
26 rows in all, interleaved; no (query, product) pair twice, products shared between queries.  Member scores are quarter-integers in [-0.5, 0.5] with
-0.0 in every third row of member 0, the 65 weight vectors quarter-integers in [-0.25, 0.75]: every product and sum of the merge is exact, so ties are
everywhere and the row order decides.  65 vectors are two tiles of 64, the second with one live lane."""
import numpy as np

ROWS_PER_QUERY = (1, 4, 5, 7, 9)
MS, KS = (1, 4, 5, 8), (1, 3, 5)
NO_FILTER = np.array([[-np.inf, np.inf]], np.float64)                     # every row survives: the submission row is the unfiltered top-5


def table(M):
    """-> (query_id int64 [26], product_id int64 [26], members float32 [M, 26], weights float64 [65, M], answer key dict)."""
    rng = np.random.default_rng(17)
    q = np.concatenate([np.full(c, 11 + j, np.int64) for j, c in enumerate(ROWS_PER_QUERY)])
    p = np.concatenate([100 + (3 * j + np.arange(c)) % 12 for j, c in enumerate(ROWS_PER_QUERY)]).astype(np.int64)
    key = {str(11 + j): [str(100 + (3 * j + r) % 12) for r in range(0, c, 2)] + ["999"] for j, c in enumerate(ROWS_PER_QUERY)}
    order = rng.permutation(len(q))
    mem = (rng.integers(-2, 3, (max(MS), len(q))) / 4).astype(np.float32)
    mem[0, ::3] = -0.0
    w = rng.integers(-1, 4, (65, max(MS))) / 4
    assert len(set(zip(q.tolist(), p.tolist()))) == len(q) == 26
    return q[order], p[order], np.ascontiguousarray(mem[:M]), np.ascontiguousarray(w[:, :M]), key
