"""Tables for the joint-sweep tests (the CPU host form and the device path share them) -- no test in here.  The rows and the answer key are those
of filter_tables.table; the score is replaced by M member scores, multiples of 1/64 in [-1, 1] as fp32.  The weight rows are ensemble.weight_grid(M, 4)
(multiples of 1/4) plus two rows that are not dyadic.  With the dyadic rows every product and every sum of the merge is exact and a multiple of 1/256,
so ``d == gap`` and ``e == tie`` happen all the time against filter_tables.grid() (multiples of 1/64); the last two rows exercise the rounding of the
merge.  The host loop costs about 2.6 ms per (weight vector, filter) on a 900-row table: keep W * G at about 1 000 per table; a reference is computed
once per (table, grids, k) and shared."""
import functools

import numpy as np

import filter_tables
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg


def members(trial, n, M=4):
    """float32 [M, n]: default_rng(trial).integers(-64, 65, (M, n)) / 64."""
    return (np.random.default_rng(trial).integers(-64, 65, (M, n)) / 64).astype(np.float32)


def table(trial, rows_per_query=None, M=4):
    """-> (query_id, product_id, members float32 [M, n], answer key dict): filter_tables.table(trial, rows_per_query) with member scores."""
    q, p, _, key = filter_tables.table(trial, rows_per_query)
    return q, p, members(trial, len(q), M), key


def weights(M=4, n=None):
    """float64 [W, M]: weight_grid(M, 4) -- 35 rows for M = 4 --, then (0.2, 0.2, 0.3, 0.3) and (1/3, 1/3, 1/6, 1/6) (cycled to M entries).  ``n``: the
    first n rows of that list repeated as often as it takes (the two rounding rows come first then, so that a short list holds them)."""
    w = np.r_[ensemble.weight_grid(M, 4), [np.resize([0.2, 0.2, 0.3, 0.3], M)], [np.resize([1 / 3, 1 / 3, 1 / 6, 1 / 6], M)]]
    if n is None:
        return w
    w = np.r_[w[-2:], w[:-2]]
    return np.ascontiguousarray(np.resize(w, (n, M)))


def filters(n=13, seed=0):
    """filter_tables.grid(n, seed): row 0 is (-inf, +inf), row 1 the default filter; NaN / +-inf / 0 / -0.0 among the rest."""
    return filter_tables.grid(n, seed)


@functools.lru_cache(maxsize=None)
def _host(trial, rows_per_query, M, n_weights, n_filters, seed, k):
    q, p, mem, key = table(trial, None if rows_per_query is None else list(rows_per_query), M)
    with np.errstate(invalid="ignore"):
        values, hist = ndcg.joint_sweep_host(q, p, mem, weights(M, n_weights), filters(n_filters, seed), key, k)
    values.setflags(write=False)
    hist.setflags(write=False)
    return values, hist


def host(trial, rows_per_query=None, M=4, n_weights=None, n_filters=13, seed=0, k=5):
    """ndcg.joint_sweep_host on table(trial, rows_per_query, M) with weights(M, n_weights) x filters(n_filters, seed): computed once, read-only."""
    return _host(trial, None if rows_per_query is None else tuple(rows_per_query), M, n_weights, n_filters, seed, k)
