"""GPU suite: the resampled joint fit on the device -- the byte codes of mms_joint_sweep_codes against ndcg.joint_codes_host (entry for entry; its
values, histograms and status against mms_joint_sweep, bit for bit), mms_resample_select against ndcg.resample_select_host (winners entry for entry,
values and probes bit for bit, NaN matching NaN) and ensemble.fit_joint_resampled(where="device") against where="host", field for field."""
import functools

import numpy as np
import pytest
import torch

import joint_tables
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SMALL = (7, 3, 12, 5, 1, 20, 9, 6, 33, 4)                                # rows of the key queries of the small table
BEST_BYTE = 0x21                                                         # ideal 1, mask 1: value 1.0, the largest -- the padding of the host-built code matrices


@functools.lru_cache(maxsize=None)
def _host_codes(trial, rows_per_query, M, n_weights, n_filters, k, missing=False):
    """ndcg.joint_codes_host on joint_tables.table(trial, rows_per_query, M) (``missing``: plus two key queries without rows): once, read-only."""
    q, p, mem, key = _table(trial, rows_per_query, M, missing)
    with np.errstate(invalid="ignore"):
        c = ndcg.joint_codes_host(q, p, mem, joint_tables.weights(M, n_weights), joint_tables.filters(n_filters), key, k, allow_missing=missing)
    c.setflags(write=False)
    return c


def _table(trial, rows_per_query, M=4, missing=False):
    q, p, mem, key = joint_tables.table(trial, None if rows_per_query is None else list(rows_per_query), M)
    if missing:
        key = dict(key)
        key[999999] = [5]
        key = {**{999998: []}, **key}                                    # one in front, one behind
    return q, p, mem, key


def _check_codes(trial, rows_per_query, M=4, n_weights=None, n_filters=13, k=5, missing=False, chunk=None):
    q, p, mem, key = _table(trial, rows_per_query, M, missing)
    w, f = joint_tables.weights(M, n_weights), joint_tables.filters(n_filters)
    values, hist, status, codes = ndcg.joint_codes_device(q, p, mem, w, f, key, k, missing, want_hist=True, chunk_tiles=chunk)
    plain = ndcg.joint_sweep_device(q, p, mem, w, f, key, k, missing, want_hist=True, chunk_tiles=chunk)
    for a, b in zip((values, hist, status), plain):                     # what mms_joint_sweep gives, bit for bit
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert status.tolist()[2] == 0
    W, G, Qa = len(w), len(f), len(key)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (G, Qa, (W + 63) // 64 * 64)
    got = codes.cpu().numpy()[:, :, :W].transpose(2, 0, 1)
    want = _host_codes(trial, rows_per_query, M, n_weights, n_filters, k, missing)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, ("(vector, filter, key query) codes that differ", len(bad), bad[:8].tolist())
    return want


# ---- 1. the codes of mms_joint_sweep_codes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 2, None])
@pytest.mark.parametrize("w", [37, 64, 65, 130])
def test_codes_at_the_edges_of_the_64_vector_tile_in_every_chunking(w, chunk):
    _check_codes(3, SMALL, n_weights=w, n_filters=3, chunk=chunk)


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("m", [4, 5])
def test_codes_for_both_record_sizes_and_k(k, m):
    _check_codes(2, SMALL, M=m, n_weights=20, n_filters=5, k=k)


def test_codes_of_dropped_queries():
    want = _check_codes(4, tuple([12] * 16))
    assert int((want == 0xFE).sum()) == 4816 and not (want == 0xFF).any()


@pytest.mark.parametrize("chunk", [1, None])
def test_codes_of_key_queries_without_rows(chunk):
    want = _check_codes(1, SMALL, n_weights=70, n_filters=5, missing=True, chunk=chunk)
    assert (want[:, :, 0] == 0xFF).all() and (want[:, :, -1] == 0xFF).all() and not (want[:, :, 1:-1] == 0xFF).any()


# ---- 2. mms_resample_select against the host form ----------------------------------------------------------------------------------------------------------------
def _dev_codes(codes):
    """Host codes [W, G, Qa] in the device layout [G, Qa, Wp]; the padding v >= W holds the best byte there is: a lane that read it would win."""
    W, G, Qa = codes.shape
    out = np.full((G, Qa, (W + 63) // 64 * 64), BEST_BYTE, np.uint8)
    out[:, :, :W] = codes.transpose(1, 2, 0)
    return torch.from_numpy(out).to(DEV)


def _select(codes, cf, ce, k=5, probes=None):
    out = ndcg.resample_select_device(_dev_codes(codes), codes.shape[0], cf, ce, k, probes)
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want):
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), ("winners", got[0].tolist(), want[0].tolist())
    for name, a, b in zip(("fit_value", "eval_value", "probe_fit", "probe_eval"), got[1:5], want[1:]):
        assert a.dtype == np.float64 and a.shape == b.shape, name
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan) and a[~nan].tobytes() == b[~nan].tobytes(), name                  # bit for bit, NaN matching NaN


def _counts(qa, r, scheme):
    cf, ce = ensemble.kfold_counts(qa, 5, 8, seed=r) if scheme == "kfold" else ensemble.bootstrap_counts(qa, 40, seed=r)
    return np.ascontiguousarray(cf[:r]), np.ascontiguousarray(ce[:r])


@pytest.mark.parametrize("r,p,scheme", [(1, 0, "kfold"), (5, 1, "kfold"), (17, 3, "bootstrap"), (40, 3, "kfold"), (40, 0, "bootstrap")])
def test_replicates_and_probes_against_the_host_form(r, p, scheme):
    codes = _host_codes(1, None, 4, None, 13, 5)                         # 37 x 13 items, 58 key queries
    cf, ce = _counts(codes.shape[2], r, scheme)
    probes = [480, 0, 207][:p]
    got = _select(codes, cf, ce, 5, probes)
    _same(got, ndcg.resample_select_host(codes, cf, ce, 5, probes))
    assert got[5].tolist() == [0, 0, 0, 0] and (got[0] >= 0).all()
    if r >= 17:
        assert len(set(got[0].tolist())) > 1                             # the replicates do not all select the same item


def test_a_count_of_255_an_empty_eval_row_and_an_empty_fit_row():
    codes = _host_codes(4, tuple([12] * 16), 4, None, 13, 5)             # the table with dropped queries: bytes of 0xFE
    cf, ce = _counts(codes.shape[2], 17, "bootstrap")
    cf, ce = cf.copy(), ce.copy()
    cf[2] = 0
    ce[4] = 0
    cf[5, 3] = 255
    ce[16, 15] = 255
    got = _select(codes, cf, ce, 5, [7, 100000, -1])                     # two probes outside the grid: NaN
    want = ndcg.resample_select_host(codes, cf, ce, 5, [7, 100000, -1])
    _same(got, want)
    assert got[5].tolist() == [0, 0, ndcg.FLAG_EMPTY_FIT, 0]
    assert got[0][2] == -1 and np.isnan(got[1][2]) and np.isnan(got[2][2]) and np.isnan(got[2][4]) and not np.isnan(got[1][4])
    assert np.isnan(got[3][:, 1:]).all() and np.isnan(got[4][:, 1:]).all() and not np.isnan(got[4][2, 0])


@pytest.mark.parametrize("k", [1, 3])
def test_other_k(k):
    codes = _host_codes(2, SMALL, 4, 20, 5, k)
    cf, ce = _counts(codes.shape[2], 5, "kfold")
    _same(_select(codes, cf, ce, k, [3]), ndcg.resample_select_host(codes, cf, ce, k, [3]))


def test_ties_across_lanes_and_tiles_take_the_first_item():
    codes = _host_codes(1, None, 4, 80, 13, 5)                           # weights(4, 80): every item occurs again 37 vectors later, two tiles
    assert np.array_equal(codes[:37], codes[37:74])
    cf, ce = _counts(codes.shape[2], 17, "kfold")
    got = _select(codes, cf, ce)
    _same(got, ndcg.resample_select_host(codes, cf, ce))
    assert (got[0] < 37 * 13).all()


def _random_case(W, G, Qa, R, seed):
    rng = np.random.default_rng(seed)
    valid = np.array([i << 5 | m for i in range(6) for m in range(32)] + [0xFE, 0xFF] * 8, np.uint8)
    codes = valid[rng.integers(0, len(valid), (W, G, Qa))]
    codes[W - 1] = codes[3]                                              # exact ties between the first and the last tile
    codes[W // 2, :, :] = codes[1, ::-1, :]
    cf = rng.integers(0, 4, (R, Qa)).astype(np.uint8)
    ce = (cf == 0).astype(np.uint8)
    cf[R // 2, Qa // 2] = 255
    return codes, cf, ce


@pytest.mark.parametrize("shape", [(300, 7, 1000, 40), (70, 600, 3, 224)])
def test_random_bytes_without_a_sweep_across_every_block_boundary_twice(shape):
    # (300, 7, 1000, 40): five tiles, nine unit blocks with a partial last one, three replicate blocks with a partial last one, 250 steps of four key queries
    # (70, 600, 3, 224): 300 unit blocks (more than the 256 threads that pick), 4 200 tasks (more than the grid), fewer key queries than a step: ties everywhere
    W, G, Qa, R = shape
    codes, cf, ce = _random_case(W, G, Qa, R, seed=W)
    probes = [0, W * G - 1, 64 * G]
    dev = _dev_codes(codes)
    a = ndcg.resample_select_device(dev, W, cf, ce, 5, probes)
    b = ndcg.resample_select_device(dev, W, cf, ce, 5, probes)
    a, b = (tuple(t.cpu().numpy() for t in x) for x in (a, b))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))        # equal inputs, equal bytes
    _same(a, ndcg.resample_select_host(codes, cf, ce, 5, probes))
    empty = bool((cf.sum(1) == 0).any())                                 # (three key queries with counts 0..3: some fit rows are empty)
    assert empty == (Qa == 3) and a[5].tolist() == [0, 0, ndcg.FLAG_EMPTY_FIT if empty else 0, 0] and np.array_equal(a[0] < 0, cf.sum(1) == 0)


# ---- 3. ensemble.fit_joint_resampled --------------------------------------------------------------------------------------------------------------------------
def _fields_equal(got, want):
    assert got["whole"][2:4] == want["whole"][2:4] and got["whole"][4].tobytes() == want["whole"][4].tobytes() and repr(got["whole"][:2]) == repr(want["whole"][:2])
    assert got["probes"] == want["probes"] and np.array_equal(got["winners"], want["winners"])
    for name in ("fit_values", "eval_values", "probe_fit", "probe_eval", "count_fit", "count_eval"):
        a, b = got[name], want[name]
        nan = np.isnan(b) if b.dtype == np.float64 else np.zeros(b.shape, bool)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(nan, np.isnan(a) if a.dtype == np.float64 else nan), name
        assert a[~nan].tobytes() == b[~nan].tobytes(), name
    for name in ("heldout", "optimism", "agreement"):
        assert got[name] == want[name] or (np.isnan(got[name]) and np.isnan(want[name])), name


W20, F7 = joint_tables.weights(4, 20), joint_tables.filters(7)


@pytest.mark.parametrize("scheme", ["kfold", "bootstrap"])
def test_fit_joint_resampled_on_the_device_equals_the_host_form(scheme):
    q, p, mem, key = joint_tables.table(1)
    info = {}
    kw = dict(scheme=scheme, folds=5, repeats=2, replicates=12, seed=3, probes=[(2, 1), (19, 6)])
    got = ensemble.fit_joint_resampled(q, p, mem, key, W20, F7, info=info, **kw)
    with np.errstate(invalid="ignore"):
        want = ensemble.fit_joint_resampled(q, p, mem, key, W20, F7, where="host", **kw)
        whole = ensemble.fit_joint(q, p, mem, key, W20, F7)
    assert info == {"path": "device", "flags": 0}
    _fields_equal(got, want)
    assert got["whole"][2:4] == whole[2:4] and got["whole"][4].tobytes() == whole[4].tobytes()                   # bit-equal to fit_joint
    assert got["probes"][0] == whole[3] and got["winners"].shape == (10 if scheme == "kfold" else 12, 2)
    assert (got["fit_values"] >= got["probe_fit"][:, 0]).all() and 0.0 <= got["agreement"] <= 1.0


def test_a_repeated_pair_goes_to_the_host_path_and_still_agrees():
    q, p, mem, key = joint_tables.table(1, list(SMALL))
    q2, p2, mem2 = np.r_[q, q[5]], np.r_[p, p[5]], np.c_[mem, np.full((4, 1), 0.5, np.float32)]
    w, f = joint_tables.weights(4, 9), joint_tables.filters(5)
    info = {}
    with np.errstate(invalid="ignore"):
        got = ensemble.fit_joint_resampled(q2, p2, mem2, key, w, f, folds=3, repeats=1, info=info)
        want = ensemble.fit_joint_resampled(q2, p2, mem2, key, w, f, folds=3, repeats=1, where="host")
    assert info["path"] == "host" and info["flags"] & ndcg.FLAG_REPEATED_PAIR, info
    _fields_equal(got, want)


def test_missing_key_query_raises_keyerror_unless_allowed_and_the_budget_is_checked():
    q, p, mem, key = _table(1, SMALL, missing=True)
    w, f = joint_tables.weights(4, 9), joint_tables.filters(5)
    with pytest.raises(KeyError):
        ensemble.fit_joint_resampled(q, p, mem, key, w, f, folds=3, repeats=1)
    info = {}
    got = ensemble.fit_joint_resampled(q, p, mem, key, w, f, folds=3, repeats=1, allow_missing=True, info=info)
    assert info == {"path": "device", "flags": 0}
    _fields_equal(got, ensemble.fit_joint_resampled(q, p, mem, key, w, f, folds=3, repeats=1, allow_missing=True, where="host"))
    with pytest.raises(ValueError, match="coarser grid"):
        ensemble.fit_joint_resampled(q, p, mem, key, w, f, code_budget=5 * len(key) * 64 - 1)
