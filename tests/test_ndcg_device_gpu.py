"""GPU suite: the valid half on the device (mms_key_relevance / mms_ndcg_at_k, ndcg.relevance_device / ndcg_device, pipeline.evaluate_tsv_native)
against the HOST code: ndcg.ndcg_from_arrays (the restatement of the reference's evaluation.py) for the value, ndcg.ndcg_codes (numpy, a stable
argsort per query) for the per-query decisions, and a numpy membership test for the labels.  The reference side is never the device output of another
call.  Values are compared bit for bit; wherever the inputs carry no flagged condition the device path may not hide behind its host fallback
(info == {"path": "device", "flags": 0})."""
import numpy as np
import pytest
import torch

from helpers import small_cfg
from ndcg_tables import N_RANDOM, fixture, random_table
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib, ndcg, sharding

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64                  # sentinel elements on either side of every raw output
S32, S64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _device_all(q, p, s, key, k, allow_missing=False):
    """-> (codes, topk, hist, status) of one mms_ndcg_at_k call as numpy arrays."""
    codes, topk, hist, status = ndcg.ndcg_codes_device(q, p, s, key, k, allow_missing, want_topk=True)
    return codes.cpu().numpy(), topk.cpu().numpy(), hist.cpu().numpy(), status.cpu().numpy()


def _check(q, p, s, key, k):
    """Every output of the device path against the host forms; -> the value."""
    want_codes, want_topk = ndcg.ndcg_codes(q, p, s, key, k, return_topk=True)
    codes, topk, hist, status = _device_all(q, p, s, key, k)
    assert status[2] == 0, status
    assert np.array_equal(codes, want_codes)
    assert np.array_equal(topk, want_topk)
    assert hist.dtype == np.int64 and np.array_equal(hist, ndcg.hist_from_codes(want_codes, k))
    keys = np.array([int(x) for x in key], np.int64)
    assert status[0] == len(key) and status[3] == 0 and status[1] == int(np.isin(q, keys).sum())
    info = {}
    got = ndcg.ndcg_device(q, p, s, key, k, info=info)
    assert info == {"path": "device", "flags": 0}, info
    want = ndcg.ndcg_from_arrays(q, p, s, key, k)
    assert got == want, (got, want)                                       # bit for bit
    h, ev = ndcg.ndcg_device(q, p, s, key, k, return_hist=True)
    assert ev == len(key) and np.array_equal(h, hist)
    return got


# ---- 1. the golden valid subset ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fixture_codes_histogram_and_value(dtype):
    q, p, s, ans, exp = fixture()
    s = s.astype(dtype)
    got = {k: _check(q, p, s, ans, k) for k in (1, 5, 8)}
    if dtype is np.float64:
        assert abs(got[5] - exp["ndcg5_subset"]) < 1e-12 and abs(got[1] - exp["ndcg1_subset"]) < 1e-12
    # device tensors in place, and a prebuilt key
    key = ndcg.AnswerKey(ans, DEV)
    dq, dp, ds = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (q, p, s))
    assert ndcg.ndcg_device(dq, dp, ds, key, 5) == got[5]


# ---- 2. random tables: ties, signed zeros, interleaved rows, repeated rows and truth products, empty truth lists, short and long queries, foreign rows,
#         ids near +-2^62 (ndcg_tables.random_table) -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trial", range(N_RANDOM))
def test_random_tables(trial):
    q, p, s, key = random_table(trial)
    for k in (5, 1 if trial % 2 else 8):
        _check(q, p, s, key, k)


# ---- 3. size edges --------------------------------------------------------------------------------------------------------------------------------------
def _plain_table(n_rows_per_query, seed):
    """queries 1000 + i with the given row counts, products 1..40 per query, scores on a 0.25 grid, rows interleaved; truth = three products per query."""
    rng = np.random.default_rng(seed)
    q = np.repeat(1000 + np.arange(len(n_rows_per_query), dtype=np.int64), n_rows_per_query)
    p = rng.integers(1, 41, len(q)).astype(np.int64)
    s = (rng.integers(0, 5, len(q)) * 0.25).astype(np.float64)
    perm = rng.permutation(len(q))
    key = {int(1000 + i): rng.integers(1, 41, 3).tolist() for i in range(len(n_rows_per_query))}
    return q[perm], p[perm], s[perm], key


@pytest.mark.parametrize("n", [1, 1024, 1025])
def test_row_count_edges(n):
    per = [n] if n == 1 else [n - 3 * (n // 4), n // 4, n // 4, n // 4]
    q, p, s, key = _plain_table(per, 60 + n)
    assert len(q) == n
    _check(q, p, s, key, 5)


@pytest.mark.parametrize("qa", [1, 1023, 1024, 1025, 2500])
def test_key_length_edges_of_the_scan_block(qa):
    """the exclusive scan of the per-key row counts works in blocks of 1 024 key queries"""
    rng = np.random.default_rng(qa)
    q, p, s, key = _plain_table(rng.integers(1, 4, qa).tolist(), 70 + qa)
    assert len(key) == qa
    _check(q, p, s, key, 5)
    _check(q, p, s, key, 8)


def test_262145_key_queries_take_two_block_sums_per_thread_of_the_scan_top():
    """257 scan blocks of 1 024 key queries: the one workgroup that turns the block sums into prefixes owns two of them per thread.  One row per key
    query in shuffled order, so a wrong list offset hands a query another query's row: its relevance bit in the code differs."""
    qa = 256 * 1024 + 1
    rng = np.random.default_rng(262145)
    perm = rng.permutation(qa)
    q, p = (1000 + np.arange(qa, dtype=np.int64))[perm], rng.integers(1, 3, qa).astype(np.int64)[perm]
    s = (rng.integers(0, 5, qa) * 0.25).astype(np.float64)
    key = {int(1000 + i): [int(t)] for i, t in enumerate(rng.integers(1, 3, qa))}
    want = ndcg.ndcg_codes(q, p, s, key, 1)
    assert 0 < int((want & 1).sum()) < qa
    codes, _, hist, status = _device_all(q, p, s, key, 1)
    assert status.tolist() == [qa, qa, 0, 0]
    assert np.array_equal(codes, want)
    assert np.array_equal(hist, ndcg.hist_from_codes(want, 1))


def test_one_query_of_300_rows_loops_over_its_list():
    q, p, s, key = _plain_table([300, 7, 64, 65, 128, 129], 81)
    _check(q, p, s, key, 5)
    _check(q, p, s, key, 8)
    s[:] = 0.5                                                           # every score equal: the order is the row order
    _check(q, p, s, key, 8)


def test_no_rows_with_allow_missing():
    _, _, _, ans, _ = fixture()
    e = np.zeros(0, np.int64)
    codes, topk, hist, status = _device_all(e, e, np.zeros(0, np.float32), ans, 5, allow_missing=True)
    assert (codes == -1).all() and (topk == -1).all() and not hist.any() and status.tolist() == [0, 0, 0, len(ans)]
    h, ev = ndcg.ndcg_device(e, e, np.zeros(0, np.float64), ans, 5, allow_missing=True, return_hist=True)
    assert ev == 0 and not h.any()
    assert ndcg.ndcg_device(e, e, np.zeros(0, np.float64), ans, 5, allow_missing=True) == 0.0
    assert ndcg.relevance_device(e, e, ans).shape == (0,)


# ---- 4. flags; nothing is written outside the outputs ------------------------------------------------------------------------------------------------------
def _raw(q, p, s, key_q, key_off, key_p, k, allow_missing, relevance=False):
    """The raw entry point on sentinel-guarded buffers (outputs AND workspace) -> (codes, topk, hist, status, labels) after the guards were checked."""
    l = lib.load()
    n, qa, tk = len(q), len(key_q), len(key_p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dq, dp, ds, dkq, dko, dkp = up(q), up(p), up(s), up(np.asarray(key_q, np.int64)), up(np.asarray(key_off, np.int64)), up(np.asarray(key_p, np.int64))
    ws_bytes = l.mms_ndcg_workspace_bytes(n, qa, tk)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    off = (-ws.data_ptr()) % 256 + 256

    def guarded(count, dtype, fill):
        return torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=DEV)

    codes, topk, hist = guarded(qa, torch.int32, S32), guarded(qa * k, torch.int64, S64), guarded((k + 1) << k, torch.int64, S64)
    status, labels = guarded(4, torch.int32, S32), guarded(n, torch.int64, S64)
    inner = lambda t: t.data_ptr() + GUARD * t.element_size()
    ptr = lambda t: t.data_ptr() if t.numel() else None
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if relevance:
        rc = l.mms_key_relevance(ptr(dq), ptr(dp), n, ptr(dkq), ptr(dko), ptr(dkp), qa, tk, ws.data_ptr() + off, ws_bytes, inner(labels), inner(status), stream)
    else:
        f32 = s.dtype == np.float32
        sp = ptr(ds) or inner(status)
        rc = l.mms_ndcg_at_k(ptr(dq), ptr(dp), sp if f32 else None, None if f32 else sp, n, ptr(dkq), ptr(dko), ptr(dkp), qa, tk, k, int(allow_missing),
                             ws.data_ptr() + off, ws_bytes, inner(codes), inner(topk), inner(hist), inner(status), stream)
    assert rc == 0, l.mms_global_error()
    torch.cuda.synchronize()
    for t, fill in ((codes, S32), (topk, S64), (hist, S64), (status, S32), (labels, S64)):
        h = t.cpu().numpy()
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), "a guard zone was written"
    w = ws.cpu().numpy()
    assert (w[:off] == 0xA5).all() and (w[off + ws_bytes:] == 0xA5).all(), "the workspace's guard zone was written"
    cut = lambda t: t.cpu().numpy()[GUARD:-GUARD]
    if relevance:                                                        # the call may not touch the nDCG outputs at all
        assert (cut(codes) == S32).all() and (cut(hist) == S64).all()
    return cut(codes), cut(topk).reshape(qa, k), cut(hist), cut(status), cut(labels)


def _csr(key):
    kq = [int(x) for x in key]
    off = np.concatenate([[0], np.cumsum([len(t) for t in key.values()])]).astype(np.int64)
    return kq, off, [int(x) for t in key.values() for x in t]


def test_raw_entry_guard_zones_on_a_clean_table():
    q, p, s, key = random_table(2)
    kq, off, kp = _csr(key)
    codes, topk, hist, status, _ = _raw(q, p, s, kq, off, kp, 5, False)
    want_codes, want_topk = ndcg.ndcg_codes(q, p, s, key, 5, return_topk=True)
    assert status[2] == 0 and np.array_equal(codes, want_codes) and np.array_equal(topk, want_topk)
    assert np.array_equal(hist, ndcg.hist_from_codes(want_codes, 5))
    labels = _raw(q, p, s, kq, off, kp, 5, False, relevance=True)[4]
    assert np.array_equal(labels, _membership(q, p, key))


def test_key_query_without_rows_with_and_without_allow_missing():
    q, p, s, key = random_table(4, with_missing=True)
    want = ndcg.ndcg_codes(q, p, s, key, 5, allow_missing=True)
    n_missing = int((want < 0).sum())
    assert 0 < n_missing < len(key)
    kq, off, kp = _csr(key)
    for allow in (True, False):
        codes, _, hist, status, _ = _raw(q, p, s, kq, off, kp, 5, allow)
        assert status.tolist() == [len(key) - n_missing, int(np.isin(q, kq).sum()), 0 if allow else ndcg.FLAG_MISSING_QUERY, n_missing]
        if allow:
            assert np.array_equal(codes, want) and np.array_equal(hist, ndcg.hist_from_codes(want, 5)) and hist.sum() == len(key) - n_missing
    with pytest.raises(KeyError) as dev_err:
        ndcg.ndcg_device(q, p, s, key, 5)
    with pytest.raises(KeyError) as host_err:
        ndcg.ndcg_from_arrays(q, p, s, key, 5)
    assert dev_err.value.args == host_err.value.args                     # the same first missing query
    info = {}
    got = ndcg.ndcg_device(q, p, s, key, 5, info=info, allow_missing=True)
    assert info == {"path": "device", "flags": 0} and got == ndcg.ndcg_from_codes(want, 5)
    h, ev = ndcg.ndcg_device(q, p, s, key, 5, allow_missing=True, return_hist=True)
    assert ev == len(key) - n_missing and np.array_equal(h, ndcg.hist_from_codes(want, 5))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_finite_score_selects_the_host_path(bad, dtype):
    q, p, s, ans, _ = fixture()
    s = s.astype(dtype)
    s[1234] = bad
    kq, off, kp = _csr(ans)
    assert _raw(q, p, s, kq, off, kp, 5, False)[3][2] == ndcg.FLAG_NON_FINITE
    info = {}
    got = ndcg.ndcg_device(q, p, s, ans, 5, info=info)
    assert info == {"path": "host", "flags": ndcg.FLAG_NON_FINITE}
    want = ndcg.ndcg_from_arrays(q, p, s, ans, 5)
    assert got == want or (np.isnan(got) and np.isnan(want))


def test_repeated_key_query_raises_bit_2():
    q, p, s, key = random_table(5)
    kq, off, kp = _csr(key)
    if len(kq) < 2:
        kq, off = kq + [kq[0] + 1], np.r_[off, off[-1]]
    kq[-1] = kq[0]
    for k in (5, 8):
        status = _raw(q, p, s, kq, off, kp, k, True)[3]
        assert status[2] & ndcg.FLAG_REPEATED_KEY and not status[2] & ~(ndcg.FLAG_REPEATED_KEY | ndcg.FLAG_MISSING_QUERY)
    assert _raw(q, p, s, kq, off, kp, 5, True, relevance=True)[3][2] == ndcg.FLAG_REPEATED_KEY


@pytest.mark.parametrize("where", ["query_id", "product_id", "key_query", "key_product"])
def test_reserved_id_raises_bit_3(where):
    q, p, s, key = random_table(7)
    q, p = q.copy(), p.copy()
    kq, off, kp = _csr(key)
    if where == "query_id":
        ids, counts = np.unique(q, return_counts=True)
        q[np.flatnonzero(q == ids[np.argmax(counts)])[1]] = -1           # a row of the longest query: no key query loses its last row
    elif where == "product_id":
        p[len(p) // 3] = -1
    elif where == "key_query":
        kq[0] = -1
    else:
        kp[len(kp) // 2] = -1
    for allow in (True, False):
        assert _raw(q, p, s, kq, off, kp, 5, allow)[3][2] & ndcg.FLAG_RESERVED_ID
    assert _raw(q, p, s, kq, off, kp, 5, True, relevance=True)[3][2] & ndcg.FLAG_RESERVED_ID
    if where in ("query_id", "product_id"):                              # served by the host form, which knows no reserved id
        info = {}
        got = ndcg.ndcg_device(q, p, s, key, 5, info=info)
        assert info["path"] == "host" and info["flags"] & ndcg.FLAG_RESERVED_ID and got == ndcg.ndcg_from_arrays(q, p, s, key, 5)


def test_flagged_inputs_write_nothing_outside_their_buffers():
    """every flag at once, and offsets that do not describe the key: _raw checks the guard zones of all outputs and of the workspace"""
    q, p, s, key = random_table(9, with_missing=True)
    q, p, s = q.copy(), p.copy(), s.astype(np.float64)
    kq, off, kp = _csr(key)
    q[3], p[5], s[7], s[8] = -1, -1, np.nan, np.inf
    kq[1 % len(kq)] = kq[0]
    for k in (1, 8):
        status = _raw(q, p, s, kq, off, kp, k, False)[3]
        assert status[2] & (ndcg.FLAG_NON_FINITE | ndcg.FLAG_RESERVED_ID) == ndcg.FLAG_NON_FINITE | ndcg.FLAG_RESERVED_ID
    _raw(q, p, s, kq, off[::-1].copy(), kp, 5, True)                     # descending offsets
    _raw(q, p, s, kq, off * 1000 - 7, kp, 5, True)                       # offsets far outside [0, Tk]


# ---- 5. determinism and laziness ----------------------------------------------------------------------------------------------------------------------------
def test_identical_calls_give_identical_bytes():
    q, p, s, key = random_table(20)
    a = _device_all(q, p, s, key, 8)
    b = _device_all(q, p, s, key, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    q, p, s, ans, _ = fixture()
    a, b = _device_all(q, p, s, ans, 5), _device_all(q, p, s, ans, 5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_device_calls_only_enqueue():
    q, p, s, ans, _ = fixture()
    key = ndcg.AnswerKey(ans, DEV)
    dq, dp, ds = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (q, p, s))
    ndcg.ndcg_codes_device(dq, dp, ds, key, 5, want_topk=True)           # warm-up: the caching allocator now holds blocks of these sizes
    ndcg.relevance_device(dq, dp, key)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                              # a synchronising torch call in the wrappers raises
    try:
        codes, _, hist, status = ndcg.ndcg_codes_device(dq, dp, ds, key, 5, want_topk=True)
        labels = ndcg.relevance_device(dq, dp, key)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(status[2]) == 0 and np.array_equal(codes.cpu().numpy(), ndcg.ndcg_codes(q, p, s, ans, 5))
    assert np.array_equal(labels.cpu().numpy(), _membership(q, p, ans))


# ---- 6. relevance labels -----------------------------------------------------------------------------------------------------------------------------------
def _membership(q, p, key):
    truth = {int(kq): set(int(x) for x in t) for kq, t in key.items()}
    return np.array([int(int(pp) in truth.get(int(qq), ())) for qq, pp in zip(q, p)], np.int64)


def test_relevance_device_equals_the_membership_test():
    seen = set()
    for trial in range(N_RANDOM):
        q, p, _, key = random_table(trial, with_missing=trial % 4 == 0)
        st = []
        got = ndcg.relevance_device(q, p, key, status_out=st)
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        want = _membership(q, p, key)
        assert np.array_equal(got.cpu().numpy(), want), trial
        keys = [int(x) for x in key]
        present = set(q.tolist())
        assert st[0].cpu().tolist() == [sum(x in present for x in keys), int(np.isin(q, keys).sum()), 0, sum(x not in present for x in keys)]
        seen.update(want.tolist())
    assert seen == {0, 1}
    q, p, _, ans, _ = fixture()
    want = _membership(q, p, ans)
    assert 0 < want.sum() < len(q) and np.array_equal(ndcg.relevance_device(q, p, ans).cpu().numpy(), want)


# ---- 7. query shards ---------------------------------------------------------------------------------------------------------------------------------------
def test_eight_query_blocks_sum_to_the_whole_tables_histogram():
    q, p, s, ans, _ = fixture()
    whole, ev = ndcg.ndcg_device(q, p, s, ans, 5, return_hist=True)
    assert ev == 200
    qs = np.unique(q)
    total, evaluated = np.zeros_like(whole), 0
    for r in range(8):
        lo, hi = sharding.query_block(len(qs), 8, r)
        mine = np.isin(q, qs[lo:hi])
        info = {}
        h, e = ndcg.ndcg_device(q[mine], p[mine], s[mine], ans, 5, info=info, allow_missing=True, return_hist=True)
        assert info == {"path": "device", "flags": 0} and e == hi - lo == h.sum()
        h, e = sharding.reduce_ndcg(h, e)                                # no process group: the identity
        total += h.numpy()
        evaluated += e
    assert evaluated == 200 and np.array_equal(total, whole)
    assert ndcg.ndcg_from_hist(total, 5, 200) == ndcg.ndcg_from_hist(whole, 5, 200)
    assert abs(ndcg.ndcg_from_hist(total, 5, 200) - ndcg.ndcg_from_arrays(q, p, s, ans, 5)) <= 1e-12


# ---- 8. the file-fed valid pass ------------------------------------------------------------------------------------------------------------------------------
N_QUERIES, PER_QUERY = 24, 10
# These tests compare the scores of SEPARATE passes over one file bit for bit, so the scorer has to repeat itself.  lxmert's distinct-query stage
# (pack_tokens: the language layers once per distinct query, taken when at least half of a call's pairs share their query -- every call of a valid
# file) does not on calls of this size: the same feed scored twice by scorers.score_batch differs by up to 0.1 in some rows (LABBOOK.md, the entry
# of this test file).  The dense token layout does; what is under test here is the pass and the metric, not that stage.
DENSE = {"lxmert": dict(pack_tokens=False)}


def _valid_records():
    """24 queries x 10 records, product ids 5000 + row; the answer key names three of every query's products (plus one that no record carries)."""
    from test_feature_text_gather import TABLE
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer as F
    rng = np.random.default_rng(77)
    classes = [int(k) for k in TABLE]
    lines, key, pid = [], {}, 5000
    for qi in range(N_QUERIES):
        pids = list(range(pid, pid + PER_QUERY)); pid += PER_QUERY
        key[str(300 + qi)] = [int(x) for x in rng.choice(pids, 3, replace=False)] + [999999]
        for x in pids:
            nb = int(rng.integers(1, 12))
            h, w = int(rng.integers(50, 1200)), int(rng.integers(50, 1200))
            boxes = rng.uniform(0, 1, (nb, 4)).astype(np.float32) * np.array([h, w, h, w], np.float32)
            feats = rng.standard_normal((nb, 2048)).astype(np.float32)
            lines.append(F.encode_record(int(x), h, w, boxes, feats, rng.choice(classes, nb), "blue shirt %d" % qi, 300 + qi))
    return lines, key


@pytest.fixture(scope="module")
def valid_tsv(tmp_path_factory):
    lines, key = _valid_records()
    path = tmp_path_factory.mktemp("ndcg") / "valid.tsv"
    path.write_text("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n" + "".join(l + "\n" for l in lines), encoding="utf-8")
    return str(path), lines, key


@pytest.mark.parametrize("name", ["lds", "lxmert"])
def test_evaluate_tsv_native_device_metric_equals_host_metric(valid_tsv, name):
    from test_feature_text_gather import TABLE, VOCAB
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import pipeline, scorers, weights
    path, _, key = valid_tsv
    cfg = small_cfg(name)
    sc = scorers.make_scorer(cfg, weights.make_weights(cfg), **DENSE.get(name, {}))
    try:
        info, out = {}, {}
        dev = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, info=info, scores_out=out)
        host = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, metric="host")
        ones = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, labels="ones")
        qid, pid, score = pipeline.stream_scores_tsv(sc, path, VOCAB, TABLE, batch_pairs=64)
        with pytest.raises(ValueError):
            pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, metric="gpu")
        with pytest.raises(ValueError):
            pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, labels="truth")
    finally:
        sc.close()
    assert info == {"path": "device", "flags": 0}
    assert len(score) == N_QUERIES * PER_QUERY and np.array_equal(out["score"].cpu().numpy(), score) and np.array_equal(out["query_id"], qid)
    want = ndcg.ndcg_from_arrays(qid, pid, score, key, 5)
    assert dev == host == ones == want and 0.0 < want <= 1.0               # these models read no label


def _force_margin(cfg, w, lines, key):
    """zk weights whose AM-softmax margin branch is taken on this file under the answer labels: column 0 of the class kernel gets cosine 0.5 (> 0.35) with the
    pooled vector of a record whose ground-truth label is 0, found with the numpy oracle.  -> (weights, that record's row)."""
    from oracle import np_models as O
    from test_feature_text_gather import TABLE, VOCAB
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd.featurizer_native import NativeFeaturizer
    nf = NativeFeaturizer(VOCAB, TABLE, "zk", threads=2)
    try:
        b = {k: np.array(v) for k, v in nf.batch(lines[:2 * PER_QUERY]).items()}
    finally:
        nf.close()
    truth = _membership(b["query_id"], b["product_id"], key)
    row = int(np.flatnonzero(truth == 0)[0])
    inter = {}
    O.forward(cfg, w, b, np.float64, inter)
    kern = w["cls/seq_relationship/am_kernel"].astype(np.float64)
    u = inter["pooled"][row] / np.linalg.norm(inter["pooled"][row])
    v = kern[:, 0] - (kern[:, 0] @ u) * u                               # cosine 0.5: the label-0 logit falls from 15 to 4.5, a score change that
    kern[:, 0] = 0.5 * u + np.sqrt(0.75) * v / np.linalg.norm(v)        # survives the ensemble's 0.2 weight in fp32
    return dict(w, **{"cls/seq_relationship/am_kernel": kern.astype(np.float32)}), row


def test_evaluate_tsv_native_zk_answer_labels(valid_tsv):
    from test_feature_text_gather import TABLE, VOCAB
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import pipeline, scorers, weights
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd.featurizer_native import NativeFeaturizer
    path, lines, key = valid_tsv
    cfg = small_cfg("zk")
    w, row = _force_margin(cfg, weights.make_weights(cfg), lines, key)
    sc = scorers.make_scorer(cfg, w)
    nf = NativeFeaturizer(VOCAB, TABLE, "zk", threads=2)
    try:
        info, ans_out, ones_out = {}, {}, {}
        dev = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, info=info, scores_out=ans_out)
        host = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, metric="host")
        dev_dd = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, feat_decode="device")
        ones = pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, key, batch_pairs=64, labels="ones", scores_out=ones_out)
        qid, pid, stream_score = pipeline.stream_scores_tsv(sc, path, VOCAB, TABLE, batch_pairs=64)
        # ZkScorer called directly with the ground-truth labels on the same records, in the pass's own batches (ramp 1024 > the file: batches of 64)
        truth = _membership(qid, pid, key)
        direct = []
        for a in range(0, len(lines), 64):
            b = nf.batch(lines[a:a + 64])
            b = dict(b, labels=truth[a:a + 64])
            direct.append(scorers.score_batch(sc, b)[1][:, 1].float().cpu().numpy())
        direct = np.concatenate(direct)
    finally:
        nf.close()
        sc.close()
    assert info == {"path": "device", "flags": 0}
    ans_score, ones_score = ans_out["score"].cpu().numpy(), ones_out["score"].cpu().numpy()
    assert np.array_equal(ans_out["query_id"], qid) and np.array_equal(ans_out["product_id"], pid)
    assert np.array_equal(ones_score, stream_score)                      # labels="ones" is today's feed
    assert np.array_equal(ans_score, direct)                             # bit for bit
    assert truth[row] == 0 and ans_score[row] != ones_score[row]         # the margin branch was taken where _force_margin put it
    assert np.array_equal(ans_score[truth == 1], ones_score[truth == 1])  # label 1 either way
    assert dev == host == dev_dd == ndcg.ndcg_from_arrays(qid, pid, ans_score, key, 5)
    assert ones == ndcg.ndcg_from_arrays(qid, pid, ones_score, key, 5)


def test_evaluate_tsv_native_ensemble_and_shards(valid_tsv):
    from test_feature_text_gather import TABLE, VOCAB
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import pipeline, scorers, weights
    path, lines, key = valid_tsv
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    ws = {n: weights.make_weights(c) for n, c in cfgs.items()}
    ws["zk"], row = _force_margin(cfgs["zk"], ws["zk"], lines, key)
    sc = {n: scorers.make_scorer(c, ws[n], **DENSE.get(n, {})) for n, c in cfgs.items()}
    try:
        ens = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
        info, ans_out, ones_out = {}, {}, {}
        dev = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, batch_pairs=64, info=info, scores_out=ans_out)
        host = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, batch_pairs=64, metric="host")
        ones = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, batch_pairs=64, labels="ones", scores_out=ones_out)
        qid, pid, merged = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)[:3]
        # the single-model pass in two query shards: histograms for reduce_ndcg
        parts = [pipeline.evaluate_tsv_native(sc["lds"], path, VOCAB, TABLE, key, batch_pairs=64, shard=(r, 2), shard_by="queries", metric=m)
                 for r in (0, 1) for m in ("device", "host")]
        whole = pipeline.evaluate_tsv_native(sc["lds"], path, VOCAB, TABLE, key, batch_pairs=64)
    finally:
        for s in sc.values():
            s.close()
    assert info == {"path": "device", "flags": 0}
    ans_score, ones_score = ans_out["score"].cpu().numpy(), ones_out["score"].cpu().numpy()
    assert ans_score.dtype == np.float64 and np.array_equal(ones_score, merged)
    assert ans_score[row] != ones_score[row]                             # zk's margin reached the merged score
    assert dev == host == ndcg.ndcg_from_arrays(qid, pid, ans_score, key, 5)
    assert ones == ndcg.ndcg_from_arrays(qid, pid, merged, key, 5)
    (h0, e0), (h0h, e0h), (h1, e1), (h1h, e1h) = parts
    assert e0 == e0h == e1 == e1h == N_QUERIES // 2 and np.array_equal(h0, h0h) and np.array_equal(h1, h1h)
    assert ndcg.ndcg_from_hist(np.asarray(h0) + np.asarray(h1), 5, N_QUERIES) == pytest.approx(whole, abs=1e-12)
