"""GPU suite, kernel level: the pack plans (csrc/rowops.hip) and the hash-table de-duplication (csrc/batchops.hip) against numpy statements of
what they must produce (tests/helpers.py, pinned to the oracle by tests/test_plan_specs.py; np.unique; "first occurrence").  All comparisons are
exact unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib
from test_plan_specs import lds_edge_pairs, lx_edge_pairs

pytestmark = pytest.mark.gpu

GUARD = -77          # fill of every output buffer: an entry the plan does not own must keep it


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _ibuf(n):
    return torch.full((max(int(n), 1),), GUARD, device="cuda", dtype=torch.int32)


def _fbuf(n):
    return torch.full((max(int(n), 1),), float(GUARD), device="cuda", dtype=torch.float32)


def _plan(kind, n, T, a, b, S, second, refused=False):
    """-> dict of numpy tables (whole buffers, guard fill included)"""
    l = lib.load()
    da, db = _dev(a), (None if b is None else _dev(b))
    t = dict(off=_ibuf(n), cnt=_ibuf(n), src=_ibuf(n * S), add=_fbuf(n * S), off2=_ibuf(n), cnt2=_ibuf(n), src2=_ibuf(n * 10), add2=_fbuf(n * 10), rows=_ibuf(4))
    p = {k: v.data_ptr() for k, v in t.items()}
    rc = l.mms_dbg_pack_plan(kind, n, T, da.data_ptr(), None if db is None else db.data_ptr(), p["off"], p["cnt"], p["src"], p["add"],
                             p["off2"] if second else None, p["cnt2"] if second else None, p["src2"] if second else None, p["add2"] if second else None,
                             p["rows"], None)
    assert (rc != 0) if refused else (rc == 0), l.mms_global_error()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _check_table(got_off, got_cnt, got_src, got_add, got_rows, off, cnt, src, add, what, add_tol=0.0):
    n, rows = len(cnt), len(src)
    assert got_rows == rows, (what, got_rows, rows)
    assert np.array_equal(got_cnt[:n], cnt), what
    assert np.array_equal(got_off[:n], off), what
    assert np.array_equal(got_src[:rows], src), (what, np.flatnonzero(got_src[:rows] != src)[:5])
    assert np.all(got_src[rows:] == GUARD), what                        # nothing written past the live total
    if add is not None:
        if add_tol:
            err = np.abs(got_add[:rows].astype(np.float64) - add).max()
            assert err <= add_tol, (what, err)
            assert np.all(got_add[:rows][add == 0.0] == 0.0), what      # multiplicity 1: exactly 0
        else:
            assert np.array_equal(got_add[:rows], add), (what, np.flatnonzero(got_add[:rows] != add)[:5])
        assert np.all(got_add[rows:] == GUARD), what


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _zk_inputs(n, T):
    """every combination of the edge values first (25 pairs, cycled), random values after them"""
    lq_e, nb_e = np.meshgrid([-3, 0, 1, T, T + 5], [-1, 0, 1, 10, 13], indexing="ij")
    r = np.random.default_rng(n)
    lq = r.integers(-2, T + 3, n)
    nb = r.integers(-2, 13, n)
    m = min(n, 25) if n < 50 else 50
    lq[:m] = np.resize(lq_e.ravel(), m)
    nb[:m] = np.resize(nb_e.ravel(), m)
    if n >= 25:      # ... and again at the end: the last thread's pairs of the block scan
        lq[-25:] = lq_e.ravel()
        nb[-25:] = nb_e.ravel()
    return lq.astype(np.int32), nb.astype(np.int32)


def _check_zk(t, sp, what):
    _check_table(t["off"], t["cnt"], t["src"], t["add"], int(t["rows"][0]), sp["off"], sp["cnt"], sp["tok_src"], sp["key_add"], what + " tokens")
    _check_table(t["off2"], t["cnt2"], t["src2"], None, int(t["rows"][1]), sp["b_off"], sp["b_cnt"], sp["box_idx"], None, what + " boxes")


@pytest.mark.parametrize("n", [1, 5, 25, 1023, 1024, 1025, 2049, 32768, 70001])
def test_zk_plans_match_the_spec(n):
    T = 20
    lq, nb = _zk_inputs(n, T)
    sp = helpers.zk_plan_spec(lq, nb, T)
    three = _plan(1, n, T, lq, nb, T + 10, True)
    _check_zk(three, sp, "zk three-launch n=%d" % n)
    if n <= 1024:
        one = _plan(0, n, T, lq, nb, T + 10, True)
        _check_zk(one, sp, "zk one-block n=%d" % n)
        for k in one:
            assert np.array_equal(one[k], three[k]), (n, k)
    else:
        one = _plan(0, n, T, lq, nb, T + 10, True, refused=True)                       # launch_zk_plans_small takes no more than one block of pairs ...
        assert all(np.all(v == GUARD) for v in one.values()), n                        # ... and then launches nothing
    print("zk plans n=%d: %d of %d token rows and %d of %d boxes kept, tables exact" % (n, sp["rows"], n * (T + 10), sp["b_rows"], n * 10))


@pytest.mark.parametrize("T", [1, 32])
def test_zk_plans_at_the_text_length_limits(T):
    lq, nb = _zk_inputs(25, T)
    sp = helpers.zk_plan_spec(lq, nb, T)
    _check_zk(_plan(0, 25, T, lq, nb, T + 10, True), sp, "zk one-block T=%d" % T)
    _check_zk(_plan(1, 25, T, lq, nb, T + 10, True), sp, "zk three-launch T=%d" % T)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _lds_inputs(n):
    f6, l6 = lds_edge_pairs()
    r = np.random.default_rng(100 + n)
    f = np.zeros((n, 10, 2048), np.float32)
    lab = np.zeros((n, 10, 8), np.int64)
    for b in range(n):
        if b < 6 or b >= n - 2:                   # the edge pairs first, and two of them in the last workgroup
            f[b], lab[b] = f6[b % 6 if b < 6 else (4 + b - (n - 2))], l6[b % 6 if b < 6 else (4 + b - (n - 2))]
            continue
        live = r.integers(0, 11)
        f[b, np.arange(live), r.integers(0, 2048, live)] = 1.0     # one non-zero feature each, anywhere in the row
        cls = r.integers(0, 4, 10)
        lab[b] = cls[:, None] * 1000 + np.arange(8)
        lab[b, live:] = 0
    return f, lab


@pytest.mark.parametrize("n", [1, 3, 4, 5, 6, 1025])
def test_lds_plan_matches_the_spec(n):
    T = 20
    f, lab = _lds_inputs(n)
    sp = helpers.lds_plan_spec(f, lab, T)
    t = _plan(2, n, T, f, lab, T + 20, True)
    assert np.array_equal(t["src2"][:n * 10], sp["nz"].ravel().astype(np.int32)), n        # -0.0 is zero; 1e-30 and NaN are not
    rows = sp["rows"]
    err = np.abs(t["add"][:rows].astype(np.float64) - sp["key_add"]).max()
    print("lds plan n=%d: %d of %d rows kept; key_add vs np.log worst %.2e (bound 5e-7)" % (n, rows, n * (T + 20), err))
    # 5e-7: 2 ulp of fp32 at log 10 = 2.3 (ulp 2.4e-7) -- one for logf, one for the fp32 rounding of the fp64 value
    _check_table(t["off"], t["cnt"], t["src"], t["add"], int(t["rows"][0]), sp["off"], sp["cnt"], sp["tok_src"], sp["key_add"], "lds n=%d" % n, add_tol=5e-7)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _lx_inputs(n, T):
    m6, v6 = lx_edge_pairs()
    r = np.random.default_rng(200 + n)
    m = (r.random((n, T)) < 0.5).astype(np.int64)                       # non-prefix masks, CLS masked in half of them
    ln = r.integers(0, T + 1, n)
    pre = np.arange(T)[None, :] < ln[:, None]
    m[::2] = pre[::2]                                                    # prefix masks
    v = (r.random((n, 10)) < 0.4).astype(np.float32)
    k = min(n, 6)
    m[:k], v[:k] = m6[:k], v6[:k]
    if n > 12:
        m[-6:], v[-6:] = m6, v6
    return m, v


@pytest.mark.parametrize("n", [1, 6, 257, 1025, 30000])
def test_lx_plans_match_the_spec(n):
    T = 23
    m, v = _lx_inputs(n, T)
    sp = helpers.lx_plan_spec(m, v, T)
    t = _plan(3, n, T, m, v, T, True)
    _check_table(t["off"], t["cnt"], t["src"], t["add"], int(t["rows"][0]), sp["l_off"], sp["l_cnt"], sp["l_src"], sp["l_add"], "lxmert language n=%d" % n)
    _check_table(t["off2"], t["cnt2"], t["src2"], t["add2"], int(t["rows"][1]), sp["v_off"], sp["v_cnt"], sp["v_src"], sp["v_add"], "lxmert vision n=%d" % n)
    # the language-only plan of the distinct-query stage: same language tables, the vision buffers untouched
    l = lib.load()
    dm = _dev(m)
    bufs = dict(off=_ibuf(n), cnt=_ibuf(n), src=_ibuf(n * T), add=_fbuf(n * T), off2=_ibuf(n), cnt2=_ibuf(n), src2=_ibuf(n * 10), add2=_fbuf(n * 10), rows=_ibuf(4))
    p = {k: b.data_ptr() for k, b in bufs.items()}
    rc = l.mms_dbg_pack_plan(4, n, T, dm.data_ptr(), None, p["off"], p["cnt"], p["src"], p["add"], p["off2"], p["cnt2"], p["src2"], p["add2"], p["rows"], None)
    assert rc == 0, l.mms_global_error()
    g = {k: b.cpu().numpy() for k, b in bufs.items()}
    _check_table(g["off"], g["cnt"], g["src"], g["add"], int(g["rows"][0]), sp["l_off"], sp["l_cnt"], sp["l_src"], sp["l_add"], "lxmert language-only n=%d" % n)
    for k in ("off2", "cnt2", "src2", "add2"):
        assert np.all(g[k] == GUARD), (n, k)
    assert g["rows"][1] == GUARD
    print("lxmert plans n=%d: %d language and %d vision rows kept, tables exact" % (n, sp["l_rows"], sp["v_rows"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _dedup(kind, ids):
    l = lib.load()
    rows = ids.shape[0]
    d = _dev(ids)
    index, u32 = _ibuf(rows), _ibuf(rows * 8)
    u64 = torch.full((rows * 8,), GUARD, device="cuda", dtype=torch.int64)
    count = C.c_int32(-1)
    rc = l.mms_dbg_dedup(kind, d.data_ptr(), None, 0, rows, C.byref(count), index.data_ptr(), u32.data_ptr(), u64.data_ptr(), None, None)
    assert rc == 0, l.mms_global_error()
    return count.value, index.cpu().numpy(), u32.cpu().numpy().reshape(rows, 8), u64.cpu().numpy().reshape(rows, 8)


def _check_dedup(kind, ids, what):
    """np.unique(axis=0) is the spec: as many table rows as distinct tuples, pairwise distinct, and every row's index names its own tuple; the order of
    the table is unspecified"""
    count, index, u32, u64 = _dedup(kind, ids)
    want = len(np.unique(ids, axis=0))
    assert count == want, (what, count, want)
    assert index.min() >= 0 and index.max() < count, what
    assert np.array_equal(u64[index], ids.astype(np.int64)), what
    assert len(np.unique(u64[:count], axis=0)) == count, what
    assert np.array_equal(u32[:count], u64[:count].astype(np.int32)), what            # the 32-bit table holds the same tuples (truncated where they do not fit)
    assert np.all(u64[count:] == GUARD) and np.all(u32[count:] == GUARD), what
    return count


def _tuples(rows, distinct, seed, dtype):
    """`distinct` tuples that differ in their LAST id only (0: every row its own tuple), dealt to the rows at random, negative ids among them"""
    r = np.random.default_rng(seed)
    base = r.integers(-50, 30000, 8)
    if distinct == 0:
        pick = r.permutation(rows)
    else:
        pick = np.concatenate([np.arange(min(distinct, rows)), r.integers(0, distinct, max(rows - distinct, 0))])
        pick = r.permutation(pick)
    ids = np.tile(base, (rows, 1))
    ids[:, 7] = pick - 17
    return ids.astype(dtype)


# distinct tuples per call: every tuple equal, 33, 300, 5000, 0 = every row its own tuple (each workgroup's LDS table then holds 256 entries); the million-row
# call runs with few and with all-distinct tuples (wall time of the numpy side)
DEDUP_CASES = [(rows, d) for rows in (1, 255, 256, 257, 510, 100_000) for d in (1, 33, 300, 5000, 0)] + [(1_000_000, 33), (1_000_000, 0)]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("rows,distinct", DEDUP_CASES)
def test_label_dedup_is_np_unique(rows, distinct, kind):
    ids = _tuples(rows, distinct, rows + distinct, [np.int32, np.int64][kind])
    n = _check_dedup(kind, ids, "dedup kind %d rows %d distinct %d" % (kind, rows, distinct))
    print("label de-duplication (int%d) rows %d: %d distinct tuples, index and tables exact" % (32 << kind, rows, n))


def test_label_dedup_int64_ids_that_differ_above_bit_31():
    """The int64 path hashes the low halves: such tuples share one probe chain and only tuple_eq tells them apart (at most 64 of them, so the chain
    stays short)."""
    r = np.random.default_rng(9)
    hi = np.zeros((64, 8), np.int64)
    hi[np.arange(64), np.arange(64) % 8] = (np.arange(64) // 8 + 1) << 32            # 64 tuples, equal in every low half
    hi[1::2] = -hi[1::2]                                                             # negative high halves as well
    tup = hi + np.arange(8)[None, :] * 3 + 5
    ids = tup[r.integers(0, 64, 2000)]
    ids[:64] = tup
    assert len(np.unique(ids.astype(np.int32), axis=0)) == 1 and len(np.unique(ids, axis=0)) == 64
    assert _check_dedup(1, ids, "int64 high halves") == 64


def _qdedup(ids, mask):
    l = lib.load()
    rows, T = ids.shape
    di, dm = _dev(ids), _dev(mask)
    index, rows_of = _ibuf(rows), _ibuf(rows)
    count = C.c_int32(-1)
    rc = l.mms_dbg_dedup(2, di.data_ptr(), dm.data_ptr(), T, rows, C.byref(count), index.data_ptr(), None, None, rows_of.data_ptr(), None)
    assert rc == 0, l.mms_global_error()
    return count.value, index.cpu().numpy(), rows_of.cpu().numpy()


@pytest.mark.parametrize("rows", [2, 257, 30_000])
@pytest.mark.parametrize("share", ["one", "twelfth", "all"])
def test_query_dedup_numbers_by_first_occurrence(rows, share):
    """lxmert's distinct-query stage: index = the number of the query in the order of FIRST occurrence, rows_of[u] = the first row of query u, the same
    bits on every run.  Queries with equal ids and different masks are different queries."""
    T = 23
    Q = {"one": 1, "twelfth": max(rows // 12, 1), "all": rows}[share]
    r = np.random.default_rng(rows * 3 + Q)
    # Q distinct (ids, mask) keys in groups of three that share their ids and differ in the mask row alone: five live positions, eight live positions, and
    # five live positions one of which holds a 2 -- the same zero pattern as the first, so the two meet in ONE hash slot and only the comparison of the
    # mask VALUES keeps them apart (their key terms (1 - m) * -10000 differ)
    id_rows = r.integers(0, 30000, ((Q + 2) // 3, T)).astype(np.int64)
    id_rows[:, 0] = np.arange(len(id_rows))
    variant = np.arange(Q) % 3
    key_ids = id_rows[np.arange(Q) // 3]
    key_mask = (np.arange(T)[None, :] < np.where(variant == 1, 8, 5)[:, None]).astype(np.int64)
    key_mask[variant == 2, 4] = 2
    which = r.permutation(np.concatenate([np.arange(Q), r.integers(0, Q, rows - Q)]))      # repeats scattered, not contiguous
    ids, mask = key_ids[which], key_mask[which]
    # the spec: first occurrence
    key = np.concatenate([ids, mask], 1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                     # distinct keys in the order of their first rows
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    want_index, want_rows_of = rank[inv.ravel()], first[order]
    assert len(first) == Q
    count, index, rows_of = _qdedup(ids, mask)
    assert count == Q, (rows, share, count)
    assert np.array_equal(index, want_index), (rows, share)
    assert np.array_equal(rows_of[:Q], want_rows_of) and np.all(rows_of[Q:] == GUARD), (rows, share)
    again = _qdedup(ids, mask)
    assert again[0] == count and np.array_equal(again[1], index) and np.array_equal(again[2], rows_of), (rows, share)
    print("query de-duplication rows %d: %d distinct queries, first-occurrence numbering exact, second run identical" % (rows, Q))
