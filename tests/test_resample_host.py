"""CPU suite: the host forms of the resampled joint fit -- the byte codes (ndcg.joint_codes_host), the replicate selection
(ndcg.resample_select_host), the count generators (ensemble.kfold_counts / bootstrap_counts) and ensemble.fit_joint_resampled(where="host") --
against the existing grader: a replicate of 0/1 counts is ndcg.ndcg_from_codes of ndcg.submission_codes on the sub-key, bit for bit."""
import functools

import numpy as np
import pytest

import joint_tables
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg

DROPS = (4, tuple([12] * 16))                                            # table(4, [12] * 16): 4 816 codes of -2 under weights() x filters(13)


@functools.lru_cache(maxsize=None)
def _codes(trial, rows_per_query=None, n_weights=None, n_filters=13):
    """-> (byte codes [W, G, Qa] of joint_codes_host, int32 codes [W, G, Qa] of submission_codes): computed once, read-only."""
    q, p, mem, key = joint_tables.table(trial, None if rows_per_query is None else list(rows_per_query))
    w, f = joint_tables.weights(4, n_weights), joint_tables.filters(n_filters)
    with np.errstate(invalid="ignore"):
        got = ndcg.joint_codes_host(q, p, mem, w, f, key)
        want = np.stack([[ndcg.submission_codes(q, p, ndcg.merge_members(mem, wv), key, g[0], g[1]) for g in f] for wv in w])
    got.setflags(write=False)
    want.setflags(write=False)
    return got, want


def test_byte_values_are_the_code_values_and_zero_elsewhere():
    for k in (1, 3, 5):
        t = ndcg.byte_values(k)
        assert t.dtype == np.float64 and t.shape == (256,) and t[0xFF] == 0.0 and t[0xFE] == 0.0 and (t >= 0).all() and np.isfinite(t).all()
        for b in range(256):
            ideal, mask = b >> 5, b & 31
            want = ndcg._code_value(mask | ideal << 8, k) if ideal <= k and mask < 1 << k else 0.0
            assert t[b] == want, (k, b)
    with pytest.raises(ValueError):
        ndcg.byte_values(6)


def test_byte_codes_equal_submission_codes_under_the_byte_mapping_with_dropped_queries():
    got, want = _codes(*DROPS)
    assert got.dtype == np.uint8 and got.shape == want.shape == (37, 13, 16)
    assert int((want == ndcg.CODE_DROPPED).sum()) == 4816
    assert np.array_equal(got == 0xFE, want == ndcg.CODE_DROPPED) and not (got == 0xFF).any()
    graded = want >= 0
    assert np.array_equal(got[graded] >> 5, want[graded] >> 8) and np.array_equal(got[graded] & 31, want[graded] & 0xFF)
    assert np.array_equal(ndcg.byte_codes(want), got)


def test_a_key_query_without_rows_is_0xff_under_allow_missing():
    q, p, mem, key = joint_tables.table(1)
    key = dict(key)
    key[999999] = [5]
    w, f = joint_tables.weights(4, 5), joint_tables.filters(3)
    with pytest.raises(KeyError):
        ndcg.joint_codes_host(q, p, mem, w, f, key)
    got = ndcg.joint_codes_host(q, p, mem, w, f, key, allow_missing=True)
    assert (got[:, :, -1] == 0xFF).all() and not (got[:, :, :-1] == 0xFF).any()
    best, fit, ev, _, _ = ndcg.resample_select_host(got, np.ones((1, len(key)), np.uint8), np.ones((1, len(key)), np.uint8))
    v, g = divmod(int(best[0]), 3)
    assert fit[0] == ev[0] == ndcg.ndcg_from_codes(ndcg.submission_codes(q, p, ndcg.merge_members(mem, w[v]), key, f[g, 0], f[g, 1], 5, True))


@pytest.mark.parametrize("table", [DROPS, (1, None)])
def test_all_ones_replicate_is_ndcg_from_codes_per_item_bit_for_bit(table):
    got, want = _codes(*table)
    W, G, Qa = got.shape
    ones = np.ones((1, Qa), np.uint8)
    probes = list(range(0, W * G, max(1, W * G // 200)))
    best, fit, ev, pf, pe = ndcg.resample_select_host(got, ones, ones, 5, probes)
    per_item = np.array([ndcg.ndcg_from_codes(want.reshape(W * G, Qa)[it]) for it in range(W * G)])
    assert pf[0].tobytes() == per_item[probes].tobytes() == pe[0].tobytes()
    assert int(best[0]) == int(np.argmax(per_item)) and fit[0] == per_item.max() == ev[0]


def test_a_sub_key_replicate_is_the_grader_on_the_sub_key():
    q, p, mem, key = joint_tables.table(1)
    w, f = joint_tables.weights(4), joint_tables.filters(13)
    got, _ = _codes(1)
    Qa = len(key)
    rng = np.random.default_rng(5)
    fit_rows = (rng.random((3, Qa)) < 0.6).astype(np.uint8)
    probes = [0, 14, 37 * 13 - 1, 200]
    best, fit, ev, pf, pe = ndcg.resample_select_host(got, fit_rows, (1 - fit_rows).astype(np.uint8), 5, probes)
    names = list(key)
    for r in range(3):
        for rows, out in ((fit_rows[r], pf[r]), (1 - fit_rows[r], pe[r])):
            sub = {names[i]: key[names[i]] for i in np.flatnonzero(rows)}
            for j, it in enumerate(probes):
                v, g = divmod(it, 13)
                with np.errstate(invalid="ignore"):
                    codes = ndcg.submission_codes(q, p, ndcg.merge_members(mem, w[v]), sub, f[g, 0], f[g, 1])
                assert out[j] == ndcg.ndcg_from_codes(codes), (r, it)


def test_first_at_maximum_with_duplicated_weight_rows():
    got, _ = _codes(1, None, 80)                                         # weights(4, 80): the 37 rows cycled, every item occurs again 37 rows later
    W, G, Qa = got.shape
    assert np.array_equal(got[:37], got[37:74])
    cf, ce = ensemble.kfold_counts(Qa, 5, 2, seed=3)
    best, fit, ev, _, _ = ndcg.resample_select_host(got, cf, ce)
    vals = ndcg.byte_values(5)[got.reshape(W * G, Qa)]
    for r in range(len(cf)):
        acc = np.zeros(W * G)
        for i in range(Qa):
            acc = acc + float(cf[r, i]) * vals[:, i]
        full = acc / float(cf[r].sum())
        at_max = np.flatnonzero(full == full.max())
        assert len(at_max) >= 2 and int(best[r]) == int(at_max[0]) < 37 * G and fit[r] == full.max()


def test_empty_rows_and_block_size():
    got, _ = _codes(1)
    Qa = got.shape[2]
    cf, ce = ensemble.bootstrap_counts(Qa, 7, seed=1)
    cf, ce = cf.copy(), ce.copy()
    cf[2] = 0                                                            # an empty fit row: no winner
    ce[4] = 0                                                            # an empty eval row: NaN from 0.0 / 0.0
    cf[5, 0] = 255
    a = ndcg.resample_select_host(got, cf, ce, 5, [3, 9999])
    assert a[0][2] == -1 and np.isnan(a[1][2]) and np.isnan(a[2][2]) and np.isnan(a[3][2, 0]) and not np.isnan(a[4][2, 0])
    assert a[0][4] >= 0 and np.isnan(a[2][4]) and not np.isnan(a[1][4]) and np.isnan(a[3][:, 1]).all() and np.isnan(a[4][:, 1]).all()
    for block in (1, 3):
        b = ndcg.resample_select_host(got, cf, ce, 5, [3, 9999], block=block)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    with pytest.raises(ValueError):
        ndcg.resample_select_host(got, cf.astype(np.int32), ce)
    with pytest.raises(ValueError):
        ndcg.resample_select_host(got, cf[:, :-1], ce[:, :-1])


def test_fold_counts():
    for qa, folds, repeats in ((58, 5, 1), (16, 4, 3), (7, 7, 2)):
        cf, ce = ensemble.kfold_counts(qa, folds, repeats, seed=2)
        assert cf.dtype == ce.dtype == np.uint8 and cf.shape == ce.shape == (folds * repeats, qa)
        assert ((cf + ce) == 1).all()
        assert (ce.reshape(repeats, folds, qa).sum(1) == 1).all()        # every key query in exactly one eval fold per repeat
        sizes = ce.sum(1)
        assert sizes.max() - sizes.min() <= 1
    assert np.array_equal(ensemble.kfold_counts(58, 5, 1, 0)[1][np.random.default_rng(0).permutation(58) % 5, np.arange(58)], np.ones(58, np.uint8))
    assert not np.array_equal(ensemble.kfold_counts(58, 5, 2, 0)[1][:5], ensemble.kfold_counts(58, 5, 2, 0)[1][5:])
    with pytest.raises(ValueError):
        ensemble.kfold_counts(4, 5)


def test_bootstrap_counts():
    cf, ce = ensemble.bootstrap_counts(58, 40, seed=7)
    assert cf.dtype == ce.dtype == np.uint8 and cf.shape == ce.shape == (40, 58)
    assert (cf.sum(1) == 58).all() and np.array_equal(ce, (cf == 0).astype(np.uint8))
    again = ensemble.bootstrap_counts(58, 40, seed=7)
    assert np.array_equal(cf, again[0]) and np.array_equal(ce, again[1])
    assert not np.array_equal(cf, ensemble.bootstrap_counts(58, 40, seed=8)[0])
    with pytest.raises(ValueError):
        ensemble.bootstrap_counts(58, 0)


def test_fit_joint_resampled_on_the_host():
    q, p, mem, key = joint_tables.table(1)
    w, f = joint_tables.weights(4), joint_tables.filters(13)
    info = {}
    with np.errstate(invalid="ignore"):
        got = ensemble.fit_joint_resampled(q, p, mem, key, w, f, scheme="kfold", folds=5, repeats=1, seed=0, probes=[(35, 1)], where="host", info=info)
        want = ensemble.fit_joint(q, p, mem, key, w, f, where="host")
    assert info == {"path": "host", "flags": 0}
    whole = got["whole"]
    assert whole[2:4] == want[2:4] and whole[4].tobytes() == want[4].tobytes() and repr(whole[:2]) == repr(want[:2])
    assert got["probes"] == [want[3], (35, 1)] and got["probe_fit"].shape == got["probe_eval"].shape == (5, 2)
    assert got["winners"].shape == (5, 2) and got["fit_values"].shape == got["eval_values"].shape == (5,)
    items = got["winners"][:, 0] * 13 + got["winners"][:, 1]
    print("\n[fit_joint_resampled host] winners %s heldout %.4f optimism %.4f agreement %.2f" % (items.tolist(), got["heldout"], got["optimism"], got["agreement"]))
    assert len(set(items.tolist())) > 1                                  # the folds do not all select the same item
    codes, _ = _codes(1)
    cf, ce = ensemble.kfold_counts(len(key), 5, 1, 0)
    assert np.array_equal(got["count_fit"], cf) and np.array_equal(got["count_eval"], ce)
    ref = ndcg.resample_select_host(codes, cf, ce, 5, [want[3][0] * 13 + want[3][1], 35 * 13 + 1])
    assert np.array_equal(items, ref[0])
    for name, r in zip(("fit_values", "eval_values", "probe_fit", "probe_eval"), ref[1:]):
        assert got[name].tobytes() == r.tobytes(), name
    assert got["heldout"] == float(np.mean(ref[2])) and got["optimism"] == float(np.mean(ref[1] - ref[2]))
    assert got["agreement"] == float(np.mean(ref[0] == want[3][0] * 13 + want[3][1]))
    assert (got["fit_values"] >= got["probe_fit"][:, 0]).all()           # a replicate's winner is at least as good on it as the whole-key winner
    boot = ensemble.fit_joint_resampled(q, p, mem, key, w[:3], f[:2], scheme="bootstrap", replicates=6, seed=1, where="host")
    assert boot["winners"].shape == (6, 2) and np.array_equal(boot["count_fit"], ensemble.bootstrap_counts(len(key), 6, 1)[0])
    with pytest.raises(ValueError, match="coarser grid"):
        ensemble.fit_joint_resampled(q, p, mem, key, w, f, where="host", code_budget=1000)
    with pytest.raises(ValueError):
        ensemble.fit_joint_resampled(q, p, mem, key, w, f, where="host", scheme="jackknife")
    with pytest.raises(ValueError):
        ensemble.fit_joint_resampled(q, p, mem, key, w, f, where="host", probes=[(37, 0)])
