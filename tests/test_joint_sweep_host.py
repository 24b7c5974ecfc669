"""CPU suite: the host form of the joint sweep (ndcg.joint_sweep_host) and ensemble.fit_joint(where="host").  The host form is by definition the loop
of ndcg.filter_sweep_host over ndcg.merge_members per weight vector; here it is held against that loop written out, against the weight sweep's host
form on the "no filter" column, against the reference's dict walk, and the joint optimum is shown to lie strictly above the sequential one."""
import numpy as np
import pytest

import filter_tables
import joint_tables
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg

INF = float("inf")


@pytest.mark.parametrize("trial,k", [(0, 5), (1, 5), (2, 3), (3, 1)])
def test_row_v_is_the_filter_sweep_of_the_merge(trial, k):
    q, p, mem, key = joint_tables.table(trial)
    w, f = joint_tables.weights(4, 7), joint_tables.filters(13)
    with np.errstate(invalid="ignore"):
        values, hist = ndcg.joint_sweep_host(q, p, mem, w, f, key, k)
        assert values.shape == (7, 13) and values.dtype == np.float64 and hist.shape == (7, 13, (k + 1) << k) and hist.dtype == np.int64
        for v in range(len(w)):
            want_values, want_hist, _ = ndcg.filter_sweep_host(q, p, ndcg.merge_members(mem, w[v]), f, key, k)
            assert values[v].tobytes() == want_values.tobytes() and np.array_equal(hist[v], want_hist), v
    assert len({h.tobytes() for h in hist.reshape(-1, hist.shape[-1])}) > 20          # weights and filters both move the grading


def test_no_filter_column_is_the_weight_sweep():
    q, p, mem, key = joint_tables.table(2)
    w = joint_tables.weights(4)
    f = np.array([(0.5, 1e-5), (-INF, INF)])
    values, hist = ndcg.joint_sweep_host(q, p, mem, w, f, key, 5)
    want_values, want_hist = ndcg.ndcg_sweep_host(q, p, mem, w, key, 5)
    assert np.array_equal(hist[:, 1], want_hist) and values[:, 1].tobytes() == want_values.tobytes()
    assert not np.array_equal(hist[:, 0], want_hist)


def test_codes_equal_the_dict_walk_on_the_merged_score():
    q, p, mem, key = joint_tables.table(3)
    w, f = joint_tables.weights(4), joint_tables.filters(13)
    _, hist = ndcg.joint_sweep_host(q, p, mem, w[[0, 17, 35, 36]], f, key, 5)
    for i, v in enumerate((0, 17, 35, 36)):
        merged = ndcg.merge_members(mem, w[v])
        for g in (0, 1, 4, 9):
            if np.isnan(f[g]).any():
                continue
            codes = filter_tables.submission_codes_dict(q, p, merged, key, f[g, 0], f[g, 1])
            assert np.array_equal(hist[i, g], ndcg.hist_from_codes(codes, 5)), (v, g)


def test_fit_joint_on_the_host_takes_the_first_row_major_maximum():
    q, p, mem, key = joint_tables.table(1)
    w, f = joint_tables.weights(4, 9), joint_tables.filters(13)
    w = np.r_[w, w]                                                       # every value occurs again later: the first one must win
    f = np.r_[f, f[::-1]]
    info = {}
    with np.errstate(invalid="ignore"):
        weights, (gap, tie), value, (iw, ig), values = ensemble.fit_joint(q, p, mem, key, w, f, where="host", info=info)
        want = ndcg.joint_sweep_host(q, p, mem, w, f, key)[0]
    assert info == {"path": "host", "flags": 0}
    assert values.shape == (18, 26) and values.tobytes() == want.tobytes()
    assert (iw, ig) == divmod(int(np.argmax(want)), 26) and iw < 9 and ig < 13
    assert value == want[iw, ig] == want.max() and weights == tuple(w[iw].tolist())
    assert repr((gap, tie)) == repr((float(f[ig, 0]), float(f[ig, 1])))
    assert (want == want.max()).sum() >= 4
    # lists of members, and an AnswerKey-free dict with str keys, are taken as fit_weights takes them
    again = ensemble.fit_joint(list(q), list(p), [m for m in mem], key, w, f, where="host")
    assert again[3] == (iw, ig) and again[4].tobytes() == values.tobytes()


def test_the_joint_optimum_lies_strictly_above_the_sequential_one():
    """The table of the issue (trial 4, 16 key queries of 12 rows): fitting the weights on the unfiltered ranking and then the filter for that one merge
    gives 0.3875; the best (weights, filter) pair of the same two grids gives 0.4249."""
    q, p, mem, key = joint_tables.table(4, rows_per_query=[12] * 16)
    grid = ensemble.weight_grid(4, 4)
    f = filter_tables.grid(13)
    f = f[~np.isnan(f).any(1)]
    w_seq = ensemble.fit_weights(q, p, mem, key, grid, where="host")[0]
    seq = ensemble.fit_filter(q, p, ndcg.merge_members(mem, np.array(w_seq)), key, f, where="host")[1]
    weights, flt, joint, (iw, ig), values = ensemble.fit_joint(q, p, mem, key, grid, f, where="host")
    assert joint > seq
    assert abs(seq - 0.3875) < 5e-5 and abs(joint - 0.4249) < 5e-5, (seq, joint)
    assert values[int(np.flatnonzero((grid == np.array(w_seq)).all(1))[0])].max() == seq          # the sequential answer is one row of the joint table


def test_argument_errors():
    q, p, mem, key = joint_tables.table(0)
    w, f = joint_tables.weights(4, 3), joint_tables.filters(4)
    with pytest.raises(ValueError):
        ndcg.joint_sweep_host(q, p, mem, w, f, key, 6)                    # a submission row holds five products
    with pytest.raises(ValueError):
        ndcg.joint_sweep_host(q, p, mem, w[:, :3], f, key)
    with pytest.raises(ValueError):
        ndcg.joint_sweep_host(q, p, mem, w, f[:, :1], key)
    with pytest.raises(ValueError):
        ndcg.joint_sweep_host(q, p, np.zeros((9, len(q)), np.float32), np.zeros((2, 9)), f, key)
    with pytest.raises(ValueError):
        ndcg.joint_sweep_host(q, p, mem, np.zeros((ndcg.MAX_JOINT_ITEMS // 4 + 1, 4)), f, key)
    with pytest.raises(ValueError):
        ensemble.fit_joint(q, p, mem, key, w, f, where="gpu")
    with pytest.raises(ValueError):
        ensemble.fit_joint(q, p, mem, key, w[:0], f, where="host")
    with pytest.raises(ValueError):
        ensemble.fit_joint(q, p, mem, key, w, f[:0], where="host")
    missing = dict(key)
    missing[999999] = [5]
    with pytest.raises(KeyError):
        ensemble.fit_joint(q, p, mem, missing, w, f, where="host")
    got = ensemble.fit_joint(q, p, mem, missing, w, f, where="host", allow_missing=True)
    assert got[4].shape == (3, 4)
    values, hist = ndcg.joint_sweep_host(q, p, mem, w[:0], f, key)
    assert values.shape == (0, 4) and hist.shape == (0, 4, 192)
