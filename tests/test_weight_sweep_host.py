"""CPU suite: the host side of the weight fit -- ensemble.weight_grid, ndcg.ndcg_sweep_host (the reference of the device sweep) and
ensemble.fit_weights(where="host") -- against the host forms that were there before: ndcg_from_arrays / ndcg_codes / ndcg_from_codes / ndcg_from_hist
on the merged scores of each weight vector.  The merge is written out here a second time, in Python floats (main.py:59's own evaluation)."""
from math import comb

import numpy as np
import pytest

from ndcg_tables import fixture, random_table
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg

LEVELS = np.array([-0.5, -0.0, 0.0, 0.25, 0.5], np.float32)
SIGMA = (0.8, 0.8, 1.0, 1.2)


def golden_members():
    """The golden valid subset with four synthetic members: the fixture score plus seeded noise of 0.8 / 0.8 / 1.0 / 1.2 sigma, cast to fp32."""
    q, p, s, ans, _ = fixture()
    rng = np.random.default_rng(7)
    mem = np.stack([(s + f * s.std() * rng.standard_normal(len(s))).astype(np.float32) for f in SIGMA])
    return q, p, mem, ans


_GOLDEN = []


def golden_sweep():
    """(q, p, members, key, grid, values, hist) of the 286-vector grid on the golden subset by the host form: computed once, shared, read-only."""
    if not _GOLDEN:
        q, p, mem, ans = golden_members()
        grid = ensemble.weight_grid(4, 10)
        values, hist = ndcg.ndcg_sweep_host(q, p, mem, grid, ans, 5)
        for a in (mem, grid, values, hist):
            a.setflags(write=False)
        _GOLDEN.append((q, p, mem, ans, grid, values, hist))
    return _GOLDEN[0]


@pytest.mark.parametrize("members,steps", [(4, 4), (4, 10), (4, 20), (1, 3), (2, 5), (8, 2), (3, 1)])
def test_weight_grid(members, steps):
    g = ensemble.weight_grid(members, steps)
    assert g.dtype == np.float64 and g.shape == (comb(steps + members - 1, members - 1), members)
    assert g[0].tolist() == [0.0] * (members - 1) + [1.0] and g[-1].tolist() == [1.0] + [0.0] * (members - 1)
    c = g * steps
    assert np.array_equal(c, np.rint(c)) and (c >= 0).all() and (c.sum(1) == steps).all()
    rows = [tuple(r) for r in c.astype(int).tolist()]
    assert rows == sorted(set(rows))                                     # lexicographic, no repeats
    assert np.array_equal(g, np.array(rows, np.float64) / steps)


def test_weight_grid_sizes_of_the_issue():
    assert len(ensemble.weight_grid(4, 4)) == 35 and len(ensemble.weight_grid(4, 20)) == 1771 and len(ensemble.weight_grid()) == 1771
    with pytest.raises(ValueError):
        ensemble.weight_grid(0, 4)


def _python_merge(mem, w):
    """main.py:59 in Python floats, row by row"""
    out = []
    for r in range(mem.shape[1]):
        acc = float(w[0]) * float(mem[0, r])
        for m in range(1, mem.shape[0]):
            acc = acc + float(w[m]) * float(mem[m, r])
        out.append(acc)
    return np.array(out, np.float64)


@pytest.mark.parametrize("trial", [0, 3, 9, 14])
def test_sweep_host_equals_the_existing_host_forms_per_vector(trial):
    q, p, _, key = random_table(trial)
    mem = LEVELS[np.random.default_rng(50 + trial).integers(0, 5, (4, len(q)))]
    grid = np.concatenate([ensemble.weight_grid(4, 4)[::5], [[0, 0, 0, 0], [-1, 0, 0, 0], [1e-3, 0.5, 0.25, 0.2485]]])
    for k in (5, 1, 8):
        values, hist = ndcg.ndcg_sweep_host(q, p, mem, grid, key, k)
        assert values.dtype == np.float64 and hist.dtype == np.int64 and hist.shape == (len(grid), (k + 1) << k)
        for v, w in enumerate(grid):
            merged = _python_merge(mem, w)
            assert np.array_equal(merged, ndcg.merge_members(mem, w))
            codes = ndcg.ndcg_codes(q, p, merged, key, k)
            assert np.array_equal(hist[v], ndcg.hist_from_codes(codes, k))
            assert ndcg.ndcg_from_codes(codes, k) == ndcg.ndcg_from_arrays(q, p, merged, key, k)          # bitwise
            assert values[v] == ndcg.ndcg_from_hist(hist[v], k, len(key))                                  # bit for bit
            assert abs(values[v] - ndcg.ndcg_from_arrays(q, p, merged, key, k)) <= 1e-12                   # summation order only
    assert len({h.tobytes() for h in hist}) > 1                          # the grid moves the ranking


def test_bin_values_reproduce_ndcg_from_hist_over_all_bins():
    """the device's value formula: ALL bins in bin order, an empty bin adding +0.0"""
    _, _, _, _, _, values, hist = golden_sweep()
    t = ndcg.bin_values(5)
    assert t.shape == (192,) and (t >= 0).all() and not t.flags.writeable
    for v in (0, 100, 285):
        acc = 0.0
        for b in range(192):
            acc = acc + float(int(hist[v, b])) * float(t[b])
        assert acc / 200 == values[v]


def test_golden_subset_has_a_unique_interior_maximum():
    q, p, mem, ans, grid, values, hist = golden_sweep()
    assert len(grid) == 286 and (hist.sum(1) == 200).all()
    best = int(np.argmax(values))
    assert (values == values[best]).sum() == 1
    assert grid[best].tolist() == [0.4, 0.2, 0.2, 0.2] and values[best] == 0.6248067033286765
    fixed = ndcg.ndcg_sweep_host(q, p, mem, [ensemble.WEIGHTS], ans, 5)[0][0]
    assert fixed == 0.6217035015517502 and values[best] > fixed
    assert values.min() > 0.50 and values.max() < 0.63


def test_fit_weights_host():
    q, p, mem, ans, grid, values, _ = golden_sweep()
    info = {}
    w, value, index, vals = ensemble.fit_weights(q, p, mem, ans, grid, where="host", info=info)
    assert w == (0.4, 0.2, 0.2, 0.2) and value == values[index] == values.max() and np.array_equal(vals, values)
    assert info == {"path": "host", "flags": 0}
    with pytest.raises(ValueError):
        ensemble.fit_weights(q, p, mem, ans, grid, where="gpu")


def test_fit_weights_takes_the_first_row_on_a_tie():
    q, p, _, key = random_table(3)
    mem = np.zeros((4, len(q)), np.float32)
    w, value, index, vals = ensemble.fit_weights(q, p, mem, key, ensemble.weight_grid(4, 4), where="host")
    assert index == 0 and w == (0.0, 0.0, 0.0, 1.0) and (vals == value).all()


def test_missing_key_query_raises_keyerror_unless_allowed():
    q, p, _, key = random_table(4, with_missing=True)
    mem = LEVELS[np.random.default_rng(54).integers(0, 5, (4, len(q)))]
    grid = ensemble.weight_grid(4, 2)
    with pytest.raises(KeyError):
        ensemble.fit_weights(q, p, mem, key, grid, where="host")
    w, value, index, vals = ensemble.fit_weights(q, p, mem, key, grid, allow_missing=True, where="host")
    assert vals.shape == (10,) and value == vals.max()


def test_scorer_weights_can_be_set():
    """set_weights of the fused scorer needs no device: the ctypes array the fused call reads follows it"""
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import scorers
    s = scorers.EnsembleScorer.__new__(scorers.EnsembleScorer)
    s.set_weights((0.4, 0.2, 0.2, 0.2))
    assert s.weights == (0.4, 0.2, 0.2, 0.2) and list(s.w) == [np.float32(x) for x in (0.4, 0.2, 0.2, 0.2)]
    with pytest.raises(ValueError):
        s.set_weights((0.5, 0.5))
