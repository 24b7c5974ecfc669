"""CPU suite: what ties the fit family together.  The weight sweep and the joint sweep share ONE merge (csrc/merge_members.h on the device,
ndcg.merge_members on the host): with the single filter row (-inf, +inf) every row survives and the submission row is the unfiltered top-5, so
ndcg.joint_sweep_host must equal ndcg.ndcg_sweep_host -- histograms entry for entry, values bit for bit (tests/test_fit_family_gpu.py asks the same
of the two kernels).  And the fit_* functions share their argument checks and the tuple of fit_joint."""
import numpy as np
import pytest

import fit_family_tables as T
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg


@pytest.mark.parametrize("k", T.KS)
@pytest.mark.parametrize("M", T.MS)
def test_joint_sweep_without_a_filter_is_the_weight_sweep(M, k):
    q, p, mem, w, key = T.table(M)
    assert np.signbit(mem[0, ::3]).all() and (mem[0, ::3] == 0).all() and np.unique(q, return_counts=True)[1].tolist() == list(T.ROWS_PER_QUERY)
    values, hist = ndcg.ndcg_sweep_host(q, p, mem, w, key, k)
    jvalues, jhist = ndcg.joint_sweep_host(q, p, mem, w, T.NO_FILTER, key, k)
    assert jhist.shape == (65, 1, (k + 1) << k) and (jhist[:, 0] == hist).all()
    assert jvalues[:, 0].tobytes() == values.tobytes()                     # bit for bit
    assert len({h.tobytes() for h in hist}) > 1 or M == 1                  # the weights move the grading


def _fits(where):
    q, p, mem, w, key = T.table(4)
    score = ndcg.merge_members(mem, w[0])
    f = ensemble.filter_grid(4)
    return {"fit_weights": lambda grid=w, filters=None: ensemble.fit_weights(q, p, mem, key, grid, where=where),
            "fit_filter": lambda grid=None, filters=f: ensemble.fit_filter(q, p, score, key, filters, where=where),
            "fit_joint": lambda grid=w, filters=f: ensemble.fit_joint(q, p, mem, key, grid, filters, where=where),
            "fit_joint_resampled": lambda grid=w, filters=f: ensemble.fit_joint_resampled(q, p, mem, key, grid, filters, folds=2, repeats=1, where=where)}


@pytest.mark.parametrize("name", ["fit_weights", "fit_filter", "fit_joint", "fit_joint_resampled"])
def test_fit_functions_share_their_argument_checks(name):
    with pytest.raises(ValueError, match="where must be 'host' or 'device'"):
        _fits("gpu")[name]()
    fit = _fits("host")[name]
    if name != "fit_filter":
        with pytest.raises(ValueError, match="^%s: the grid must be" % name):
            fit(grid=np.zeros((0, 4)))
    if name != "fit_weights":
        with pytest.raises(ValueError, match="^%s: the filters must be" % name):
            fit(filters=np.zeros((0, 2)))


def test_resampled_whole_is_fit_joint():
    fits = _fits("host")
    whole, want = fits["fit_joint_resampled"]()["whole"], fits["fit_joint"]()
    assert whole[:4] == want[:4] and whole[4].shape == want[4].shape and whole[4].tobytes() == want[4].tobytes()
