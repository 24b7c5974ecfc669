"""GPU suite: pipeline.EnsembleScorer.fit_joint_tsv_native -- one pass over a valid TSV file with the four member scores left on the device, then the
joint sweep -- against ensemble.fit_joint(where="host") on the member scores the pass hands out; then its winner through set_weights and
submission_tsv_native(gap=, tie=): the rows that are written grade to the fitted value."""
import numpy as np
import pytest

from helpers import small_cfg
from test_fit_filter_tsv_gpu import FILTERS, N_QUERIES, PER_QUERY, _valid_records
from test_ndcg_device_gpu import DENSE
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg, pipeline, scorers, weights

pytestmark = pytest.mark.gpu

GRID = np.r_[ensemble.weight_grid(4, 4), [ensemble.WEIGHTS]]             # 35 rows in steps of 1/4, and main.py's


def test_fit_joint_tsv_native_and_submission_with_the_fitted_pair(tmp_path):
    from test_feature_text_gather import TABLE, VOCAB
    lines, key = _valid_records()
    path = tmp_path / "valid.tsv"
    path.write_text("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n" + "".join(l + "\n" for l in lines), encoding="utf-8")
    path = str(path)
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), **DENSE.get(n, {})) for n, c in cfgs.items()}
    try:
        ens = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
        info, out = {}, {}
        got = ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, grid=GRID, filters=FILTERS, labels="ones", batch_pairs=64, info=info, scores_out=out)
        assert tuple(ens.weights) == tuple(ensemble.WEIGHTS)                 # the fit does not change the scorer
        with pytest.raises(ValueError):
            ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, labels="truth")
        qid, pid = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)[:2]
        ens.set_weights(got[0])
        rows = ens.submission_tsv_native(path, VOCAB, TABLE, batch_pairs=64, gap=got[1][0], tie=got[1][1])
    finally:
        for s in sc.values():
            s.close()
    assert info == {"path": "device", "flags": 0}
    assert np.array_equal(out["query_id"], qid) and np.array_equal(out["product_id"], pid) and out["members"].is_cuda
    mem = out["members"].cpu().numpy()
    assert mem.dtype == np.float32 and mem.shape == (4, N_QUERIES * PER_QUERY)
    want = ensemble.fit_joint(qid, pid, mem, key, GRID, FILTERS, where="host")
    print("\n[fit_joint_tsv_native] winner %s %s value %.4f at %s; best per filter: %s" % (want[0], want[1], want[2], want[3], np.round(want[4].max(0), 4).tolist()))
    assert got[4].shape == (len(GRID), len(FILTERS)) and got[4].tobytes() == want[4].tobytes()            # bit for bit
    assert got[2:4] == want[2:4] and repr(got[:2]) == repr(want[:2])
    iw, ig = got[3]
    assert got[0] == tuple(GRID[iw].tolist()) and got[1] == tuple(FILTERS[ig].tolist()) and got[2] == want[4].max() > 0.0
    # the fitted value is the grade of the submission rows of the fp64 host merge under the winner ...
    merged = ndcg.merge_members(mem, np.array(got[0]))
    codes = ndcg.submission_codes(qid, pid, merged, key, got[1][0], got[1][1])
    assert ndcg.ndcg_from_hist(ndcg.hist_from_codes(codes, 5), 5, len(key)) == got[2]
    # ... and of the rows the submission pass WROTE with the winner.  That pass ranks the fused call's fp32 merge; the shallow ensemble's member scores
    # lie much further apart than the rounding of either merge, so both merges rank and filter alike and the comparison is exact (no tolerance).
    wrote = ndcg.codes_of_rows(rows, set(np.unique(qid).tolist()), key, 5, False)
    assert np.array_equal(wrote, codes)
    assert ndcg.ndcg_from_hist(ndcg.hist_from_codes(wrote, 5), 5, len(key)) == got[2]
