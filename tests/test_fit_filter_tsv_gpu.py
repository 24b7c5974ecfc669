"""GPU suite: pipeline.EnsembleScorer.fit_filter_tsv_native -- one pass over a valid TSV file with the merged scores left on the device, then the
filter sweep -- against ndcg.filter_sweep_host on the scores the pass hands out; submission_tsv_native(gap=, tie=) on the device against the host
rank form with the same constants, and with the defaults against the call without the arguments."""
import numpy as np
import pytest

from helpers import small_cfg
from test_ndcg_device_gpu import DENSE
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg, pipeline, scorers, weights

pytestmark = pytest.mark.gpu

INF = float("inf")
N_QUERIES, PER_QUERY = 24, 8
# (no filter), gaps around the spread of a shallow model's scores at main.py's tie, "everything ties", and a tie of 0 that nothing survives
FILTERS = np.array([(-INF, INF), (0.0, 1e-5), (1e-4, 1e-5), (1e-3, 1e-5), (1e-2, 1e-5), (0.1, 1e-5), (ensemble.GAP, ensemble.TIE), (0.0, INF), (0.5, 0.0)])


def _valid_records():
    """24 queries x 8 records: even queries carry 8 product ids used nowhere else; odd queries 4 of their own and 4 from a pool of 10 shared ids, so a
    shared product survives under its best query at most and an odd query has 4 .. 8 survivors depending on the gap.  The key names three of every
    query's products and one that no record carries."""
    from test_feature_text_gather import TABLE
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer as F
    rng = np.random.default_rng(83)
    classes = [int(k) for k in TABLE]
    shared = 900000 + np.arange(10)
    lines, key, nxt = [], {}, 5000
    for qi in range(N_QUERIES):
        if qi % 2 == 0:
            pids = list(range(nxt, nxt + 8)); nxt += 8
        else:
            pids = [int(x) for x in rng.choice(shared, 4, replace=False)] + list(range(nxt, nxt + 4)); nxt += 4
            pids = [pids[i] for i in rng.permutation(8)]
        key[str(300 + qi)] = [int(x) for x in rng.choice(pids, 3, replace=False)] + [999999]
        for x in pids:
            nb = int(rng.integers(1, 12))
            h, w = int(rng.integers(50, 1200)), int(rng.integers(50, 1200))
            boxes = rng.uniform(0, 1, (nb, 4)).astype(np.float32) * np.array([h, w, h, w], np.float32)
            feats = rng.standard_normal((nb, 2048)).astype(np.float32)
            lines.append(F.encode_record(int(x), h, w, boxes, feats, rng.choice(classes, nb), "blue shirt %d" % qi, 300 + qi))
    return lines, key


def test_fit_filter_tsv_native_and_submission_with_the_fitted_filter(tmp_path):
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
        got = ens.fit_filter_tsv_native(path, VOCAB, TABLE, key, filters=FILTERS, labels="ones", batch_pairs=64, info=info, scores_out=out)
        info_a, out_a = {}, {}
        got_a = ens.fit_filter_tsv_native(path, VOCAB, TABLE, key, filters=FILTERS, batch_pairs=64, info=info_a, scores_out=out_a)      # labels="answer"
        with pytest.raises(ValueError):
            ens.fit_filter_tsv_native(path, VOCAB, TABLE, key, labels="truth")
        qid, pid, merged = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)[:3]
        rows = {}
        for name, kw in (("plain", {}), ("defaults", dict(gap=ensemble.GAP, tie=ensemble.TIE)), ("fit_dev", dict(gap=got[0][0], tie=got[0][1])),
                         ("fit_host", dict(gap=got[0][0], tie=got[0][1], rank="host")), ("g0_dev", dict(gap=0.0, tie=1e-5)),
                         ("g0_host", dict(gap=0.0, tie=1e-5, rank="host"))):
            rows[name] = ens.submission_tsv_native(path, VOCAB, TABLE, batch_pairs=64, **kw)
    finally:
        for s in sc.values():
            s.close()
    assert info == {"path": "device", "flags": 0}
    assert np.array_equal(out["query_id"], qid) and np.array_equal(out["product_id"], pid) and out["score"].is_cuda
    score = out["score"].cpu().numpy()
    assert score.dtype == np.float64 and score.shape == (N_QUERIES * PER_QUERY,) and np.array_equal(score, merged)      # labels="ones": score_tsv_native's feed
    want_values, _, want_codes = ndcg.filter_sweep_host(qid, pid, score, FILTERS, key, 5)
    print("\n[fit_filter_tsv_native] values per filter: %s" % np.round(want_values, 4).tolist())
    assert got[3].tobytes() == want_values.tobytes()                         # bit for bit
    index = int(np.argmax(want_values))
    assert got[2] == index and got[1] == want_values[index] and got[0] == tuple(FILTERS[index].tolist())
    assert want_values[0] > 0.0 == want_values[8] and (want_codes[8] == ndcg.CODE_DROPPED).all()
    # the default label feed (labels="answer": the zk members see the answer key's relevance of every record): graded on the scores of its own pass
    assert info_a == {"path": "device", "flags": 0} and np.array_equal(out_a["query_id"], qid) and np.array_equal(out_a["product_id"], pid)
    score_a = out_a["score"].cpu().numpy()
    assert score_a.dtype == np.float64 and score_a.shape == score.shape
    want_a = ndcg.filter_sweep_host(qid, pid, score_a, FILTERS, key, 5)[0]
    index_a = int(np.argmax(want_a))
    assert got_a[3].tobytes() == want_a.tobytes() and got_a[2] == index_a and got_a[0] == tuple(FILTERS[index_a].tolist())
    same = lambda a, b: list(a) == list(b) and a == {k_: list(v) for k_, v in b.items()}
    assert same(rows["defaults"], rows["plain"]) and same(rows["plain"], ensemble.submission_rows(qid, pid, score))
    for name, (g, t) in (("fit", got[0]), ("g0", (0.0, 1e-5))):
        want = ensemble.submission_rows(qid, pid, score, g, t)
        assert same(rows[name + "_dev"], want) and same(rows[name + "_host"], want), name
    # the constants reach the ranking: at gap 0 a shared product survives under its best query, at main.py's 0.92 under none
    assert rows["g0_dev"] != rows["plain"]
