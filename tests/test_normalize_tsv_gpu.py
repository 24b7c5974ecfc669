"""GPU suite: the ``normalize`` keyword of the file-fed ensemble drivers (pipeline.EnsembleScorer).  fit_joint_tsv_native(normalize="zscore") against
the host fit on the host-normalised members of the pass; its winner through set_weights and submission_tsv_native(normalize="zscore", gap=, tie=):
the rows are those of the host-normalised, host-merged scores on either rank form, and they grade to the fitted value BIT FOR BIT -- the fit and
the submission share one merge.  The batches hold 60 pairs and a query 8, so batch boundaries cut queries: the groups are those of the whole file."""
import numpy as np
import pytest

from helpers import small_cfg
from test_fit_filter_tsv_gpu import FILTERS, N_QUERIES, PER_QUERY, _valid_records
from test_fit_joint_tsv_gpu import GRID
from test_ndcg_device_gpu import DENSE
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg, pipeline, scorers, weights

pytestmark = pytest.mark.gpu

BATCH = 60


def test_normalized_fit_and_submission_share_one_merge(tmp_path):
    from test_feature_text_gather import TABLE, VOCAB
    lines, key = _valid_records()
    path = tmp_path / "valid.tsv"
    path.write_text("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n" + "".join(l + "\n" for l in lines), encoding="utf-8")
    path = str(path)
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), **DENSE.get(n, {})) for n, c in cfgs.items()}
    same = lambda a, b: list(a) == list(b) and a == {k_: list(v) for k_, v in b.items()}
    try:
        ens = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
        kw = dict(labels="ones", batch_pairs=BATCH)
        # today's results first, before any normalised call ...
        plain_fit = ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, grid=GRID, filters=FILTERS, **kw)
        plain_rows = ens.submission_tsv_native(path, VOCAB, TABLE, batch_pairs=BATCH)
        offsets = {}
        ens.cascade_curve_tsv_native(path, VOCAB, TABLE, key, [PER_QUERY], scores_out=offsets, **kw)
        # ... then the normalised fit, and its winner through the two drivers that merge
        info, out = {}, {}
        got = ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, grid=GRID, filters=FILTERS, info=info, scores_out=out, normalize="zscore", **kw)
        got_w = ens.fit_weights_tsv_native(path, VOCAB, TABLE, key, grid=GRID, normalize="rank", **kw)
        got_r = ens.fit_joint_resampled_tsv_native(path, VOCAB, TABLE, key, grid=GRID, filters=FILTERS, normalize="zscore", folds=4, repeats=1, **kw)
        assert tuple(ens.weights) == tuple(ensemble.WEIGHTS)
        ens.set_weights(got[0])
        sub = dict(batch_pairs=BATCH, gap=got[1][0], tie=got[1][1], normalize="zscore")
        sub_info = {}
        rows_dev = ens.submission_tsv_native(path, VOCAB, TABLE, info=sub_info, **sub)
        rows_host = ens.submission_tsv_native(path, VOCAB, TABLE, rank="host", **sub)
        ev_info, ev_out = {}, {}
        value_dev = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, normalize="zscore", info=ev_info, scores_out=ev_out, **kw)
        value_host = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, normalize="zscore", metric="host", **kw)
        for call in (lambda: ens.submission_tsv_native(path, VOCAB, TABLE, cascade_keep=4, **sub),
                     lambda: ens.evaluate_tsv_native(path, VOCAB, TABLE, key, normalize="rank", cascade_keep=4, **kw),
                     lambda: ens.submission_tsv_native(path, VOCAB, TABLE, normalize="softmax"),
                     lambda: ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, normalize="softmax")):
            with pytest.raises(ValueError):
                call()
        # ... and the un-normalised drivers again, with the keyword at its default and spelled out
        ens.set_weights(ensemble.WEIGHTS)
        again_fit = ens.fit_joint_tsv_native(path, VOCAB, TABLE, key, grid=GRID, filters=FILTERS, normalize="none", **kw)
        again_rows = ens.submission_tsv_native(path, VOCAB, TABLE, batch_pairs=BATCH, normalize="none")
    finally:
        for s in sc.values():
            s.close()
    cuts = offsets["batch_offsets"]
    assert cuts == [0, 60, 120, 180, 192] and any(c % PER_QUERY for c in cuts)            # queries 7, 15 and 22 are cut by a batch boundary
    assert info == {"path": "device", "flags": 0, "normalize": "zscore"} and sub_info["normalize"] == "zscore"
    qid, pid, mem = out["query_id"], out["product_id"], out["members"].cpu().numpy()
    assert mem.dtype == np.float32 and mem.shape == (4, N_QUERIES * PER_QUERY)
    nm = ensemble.normalize_members(qid, mem, "zscore")
    want = ensemble.fit_joint(qid, pid, nm, key, GRID, FILTERS, where="host")
    print("\n[fit_joint_tsv_native zscore] winner %s %s value %.4f at %s (raw scale: %s %s %.4f)" % (want[0], want[1], want[2], want[3], plain_fit[0], plain_fit[1], plain_fit[2]))
    assert got[4].tobytes() == want[4].tobytes() and got[2:4] == want[2:4] and repr(got[:2]) == repr(want[:2])
    want_w = ensemble.fit_weights(qid, pid, ensemble.normalize_members(qid, mem, "rank"), key, GRID, where="host")
    assert got_w[3].tobytes() == want_w[3].tobytes() and repr(got_w[:3]) == repr(want_w[:3])
    assert got_r["whole"][4].tobytes() == want[4].tobytes() and repr(got_r["whole"][:4]) == repr(want[:4])
    # the submission ranks the host-normalised, host-merged scores -- on both rank forms ...
    merged = ndcg.merge_members(nm, np.array(got[0]))
    want_rows = ensemble.submission_rows(qid, pid, merged, got[1][0], got[1][1])
    assert same(rows_dev, want_rows) and same(rows_host, want_rows)
    # ... and what it wrote grades to the value the fit reported for the winner, bit for bit: the seam between the fit's double merge and the fused
    # call's fp32 merge is closed
    wrote = ndcg.codes_of_rows(rows_dev, set(np.unique(qid).tolist()), key, 5, False)
    assert np.array_equal(wrote, ndcg.submission_codes(qid, pid, merged, key, got[1][0], got[1][1]))
    print("[seam] fitted %r, rows written grade to %r (per code) / %r (per bin)" % (got[2], ndcg.ndcg_from_codes(wrote, 5), ndcg.ndcg_from_hist(ndcg.hist_from_codes(wrote, 5), 5, len(key))))
    # The fit reports the PER-BIN sum of the per-query values (ndcg_from_hist: the sweep's histogram); ndcg_from_codes adds the same terms in key
    # order, and two orders of one sum of len(key) terms in [0, 1] differ by at most len(key) roundings of the total (0.4482815528199874 against
    # ...873 on joint_tables.table(4, [12] * 16) under zscore, on the host alone).  So: the codes are equal one by one (above), the per-bin sum is
    # the fitted value bit for bit, and the per-code sum lies within that bound.
    assert ndcg.ndcg_from_hist(ndcg.hist_from_codes(wrote, 5), 5, len(key)) == got[2] == want[4].max() > 0.0
    assert abs(ndcg.ndcg_from_codes(wrote, 5) - got[2]) <= len(key) * 2.0 ** -53 * got[2]
    # evaluate_tsv_native(normalize=) grades the same merge without the filter, the same float on both metrics
    assert ev_info["normalize"] == "zscore" and ev_out["score"].dtype.is_floating_point and ev_out["score"].cpu().numpy().tobytes() == merged.tobytes()
    assert value_dev == value_host == ndcg.ndcg_from_arrays(qid, pid, merged, key, 5)
    # without the keyword nothing moved
    assert again_fit[4].tobytes() == plain_fit[4].tobytes() and repr(again_fit[:4]) == repr(plain_fit[:4])
    assert same(again_rows, plain_rows)
    assert got[4].tobytes() != plain_fit[4].tobytes()
