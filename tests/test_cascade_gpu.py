"""GPU suite: the cascade form of the fused ensemble (mms_score_ensemble_cascade; scorers.EnsembleScorer(cascade=), pipeline.EnsembleScorer(cascade_keep=))
against its contract in include/mmscore.h: stage 1 bit-equal to the full call's lxmert member, the selection that of ensemble.cascade_keep, stage 2
bit-equal to the full call on the gathered feed, exact zeros for pruned pairs, the merge expression, the ordering guarantee, keep >= the largest query
bit-equal to mms_score_ensemble, ragged waves, and the file-fed drivers with a query cut by a batch boundary."""
import numpy as np
import pytest
import torch

from helpers import small_cfg
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, pipeline, scorers, synth, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def members():
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    ws = {n: weights.make_weights(c) for n, c in cfgs.items()}
    made = []

    def make(**kw):
        sc = {n: scorers.make_scorer(cfgs[n], ws[n], **kw) for n in cfgs}
        made.append(sc)
        return scorers.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])

    yield cfgs, make
    for sc in made:
        for s in sc.values():
            s.close()


def _feed(cfgs, n_queries, cands, tag):
    ps = synth.make_pairs(n_queries, cands, vocab=cfgs["zk"].vocab, tag=tag)
    zb = synth.zk_batch(ps, cfgs["zk"].text_len)
    zb2 = synth.zk_batch(synth.sen2forest_variant(ps), cfgs["zk"].text_len)
    xb = synth.lxmert_batch(ps, cfgs["lxmert"].text_len)
    return {k: np.asarray(v) for k, v in pipeline.ensemble_feed(zb, zb2, xb).items()}, np.asarray(ps.query_id, np.int64)


def _contract(ens, feed, qid, keep):
    """every bit-equality of the contract for one call -> (merged, members, kept)"""
    merged, mem, kept = ens(feed, cascade=(qid, keep))
    full_merged, full_mem = ens(feed)
    assert kept.dtype == torch.bool and merged.shape == (len(qid),) and mem.shape == (4, len(qid))
    assert torch.equal(mem[3], full_mem[3])                                              # stage 1 = member 3 of the full call
    want, want_list = ensemble.cascade_keep(qid, mem[3].cpu().numpy(), keep)
    assert np.array_equal(kept.cpu().numpy(), want) and ens.last_kept == len(want_list)
    g_merged, g_mem = ens({k: v[want_list] for k, v in feed.items()})                    # the gathered feed as a call of its own
    for k in range(3):
        assert torch.equal(mem[k][kept], g_mem[k]), k
        pruned = mem[k][~kept]
        assert torch.equal(pruned, torch.zeros_like(pruned)) and not torch.signbit(pruned).any(), k
    w = ens.WEIGHTS
    exp = ((w[0] * mem[0] + w[1] * mem[1]) + w[2] * mem[2]) + w[3] * mem[3]
    assert torch.equal(merged, exp)
    m, kp = merged.cpu().numpy(), kept.cpu().numpy()
    for q in np.unique(qid):                                                             # the ordering guarantee
        if (~kp[qid == q]).any():
            assert m[(qid == q) & kp].min() >= m[(qid == q) & ~kp].max(), q
    return merged, mem, kept


def test_tiny_second_stage(members):
    """7 queries of 3..9 candidates, keep = 2: 14 pairs in stage 2, the skinny / split-K regimes."""
    cfgs, make = members
    ens = make()
    feed, qid = _feed(cfgs, 7, (3, 9), "/cas_a")
    merged, mem, kept = _contract(ens, feed, qid, 2)
    assert int(kept.sum()) == 14 < len(qid)
    # ragged waves in both stages: within the tolerance of the existing chunk test (fp32 summation order of the tiny-launch regime)
    ens5 = make(chunk_pairs=5)
    merged5, mem5, kept5 = ens5(feed, cascade=(qid, 2))
    assert torch.equal(kept5, kept)
    assert (merged5 - merged).abs().max() < 2e-5 and (mem5 - mem).abs().max() < 2e-5


def test_second_stage_on_the_lanes_and_determinism(members):
    """10 queries of 28..30 candidates, keep = 10: ~290 pairs in stage 1 and 100 pairs = 3 000 token rows in stage 2, the fused-attention regime, members
    on their lanes; two identical calls are bit-identical."""
    cfgs, make = members
    ens = make()
    feed, qid = _feed(cfgs, 10, (28, 30), "/cas_b")
    merged, mem, kept = _contract(ens, feed, qid, 10)
    assert int(kept.sum()) == 100
    merged_b, mem_b, kept_b = ens(feed, cascade=(qid, 10))
    assert torch.equal(merged, merged_b) and torch.equal(mem, mem_b) and torch.equal(kept, kept_b)
    # keep >= the largest query: mms_score_ensemble bit for bit, both outputs
    full_merged, full_mem = ens(feed)
    merged30, mem30, kept30 = ens(feed, cascade=(qid, 30))
    assert kept30.all() and ens.last_kept == len(qid)
    assert torch.equal(merged30, full_merged) and torch.equal(mem30, full_mem)
    # cascade=None is today's path and return value
    out = ens(feed, cascade=None)
    assert isinstance(out, tuple) and len(out) == 2 and torch.equal(out[0], full_merged) and torch.equal(out[1], full_mem)
    no_mem = ens(feed, members=False, cascade=(qid, 10))
    assert no_mem[1] is None and torch.equal(no_mem[0], merged) and torch.equal(no_mem[2], kept)


def test_interleaved_queries_and_argument_errors(members):
    cfgs, make = members
    ens = make()
    feed, qid = _feed(cfgs, 5, (4, 6), "/cas_c")
    perm = np.random.default_rng(3).permutation(len(qid))
    _contract(ens, {k: v[perm] for k, v in feed.items()}, qid[perm], 2)                  # rows of a query need not be adjacent
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib
    with pytest.raises(lib.MmsError):
        ens(feed, cascade=(qid, 0))
    with pytest.raises(ValueError):
        ens(feed, cascade=(qid[:-1], 2))
    bad = qid.copy()
    bad[0] = -1                                                                          # reserved id: flagged, served by the exact form
    merged, mem, kept = ens(feed, cascade=(bad, 1))
    full_merged, full_mem = ens(feed)
    assert kept.all() and torch.equal(merged, full_merged) and torch.equal(mem, full_mem)


def test_file_fed_cascade(tmp_path):
    """submission_tsv_native(cascade_keep=) with batches that cut a query: the rows are those of ensemble.submission_rows on the scores assembled from
    cascade_keep(parts = the pass's batch offsets) and the pass's own members; cascade_curve_tsv_native: device values equal host values, as floats."""
    from test_feature_text_gather import TABLE, VOCAB
    from test_fit_filter_tsv_gpu import N_QUERIES, PER_QUERY, _valid_records
    from test_ndcg_device_gpu import DENSE
    lines, key = _valid_records()
    path = tmp_path / "valid.tsv"
    path.write_text("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n" + "".join(l + "\n" for l in lines), encoding="utf-8")
    path = str(path)
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), **DENSE.get(n, {})) for n, c in cfgs.items()}
    KEEP, BATCH = 3, 20                                                                  # 8 records per query: every batch boundary but each second cuts one
    try:
        ens = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
        info, info2, out = {}, {}, {}
        qid, pid, merged, mem = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=BATCH, cascade_keep=KEEP, info=info)
        rows = ens.submission_tsv_native(path, VOCAB, TABLE, batch_pairs=BATCH, cascade_keep=KEEP, info=info2)
        ev = ens.evaluate_tsv_native(path, VOCAB, TABLE, key, labels="ones", batch_pairs=BATCH, cascade_keep=KEEP)
        keeps = [1, KEEP, PER_QUERY]
        dev = ens.cascade_curve_tsv_native(path, VOCAB, TABLE, key, keeps, labels="ones", batch_pairs=BATCH, scores_out=out)
    finally:
        for s in sc.values():
            s.close()
    n = N_QUERIES * PER_QUERY
    offsets = info["batch_offsets"]
    assert offsets[0] == 0 and offsets[-1] == n == len(qid) and info == info2 and any(o % PER_QUERY for o in offsets)
    mem = np.stack(mem)
    kept, kept_list = ensemble.cascade_keep(qid, mem[3], KEEP, parts=offsets)
    assert info["cascade_kept"] == len(kept_list) > N_QUERIES * KEEP and info["cascade_pairs"] == n    # a cut query keeps up to KEEP per part
    assert not mem[:3, ~kept].any() and (mem[:3, kept] > 0).all()
    w = np.array(ens.weights, np.float32)
    exp = ((w[0] * mem[0] + w[1] * mem[1]) + w[2] * mem[2]) + w[3] * mem[3]
    assert exp.dtype == np.float32 and np.array_equal(merged, exp.astype(np.float64))
    assert rows == ensemble.submission_rows(qid, pid, exp.astype(np.float64))
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ndcg
    assert ev == ndcg.ndcg_from_arrays(qid, pid, exp.astype(np.float64), key, 5)
    # the curve: one full pass, then device values == host values
    assert out["batch_offsets"] == offsets and np.array_equal(out["query_id"], qid)
    host = ensemble.cascade_curve(qid, pid, out["members"].cpu().numpy(), key, keeps, ens.weights, parts=offsets, where="host")
    assert dev == host
    assert [c["keep"] for c in dev] == keeps and dev[-1]["fraction"] == 1.0 and dev[-1]["changed"] == 0
    assert dev[1]["kept"] == len(kept_list)                                              # lxmert's scores do not depend on the other members: the same selection
    print("\n[cascade curve] %s" % dev)
