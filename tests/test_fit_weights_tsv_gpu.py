"""GPU suite: pipeline.EnsembleScorer.fit_weights_tsv_native -- one pass over a valid TSV file with the member scores left on the device, then the
weight sweep -- against ensemble.fit_weights(where="host") on the member scores that score_tsv_native reads back; set_weights / the constructor's
``weights`` against the fused call's own merge expression."""
import numpy as np
import pytest
import torch

from helpers import small_cfg
from test_ndcg_device_gpu import DENSE, N_QUERIES, PER_QUERY, _valid_records
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, pipeline, scorers, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def valid_tsv(tmp_path_factory):
    lines, key = _valid_records()
    path = tmp_path_factory.mktemp("fit") / "valid.tsv"
    path.write_text("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n" + "".join(l + "\n" for l in lines), encoding="utf-8")
    return str(path), key


def _merge4(mem, w):
    """k_merge4's expression in fp32"""
    f = np.float32
    return ((f(w[0]) * mem[0] + f(w[1]) * mem[1]) + f(w[2]) * mem[2]) + f(w[3]) * mem[3]


def test_fit_weights_tsv_native_and_set_weights(valid_tsv):
    from test_feature_text_gather import TABLE, VOCAB
    path, key = valid_tsv
    cfgs = {n: small_cfg(n) for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), **DENSE.get(n, {})) for n, c in cfgs.items()}
    grid = ensemble.weight_grid(4, 4)
    try:
        ens = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
        info, out, ans_out = {}, {}, {}
        got = ens.fit_weights_tsv_native(path, VOCAB, TABLE, key, grid=grid, labels="ones", batch_pairs=64, info=info, scores_out=out)
        got_ans = ens.fit_weights_tsv_native(path, VOCAB, TABLE, key, grid=grid, batch_pairs=64, scores_out=ans_out)
        assert ens.weights == pipeline.EnsembleScorer.WEIGHTS                # the fit does not touch the scorer
        qid, pid, merged, mem = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)
        with pytest.raises(ValueError):
            ens.fit_weights_tsv_native(path, VOCAB, TABLE, key, labels="truth")
        ens.set_weights(got[0])
        merged_fit = ens.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)[2]
        ens_ctor = pipeline.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"], weights=got[0])
        merged_ctor = ens_ctor.score_tsv_native(path, VOCAB, TABLE, batch_pairs=64)[2]
    finally:
        for s in sc.values():
            s.close()
    mem = np.stack(mem)
    assert mem.shape == (4, N_QUERIES * PER_QUERY) and mem.dtype == np.float32
    assert info == {"path": "device", "flags": 0}
    assert np.array_equal(out["query_id"], qid) and np.array_equal(out["product_id"], pid) and out["members"].is_cuda
    assert np.array_equal(out["members"].cpu().numpy(), mem)                 # labels="ones": the feed of score_tsv_native
    want = ensemble.fit_weights(qid, pid, mem, key, grid, where="host")
    assert got[:3] == want[:3] and got[3].tobytes() == want[3].tobytes()
    want_ans = ensemble.fit_weights(qid, pid, ans_out["members"].cpu().numpy(), key, grid, where="host")
    assert got_ans[:3] == want_ans[:3] and got_ans[3].tobytes() == want_ans[3].tobytes()
    assert np.abs(merged - _merge4(mem, pipeline.EnsembleScorer.WEIGHTS)).max() <= 1e-6
    assert ens.weights == got[0] and got[0] != pipeline.EnsembleScorer.WEIGHTS
    assert np.abs(merged_fit - _merge4(mem, got[0])).max() <= 1e-6 and np.array_equal(merged_fit, merged_ctor)
    assert not np.array_equal(merged_fit, merged)                           # the new weights reached the fused call
