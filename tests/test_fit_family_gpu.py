"""GPU suite: the two kernel families that share csrc/merge_members.h, and the two pack kernels that share the rank-flag fold, against EACH OTHER
(each is tested against its host form elsewhere).  On the table of tests/fit_family_tables.py with the single filter row (-inf, +inf)
mms_joint_sweep must give what mms_ndcg_weight_sweep gives: histograms entry for entry, values byte for byte, both flag words zero -- with all 65
weight vectors in one chunk and with one tile per chunk (the second tile has one live lane); M = 5 and 8 take the 8-wide records.  And on a repeated
(query, product) pair and on a reserved product id mms_filter_sweep and mms_joint_sweep report the same flag word."""
import numpy as np
import pytest
import torch

import fit_family_tables as T
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ndcg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", T.KS)
@pytest.mark.parametrize("M", T.MS)
def test_joint_sweep_without_a_filter_is_the_weight_sweep(M, k):
    q, p, mem, w, key = T.table(M)
    values, hist, status = (x.cpu().numpy() for x in ndcg.ndcg_sweep_device(q, p, mem, w, key, k))
    assert status[2] == 0 and hist.sum() == 65 * len(key)
    for chunk_tiles in (None, 1):
        jvalues, jhist, jstatus = (x.cpu().numpy() for x in ndcg.joint_sweep_device(q, p, mem, w, T.NO_FILTER, key, k, want_hist=True, chunk_tiles=chunk_tiles))
        assert jstatus[2] == 0 and jstatus.tolist() == status.tolist()
        assert jhist.shape == (65, 1, (k + 1) << k) and (jhist[:, 0] == hist).all()
        assert jvalues[:, 0].tobytes() == values.tobytes()                 # byte for byte


@pytest.mark.parametrize("what, flag", [("repeated pair", ndcg.FLAG_REPEATED_PAIR), ("reserved id", ndcg.FLAG_RESERVED_ID)])
def test_filter_and_joint_sweep_report_the_same_rank_flags(what, flag):
    q, p, mem, w, key = T.table(4)
    p = p.copy()
    a, b = np.flatnonzero(q == 15)[:2]                                     # two rows of the nine-row key query
    p[b] = p[a] if what == "repeated pair" else -1
    fstatus = ndcg.filter_sweep_device(q, p, ndcg.merge_members(mem, w[0]), T.NO_FILTER, key)[2].cpu().numpy()
    jstatus = ndcg.joint_sweep_device(q, p, mem, w[:1], T.NO_FILTER, key)[2].cpu().numpy()
    assert fstatus[2] == jstatus[2] == flag, (fstatus, jstatus)
