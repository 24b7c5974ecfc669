"""The numpy statements of the pack plans (tests/helpers.py: zk_plan_spec, lds_plan_spec, lx_plan_spec) are code that can be wrong, so they are
held to the oracle here, on the CPU: their masks are the reference models' masks, and one attention sub-layer in fp64 over the rows a spec keeps,
with the spec's key_add, gives the kept rows' outputs of the same sub-layer over the dense rows with the dense mask.  tests/test_plan_dedup_kernels_gpu.py
then compares the kernels' tables with these specs."""
import numpy as np
import pytest

import helpers
from oracle import np_models as O

T_ZK, T_LDS, T_LX = 20, 20, 23
HID = 768


def _att_weights(seed):
    r = np.random.default_rng(seed)
    w = [r.standard_normal((HID, HID)) / np.sqrt(HID) * 1.5 for _ in range(3)]
    b = [r.standard_normal(HID) * 0.1 for _ in range(3)]
    return w[0], b[0], w[1], b[1], w[2], b[2]


def _sublayer(q_in, kv_in, aw, key_add):
    return O.attention(q_in[None], kv_in[None], *aw, key_add=None if key_add is None else np.asarray(key_add, np.float64)[None])[0]


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


# six edge pairs per model
ZK_EDGE = dict(len_query=np.array([0, 1, T_ZK, 7, 0, 12]), num_boxes=np.array([0, 10, 0, 3, 4, 10]))


def test_zk_spec_mask_is_the_models_mask():
    lq, nb = np.meshgrid(np.arange(0, T_ZK + 1), np.arange(0, 11), indexing="ij")
    lq, nb = lq.ravel(), nb.ravel()
    sp = helpers.zk_plan_spec(lq, nb, T_ZK)
    mask = O.zk_key_mask({"len_query_": lq, "num_boxes": nb}, T_ZK)
    assert np.array_equal(sp["dense_add"], O._key_add(mask, np.float32))
    # out-of-range lengths mean what sequence_mask makes of them: nothing / everything
    lo = helpers.zk_plan_spec(np.array([-3, T_ZK + 5]), np.array([-1, 13]), T_ZK)
    assert np.array_equal(lo["dense_add"], O._key_add(O.zk_key_mask({"len_query_": np.array([-3, T_ZK + 5]), "num_boxes": np.array([-1, 13])}, T_ZK), np.float32))


def test_zk_spec_rows_reproduce_the_dense_sublayer():
    sp = helpers.zk_plan_spec(ZK_EDGE["len_query"], ZK_EDGE["num_boxes"], T_ZK)
    S = T_ZK + 10
    aw = _att_weights(1)
    x = np.random.default_rng(2).standard_normal((6, S, HID))
    worst = 0.0
    for b in range(6):
        dense = _sublayer(x[b], x[b], aw, sp["dense_add"][b])
        r = slice(sp["off"][b], sp["off"][b] + sp["cnt"][b])
        tok = sp["tok_src"][r] - b * S
        assert sp["tok_src"][r][0] == b * S                                  # the pooler's CLS row is kept, first
        assert np.all(sp["tok_src"][r] // S == b) and np.all(np.diff(tok) > 0)
        packed = _sublayer(x[b, tok], x[b, tok], aw, sp["key_add"][r])
        worst = max(worst, _rel(packed, dense[tok]))
        # the box plan: exactly the kept boxes
        br = slice(sp["b_off"][b], sp["b_off"][b] + sp["b_cnt"][b])
        assert np.array_equal(sp["box_idx"][br], b * 10 + (tok[tok >= T_ZK] - T_ZK))
    print("zk: packed vs dense sub-layer, worst relative difference %.2e" % worst)
    assert worst < 1e-9


def lds_edge_pairs():
    """feats [6,10,2048], labelfeat [6,10,8]: nothing merges / no box at all / one class / classes repeating non-adjacently with a zero box in the
    middle / lone tiny, -0.0 and NaN features / ids equal below bit 32 and negative ids."""
    r = np.random.default_rng(3)
    f = np.zeros((6, 10, 2048), np.float32)
    lab = np.zeros((6, 10, 8), np.int64)
    f[0] = r.standard_normal((10, 2048)); lab[0] = np.arange(80).reshape(10, 8) + 100
    # pair 1: all zero
    f[2] = r.standard_normal((10, 2048)); lab[2] = np.arange(8) + 7
    f[3, [0, 1, 2, 4, 6]] = r.standard_normal((5, 2048)); lab[3] = (np.array([1, 2, 1, 3, 2, 1, 4, 0, 0, 3])[:, None] * 10 + np.arange(8))
    f[4, 1, 2047] = 1e-30; f[4, 3, 5] = -0.0; f[4, 6, 1000] = np.nan; lab[4, :7] = np.array([5, 5, 6, 6, 5, 7, 7])[:, None]
    f[5, :4] = r.standard_normal((4, 2048))
    lab[5] = 9
    lab[5, 1, 7] = 9 + (1 << 32); lab[5, 2, 0] = 9 + (1 << 40); lab[5, 3, 7] = 9 + (1 << 32); lab[5, 4] = -9; lab[5, 5] = -9; lab[5, 6, 3] = -(1 << 33) + 9
    return f, lab


def test_lds_spec_rows_reproduce_the_dense_sublayer():
    f, lab = lds_edge_pairs()
    sp = helpers.lds_plan_spec(f, lab, T_LDS)
    S = T_LDS + 20
    assert list(sp["cnt"]) == [T_LDS + 20, T_LDS + 2, T_LDS + 11, T_LDS + 6 + 5, T_LDS + 3 + 4, T_LDS + 5 + 5]
    assert list(sp["nz"][4]) == [False, True, False, False, False, False, True, False, False, False]
    aw = _att_weights(4)
    r = np.random.default_rng(5)
    worst = 0.0
    for b in range(6):
        # token rows as the model makes them: a function of the box features / of the label tuple alone (no position, no type)
        x = r.standard_normal((S, HID))
        zero_row, by_tuple = r.standard_normal(HID), {}
        for j in range(10):
            if not sp["nz"][b, j]:
                x[T_LDS + j] = zero_row
            x[T_LDS + 10 + j] = by_tuple.setdefault(tuple(lab[b, j]), r.standard_normal(HID))
        dense = _sublayer(x, x, aw, None)
        rr = slice(sp["off"][b], sp["off"][b] + sp["cnt"][b])
        tok = sp["tok_src"][rr] - b * S
        assert tok[0] == 0 and np.all(np.diff(tok) > 0) and np.all(sp["tok_src"][rr] // S == b)
        packed = _sublayer(x[tok], x[tok], aw, sp["key_add"][rr])
        worst = max(worst, _rel(packed, dense[tok]))
    print("lds: merged vs dense sub-layer, worst relative difference %.2e" % worst)
    assert worst < 1e-9


def lx_edge_pairs():
    """input_mask [6,23], visual mask [6,10]: prefix / non-prefix / CLS masked / nothing live / everything live / one live."""
    m = np.zeros((6, T_LX), np.int64)
    v = np.zeros((6, 10), np.float32)
    m[0, :9] = 1; v[0, :4] = 1
    m[1, [0, 2, 3, 11, 22]] = 1; v[1, [1, 5, 9]] = 1
    m[2, 1:6] = 1; v[2, 3:] = 1
    # pair 3: nothing live in either stream
    m[4] = 1; v[4] = 1
    m[5, 17] = 1; v[5, 9] = 1
    return m, v


def test_lx_spec_mask_and_rows():
    m, v = lx_edge_pairs()
    sp = helpers.lx_plan_spec(m, v, T_LX)
    assert np.array_equal(sp["l_dense"], O._key_add(m, np.float32)) and np.array_equal(sp["v_dense"], O._key_add(v, np.float32))
    aw = _att_weights(6)
    r = np.random.default_rng(7)
    xl, xv = r.standard_normal((6, T_LX, HID)), r.standard_normal((6, 10, HID))
    worst = 0.0
    for b in range(6):
        lr = slice(sp["l_off"][b], sp["l_off"][b] + sp["l_cnt"][b])
        vr = slice(sp["v_off"][b], sp["v_off"][b] + sp["v_cnt"][b])
        lt, vt = sp["l_src"][lr] - b * T_LX, sp["v_src"][vr] - b * 10
        assert lt[0] == 0 and np.all(np.diff(lt) > 0) and np.all(np.diff(vt) > 0)            # CLS kept, token order
        assert np.all((lt >= 0) & (lt < T_LX)) and np.all((vt >= 0) & (vt < 10))
        self_d = _sublayer(xl[b], xl[b], aw, sp["l_dense"][b])
        self_p = _sublayer(xl[b, lt], xl[b, lt], aw, sp["l_add"][lr])
        cross_d = _sublayer(xl[b], xv[b], aw, sp["v_dense"][b])                                # language queries, vision keys
        cross_p = _sublayer(xl[b, lt], xv[b, vt], aw, sp["v_add"][vr])
        back_d = _sublayer(xv[b], xl[b], aw, sp["l_dense"][b])                                 # vision queries, language keys
        back_p = _sublayer(xv[b, vt], xl[b, lt], aw, sp["l_add"][lr])
        worst = max(worst, _rel(self_p, self_d[lt]), _rel(cross_p, cross_d[lt]), _rel(back_p, back_d[vt]))
    print("lxmert: packed vs dense sub-layers, worst relative difference %.2e" % worst)
    assert worst < 1e-9
    lang_only = helpers.lx_plan_spec(m, None, T_LX)
    assert "v_src" not in lang_only and np.array_equal(lang_only["l_src"], sp["l_src"])


@pytest.mark.parametrize("delta", [3e-5, 5e-5])
def test_f8_excused_marks_exactly_the_neighbourhood_of_the_boundaries(delta):
    from oracle import fp8
    x = np.array([1.0, 1.0625, 1.0625 + delta / 2, 1.0625 - 2 * delta, 2.0 ** -10, 2.0 ** -10 + 2 * delta, -3.125, -3.125 - delta / 2, 0.0, 440.0])
    exc, lo, hi = helpers.f8_excused(x, delta)
    assert list(exc) == [False, True, True, False, True, False, True, True, False, False]
    assert (lo[1], hi[1]) == (1.0, 1.125) and (lo[4], hi[4]) == (0.0, 2.0 ** -9) and (lo[6], hi[6]) == (-3.25, -3.0)
    v = fp8.e4m3_decode(np.arange(256))
    assert np.isnan(v[0x7F]) and np.isnan(v[0xFF]) and np.isfinite(np.delete(v, [0x7F, 0xFF])).all()
    assert v[0x7E] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0xB8] == -1.0
    fin = np.delete(v, [0x7F, 0xFF])
    assert np.array_equal(fp8.e4m3_round(fin), fin)
