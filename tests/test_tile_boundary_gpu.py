"""GPU suite: the tile boundary of the persistent ping-pong GEMM (gemm_pp.hip) and the bounded grid of the LayerNorm fall-back (rowops.hip).

A persistent workgroup issues its next tile's first two LDS-DMA stages ahead of the epilogue's stores and, where every row of the wave's tile half is
live, passes the boundary on a COUNTED wait (the stores stay in flight under the next tile's first stage); a wave of a ragged tile drains its queue.
A count that is too generous would let a wave read a stage that has not landed: wrong tiles, on the second and later tiles of a workgroup only.  So
every case here has more tiles than the chip has CUs (256: at least two tiles per workgroup) and a ragged last row tile, and runs in BOTH walk
directions.  Forward, the ragged tiles are the last ones of their workgroups: every boundary crossed is a counted one.  Reversed (what every second
big launch of a forward does), they are the FIRST tiles of their workgroups and full tiles follow: those workgroups cross a boundary whose upper wave
row (live rows) counts while the lower one (fewer than 32 stores issued, or none) must drain, and then run a chained stage 0 behind a drained queue.
Each result is compared BIT FOR BIT with an engine that has no boundary: the 128 x 256 tile engine, or the same kernel on row ranges of a single
persistent round."""
import ctypes as C

import numpy as np
import pytest
import torch

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib, weights

pytestmark = pytest.mark.gpu

ENG_TILE, ENG_PP_PERSIST = lib.ENGINES["ENG_TILE"], lib.ENGINES["ENG_PP_PERSIST"]
F32, PLANES, HEAD_MAJOR = 0, 1, 2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _operands(tag, M, K, N):
    a = weights.normal("tb/a/%s/%d/%d" % (tag, M, K), (M, K), 1)
    w = weights.round_to_bf16(weights.normal("tb/w/%s/%d/%d" % (tag, N, K), (N, K), 1, 1.0 / np.sqrt(K)))
    bias = weights.normal("tb/b/%s/%d" % (tag, N), (N,), 1, 0.1)
    return a, w, bias


def _gemm_ex(da, M, K, dw, N, db, act, out_kind, engine, m_live, reverse=0):
    l = lib.load()
    out = torch.full((M * N,), 7.0, device="cuda", dtype=torch.float32)
    rc = l.mms_dbg_gemm_ex(da.data_ptr(), M, K, dw.data_ptr(), N, db.data_ptr(), act, out_kind, engine, m_live, reverse, out.data_ptr(), None)
    assert rc == 0, l.mms_global_error()
    return out.cpu().numpy()


# (M, K, N, activation, output, live rows or -1): 256-row tiles x 256-column tiles > 256 CUs in every case
BOUNDARY_CASES = [
    (8000, 768, 3072, lib.ACT_GELU_TANH, PLANES, -1),       # FFN-up: 32 x 12 tiles, the last row tile has 64 live rows (its lower wave row: none)
    (8080, 768, 3072, lib.ACT_GELU_TANH, PLANES, -1),       # ... 144 live rows: the lower wave row issues stores for 16 of its 128 rows
    (8192, 768, 3072, lib.ACT_GELU_TANH, PLANES, 7300),     # device-side row count below the padded M: 29 x 12 tiles, the last with 132 live rows
    (23000, 3072, 768, lib.ACT_NONE, F32, -1),              # N = 768 without the LayerNorm epilogue: 90 x 3 tiles
    (23000, 768, 768, lib.ACT_NONE, PLANES, 22600),
    (12000, 768, 2304, lib.ACT_NONE, HEAD_MAJOR, -1),       # QKV: fp32 head-major output, 47 x 9 tiles
    (12032, 768, 2304, lib.ACT_NONE, HEAD_MAJOR, 11111),
]


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("case", BOUNDARY_CASES)
def test_persistent_engine_with_several_tiles_per_workgroup_equals_the_tile_engine_bit_for_bit(case, reverse):
    M, K, N, act, out_kind, m_live = case
    assert ((M if m_live < 0 else m_live) + 255) // 256 * (N // 256) > 256 and (M if m_live < 0 else m_live) % 256
    a, w, bias = _operands("pp", M, K, N)
    da, dw, db = _dev(a), _dev(w), _dev(bias)
    ref = _gemm_ex(da, M, K, dw, N, db, act, out_kind, ENG_TILE, m_live)
    got = _gemm_ex(da, M, K, dw, N, db, act, out_kind, ENG_PP_PERSIST, m_live, reverse)
    assert np.array_equal(got, ref), (case, reverse, float(np.abs(got - ref).max()), int((got != ref).sum()))
    live = M if m_live < 0 else m_live
    shaped = ref.reshape(N // 64, M, 64) if out_kind == HEAD_MAJOR else ref.reshape(1, M, N)
    assert np.all(shaped[:, live:] == 0.0) and np.all(np.abs(shaped[:, :live]).max(axis=2) > 0.0)      # rows past the live count are not written; every other one is
    if m_live < 0 and out_kind != HEAD_MAJOR:      # ... and the tile engine itself is the kernel the other suites check against fp64
        rows = np.array([0, 255, 256, M // 2, M - 1])
        v = a[rows].astype(np.float64) @ w.astype(np.float64).T + bias
        if act == lib.ACT_GELU_TANH:
            v = 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (v + 0.044715 * v ** 3)))
        assert np.abs(ref.reshape(M, N)[rows] - v).max() < 2e-4 * max(1.0, np.abs(v).max())


def _gemm_ln(l, da, dr, M, K, dw, db, dg, dbe, row0=0, reverse=0):
    out = torch.empty((M, 768), device="cuda", dtype=torch.float32)
    mode = C.c_int32(0)
    rc = l.mms_dbg_gemm_ln(da.data_ptr() + row0 * K * 4, M, K, dw.data_ptr(), db.data_ptr(), dr.data_ptr() + row0 * 768 * 4, dg.data_ptr(), dbe.data_ptr(), 2 * reverse,
                           out.data_ptr(), C.byref(mode), None)
    assert rc == 0, l.mms_global_error()
    assert mode.value == 1, "the launch fell back to the two-kernel route (mode %d)" % mode.value
    return out.cpu().numpy()


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("M,K", [(45000, 768), (30000, 3072)])
def test_fused_layernorm_gemm_over_several_rounds_equals_single_round_launches_bit_for_bit(M, K, reverse):
    """The LayerNorm-fused kernel has no second engine to be compared with bit for bit (its variance is one-pass), but a row's result does not depend on
    the launch it is computed in: a launch of R row panels <= one persistent round (85 panels on 256 CUs) never crosses a tile boundary.  45 000 rows
    = 176 panels = three rounds, 30 000 rows = 118 panels = two; the last panel is ragged in both (200 / 48 live rows).  Reversed, that panel runs in
    the FIRST round and its three workgroups go on to full panels: the boundary on which one wave row counts and the other drains."""
    l = lib.load()
    a = weights.normal("tb/ln/a/%d/%d" % (M, K), (M, K), 1)
    w = weights.round_to_bf16(weights.normal("tb/ln/w/%d" % K, (768, K), 1, 1.0 / np.sqrt(K)))
    bias = weights.normal("tb/ln/b", (768,), 1, 0.1)
    r = weights.normal("tb/ln/r/%d" % M, (M, 768), 1) + 0.3
    gamma = weights.normal("tb/ln/g", (768,), 1, 0.1, 1.0)
    beta = weights.normal("tb/ln/be", (768,), 1, 0.1)
    da, dw, db, dr, dg, dbe = _dev(a), _dev(w), _dev(bias), _dev(r), _dev(gamma), _dev(beta)
    got = _gemm_ln(l, da, dr, M, K, dw, db, dg, dbe, 0, reverse)
    chunk = 64 * 256                  # 64 panels: inside one round
    assert M > 85 * 256 and M % 256
    for row0 in range(0, M, chunk):
        rows = min(chunk, M - row0)
        part = _gemm_ln(l, da, dr, rows, K, dw, db, dg, dbe, row0)
        assert np.array_equal(got[row0:row0 + rows], part), (row0, float(np.abs(got[row0:row0 + rows] - part).max()))
    rows = np.array([0, 85 * 256 - 1, 85 * 256, M - 1])       # either side of the first boundary, against the fp64 LayerNorm (bound of test_gemm_routes_gpu.py)
    v = a[rows].astype(np.float64) @ w.astype(np.float64).T + bias + r[rows]
    mu = v.mean(1, keepdims=True)
    ref = (v - mu) / np.sqrt(((v - mu) ** 2).mean(1, keepdims=True) + 1e-12) * gamma + beta
    assert np.abs(got[rows] - ref).max() / np.abs(ref).max() < 3e-5


SKIP = 4


def _ln_ex(l, dx, dg, db, M, dres, resid_rows, dri, m_live, flags, row0=0):
    out = torch.full((M, 768), 7.0, device="cuda", dtype=torch.float32)
    rc = l.mms_dbg_layernorm_ex(dx.data_ptr() + row0 * 768 * 4, dg.data_ptr(), db.data_ptr(), M, None if dres is None else dres.data_ptr(), resid_rows,
                                None if dri is None else dri.data_ptr() + row0 * 4, m_live, flags, out.data_ptr(), None, None)
    assert rc == 0, l.mms_global_error()
    return out.cpu().numpy()


def test_layernorm_fallback_on_its_bounded_grid_writes_the_same_rows_and_nothing_when_skipped():
    """The launches that carry the skip word (the fall-back queued behind every LayerNorm-fused GEMM) run on a bounded grid, 8 workgroups per CU with
    every wavefront striding over rows, once one wavefront per row would need more workgroups than that (more than 8 192 rows on 256 CUs).  Not skipped,
    they must write what the one-wavefront-per-row launch writes: mms_dbg_layernorm never carries the word, and the same hook on row ranges of 4 096 rows
    stays under the bound.  Skipped, they write nothing."""
    l = lib.load()
    M, R = 50000 + 3, 4099
    x = weights.normal("tb/lnk/x", (M, 768), 3, 2.0, 0.5)
    g = weights.normal("tb/lnk/g", (768,), 3, 0.1, 1.0)
    b = weights.normal("tb/lnk/b", (768,), 3, 0.1)
    resid = weights.normal("tb/lnk/r", (R, 768), 3, 1.5)
    r_index = np.random.default_rng(5).integers(0, R, M).astype(np.int32)
    dx, dg, db, dres, dri = _dev(x), _dev(g), _dev(b), _dev(resid), _dev(r_index)
    # no residual: against the launch without the skip word
    ref = torch.empty((M, 768), device="cuda", dtype=torch.float32)
    assert l.mms_dbg_layernorm(dx.data_ptr(), dg.data_ptr(), db.data_ptr(), M, ref.data_ptr(), None) == 0, l.mms_global_error()
    got = _ln_ex(l, dx, dg, db, M, None, 0, None, -1, 0)
    assert np.array_equal(got, ref.cpu().numpy())
    # gathered residual, device-side row count, both directions: against launches small enough for one wavefront per row
    live = M - 1234
    for m_live in (-1, live):
        lim = M if m_live < 0 else live
        got = _ln_ex(l, dx, dg, db, M, dres, R, dri, m_live, 0)
        for row0 in range(0, lim, 4096):
            rows = min(4096, lim - row0)
            part = _ln_ex(l, dx, dg, db, rows, dres, R, dri, -1, 0, row0)
            assert np.array_equal(got[row0:row0 + rows], part), (m_live, row0)
        assert np.all(got[lim:] == 0.0)
        assert np.array_equal(_ln_ex(l, dx, dg, db, M, dres, R, dri, m_live, 1), got)      # reversed walk: the same rows
    x64 = x[:64].astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    fp64 = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-12) * g + b
    assert np.abs(ref[:64].cpu().numpy() - fp64).max() < 5e-5      # test_row_kernels_gpu.py's bound
    skipped = _ln_ex(l, dx, dg, db, M, dres, R, dri, -1, SKIP)
    assert np.all(skipped == 0.0)
