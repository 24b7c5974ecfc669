"""GPU suite: the frame of the mms_dbg_* hooks (csrc/test_hooks.hip) -- a refused call leaves the caller's output alone and the hook usable, and mms_dbg_gemm,
mms_dbg_gemm_ex and mms_dbg_gemm_rows are ONE path: the dense call and the identity spec give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib, weights

pytestmark = pytest.mark.gpu

SENT = 7.0


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def test_gemm_ln_refuses_fp8_without_a_trace_and_then_runs():
    M, K = 64, 128
    l = lib.load()
    a = weights.normal("hf/ln/a", (M, K), 1)
    w = weights.round_to_bf16(weights.normal("hf/ln/w", (768, K), 1, 1.0 / np.sqrt(K)))
    bias = weights.normal("hf/ln/b", (768,), 1, 0.1)
    r = weights.normal("hf/ln/r", (M, 768), 1) + 0.3
    gamma = weights.normal("hf/ln/g", (768,), 1, 0.1, 1.0)
    beta = weights.normal("hf/ln/be", (768,), 1, 0.1)
    da, dw, db, dr, dg, dbe = _dev(a), _dev(w), _dev(bias), _dev(r), _dev(gamma), _dev(beta)
    out = torch.full((M, 768), SENT, device="cuda", dtype=torch.float32)

    def call(flags):
        rc = l.mms_dbg_gemm_ln(da.data_ptr(), M, K, dw.data_ptr(), db.data_ptr(), dr.data_ptr(), dg.data_ptr(), dbe.data_ptr(), flags, out.data_ptr(), None, None)
        torch.cuda.synchronize()
        return rc

    assert call(1) == 1 and b"two-pass" in l.mms_global_error(), l.mms_global_error()
    assert bool((out == SENT).all()), "a refused call wrote to the caller's output"
    assert call(0) == 0, l.mms_global_error()
    v = a.astype(np.float64) @ w.astype(np.float64).T + bias + r
    mu = v.mean(1, keepdims=True)
    ref = (v - mu) / np.sqrt(((v - mu) ** 2).mean(1, keepdims=True) + 1e-12) * gamma + beta
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max()
    print("gemm_ln after a refusal: max deviation %.2e (bound 3e-5)" % err)
    assert err < 3e-5, err      # the bound of test_gemm_routes_gpu.py::test_gemm_with_fused_layernorm_epilogue


def test_gemm_bench_refuses_a_mode_and_then_runs():
    l = lib.load()
    ms = C.c_float(0)
    assert l.mms_dbg_gemm_bench(256, 256, 128, 2, 0, 0, 1, 52, 2, C.byref(ms)) == 1      # 52: the mx8 engine takes no residual
    assert b"mx8 engine needs" in l.mms_global_error(), l.mms_global_error()
    assert l.mms_dbg_gemm_bench(256, 256, 128, 2, 0, 0, 0, lib.ENGINES["ENG_AUTO"], 2, C.byref(ms)) == 0, l.mms_global_error()
    assert ms.value > 0


@pytest.mark.parametrize("out_kind", [0, 1, 2], ids=["fp32", "planes", "head-major"])
def test_the_three_two_pass_gemm_hooks_are_one_path(out_kind):
    """M = 130: one full 128-row tile and a ragged one; N = 128, K = 64, bias, no residual, two passes on ENG_TILE_128.  mms_dbg_gemm has no head-major form."""
    M, N, K, engine = 130, 128, 64, lib.ENGINES["ENG_TILE_128"]
    l = lib.load()
    a = weights.normal("hf/g/a", (M, K), 1)
    w = weights.round_to_bf16(weights.normal("hf/g/w", (N, K), 1, 1.0 / np.sqrt(K)))
    bias = weights.normal("hf/g/b", (N,), 1, 0.1)
    da, dw, db = _dev(a), _dev(w), _dev(bias)
    outs = {}

    def out(name):
        outs[name] = torch.zeros(M * N, device="cuda", dtype=torch.float32)
        return outs[name].data_ptr()

    if out_kind != 2:
        assert l.mms_dbg_gemm(da.data_ptr(), M, K, K, dw.data_ptr(), N, db.data_ptr(), None, 0, 2, out_kind, engine, out("gemm"), None) == 0, l.mms_global_error()
    assert l.mms_dbg_gemm_ex(da.data_ptr(), M, K, dw.data_ptr(), N, db.data_ptr(), 0, out_kind, engine, -1, 0, out("ex"), None) == 0, l.mms_global_error()
    s = lib.RowsSpec()
    s.M, s.N, s.K, s.nsplit, s.engine, s.act, s.reverse, s.m_live = M, N, K, 2, engine, 0, 0, -1
    s.a_rows, s.lda, s.out_kind, s.ldo, s.c_rows = M, K, out_kind, N, M
    s.hm_rows, s.hm_col0, s.hm_blocks = M, 0, 2
    assert l.mms_dbg_gemm_rows(C.byref(s), da.data_ptr(), None, dw.data_ptr(), db.data_ptr(), None, None, out("rows"), None) == 0, l.mms_global_error()
    torch.cuda.synchronize()
    bits = {k: v.cpu().numpy().view(np.uint32) for k, v in outs.items()}
    for name in bits:
        assert np.array_equal(bits[name], bits["rows"]), (name, int((bits[name] != bits["rows"]).sum()))
    # ... and it is the product: fp64 reference, the two-pass bound of test_gemm_addressing_gpu.py (planes round the result to hi + lo bf16: 2^-17)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias
    got = outs["rows"].cpu().numpy().astype(np.float64)
    got = got.reshape(2, M, 64).transpose(1, 0, 2).reshape(M, N) if out_kind == 2 else got.reshape(M, N)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("out_kind %d: max deviation %.2e (bound 3e-5)" % (out_kind, err))
    assert err < 3e-5, err
