"""CPU suite: the weight-sweep entry points of include/mmscore.h (mms_ndcg_sweep_workspace_bytes / mms_ndcg_weight_sweep) are declared, exported, bound,
size their workspace sanely, and refuse every bad argument with MMS_ERR_ARG and a message that names the function -- before anything is dereferenced
or launched, so dummy addresses do and no GPU is needed."""
import ctypes
import os
import re

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib, ndcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mmscore.h")).read()
MAX_ROWS, MAX_KEYS, MAX_K = 1 << 22, 1 << 20, 8
MAX_MEMBERS, MAX_WEIGHTS = 8, 1 << 20


def test_header_declares_the_functions_and_the_caps():
    assert re.search(r"^int64_t\s+mms_ndcg_sweep_workspace_bytes\s*\(", HEADER, re.M)
    assert re.search(r"^int\s+mms_ndcg_weight_sweep\s*\(", HEADER, re.M)
    assert int(re.search(r"#define\s+MMS_SWEEP_MAX_MEMBERS\s+(\d+)", HEADER).group(1)) == MAX_MEMBERS == ndcg.MAX_MEMBERS
    assert re.search(r"#define\s+MMS_SWEEP_MAX_WEIGHTS\s+\(1 << 20\)", HEADER) and ndcg.MAX_WEIGHTS == MAX_WEIGHTS
    assert int(re.search(r"#define\s+MMS_ABI_VERSION\s+(\d+)", HEADER).group(1)) >= 10
    assert "r10: 10" in HEADER and "rounded on its own" in HEADER        # the history line and the arithmetic contract


def test_symbols_are_exported_listed_and_bound():
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in ("mms_ndcg_sweep_workspace_bytes", "mms_ndcg_weight_sweep"):
        assert hasattr(so, n) and n in lib.EXPORTS, n
    assert lib.ABI_VERSION >= 10
    l = lib.load()
    assert len(l.mms_ndcg_sweep_workspace_bytes.argtypes) == 4 and l.mms_ndcg_sweep_workspace_bytes.restype is ctypes.c_int64
    assert len(l.mms_ndcg_weight_sweep.argtypes) == 22


def test_workspace_bytes():
    l = lib.load()
    for n, qa, tk in ((0, 0, 0), (0, 1, 0), (1, 1, 1), (511, 20, 60), (14720, 496, 2500), (1000000, 50000, 250000), (MAX_ROWS, MAX_KEYS, MAX_ROWS)):
        base, prev = l.mms_ndcg_workspace_bytes(n, qa, tk), 0
        for m in range(1, MAX_MEMBERS + 1):
            b = l.mms_ndcg_sweep_workspace_bytes(n, qa, tk, m)
            assert b % 256 == 0 and b >= base + 4 * n * (m + 1) and b >= prev, (n, qa, tk, m, b)      # the packed records on top of the sibling's
            prev = b
    for bad in ((-1, 1, 1, 4), (1, -1, 1, 4), (1, 1, -1, 4), (MAX_ROWS + 1, 1, 1, 4), (1, MAX_KEYS + 1, 1, 4), (1, 1, MAX_ROWS + 1, 4),
                (100, 10, 30, 0), (100, 10, 30, -1), (100, 10, 30, MAX_MEMBERS + 1)):
        assert l.mms_ndcg_sweep_workspace_bytes(*bad) == -1, bad


A = 0x10000                                         # a 256-byte aligned dummy address; never dereferenced
N, QA, TK, M, W = 100, 10, 30, 4, 35


def test_weight_sweep_argument_errors_name_the_function_and_launch_nothing():
    l = lib.load()
    ws = l.mms_ndcg_sweep_workspace_bytes(N, QA, TK, M)
    good = dict(q=A, p=A, mem=A, m=M, n=N, kq=A, ko=A, kp=A, qa=QA, tk=TK, w=A, nw=W, k=5, am=0, bv=A, tot=QA, ws=A, wsb=ws, hist=A, val=A, st=A, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return l.mms_ndcg_weight_sweep(a["q"], a["p"], a["mem"], a["m"], a["n"], a["kq"], a["ko"], a["kp"], a["qa"], a["tk"], a["w"], a["nw"], a["k"], a["am"],
                                       a["bv"], a["tot"], a["ws"], a["wsb"], a["hist"], a["val"], a["st"], a["stream"])

    bad = [dict(m=0), dict(m=MAX_MEMBERS + 1), dict(m=-1), dict(nw=MAX_WEIGHTS + 1), dict(nw=-1), dict(val=A, bv=None), dict(wsb=ws - 1), dict(wsb=0),
           dict(wsb=l.mms_ndcg_workspace_bytes(N, QA, TK)),                                  # the sibling's size is too small
           dict(n=-1), dict(n=MAX_ROWS + 1), dict(qa=-1), dict(qa=MAX_KEYS + 1), dict(tk=-1), dict(tk=MAX_ROWS + 1), dict(k=0), dict(k=MAX_K + 1),
           dict(q=None), dict(p=None), dict(mem=None), dict(kq=None), dict(ko=None), dict(kp=None), dict(w=None), dict(hist=None), dict(ws=None), dict(st=None),
           dict(ws=A + 128), dict(ws=A + 8), dict(tot=0), dict(qa=0, tk=TK), dict(n=0, st=None), dict(n=0, nw=0, m=9)]
    for kw in bad:
        assert call(**kw) == 1, kw                  # MMS_ERR_ARG
        assert b"mms_ndcg_weight_sweep" in l.mms_global_error(), kw
