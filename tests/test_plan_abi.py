"""CPU suite: the plan entry points of include/mmscore.h (mms_score_ensemble_plan / mms_cascade_safe_workspace_bytes / mms_cascade_select_safe) are
exported, the ABI revision is at least 16 and the header says so, mms_plan_stage has the C layout, the workspace is sized sanely, and the two
handle-free entry points refuse every bad argument with MMS_ERR_ARG and a message that names the function -- before anything is dereferenced or
launched, so dummy addresses do and no GPU is needed."""
import ctypes
import os
import shutil
import subprocess

import pytest

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, lib

MAX_ROWS = 1 << 22          # MMS_CASCADE_MAX_ROWS
HEADER = os.path.join(os.path.dirname(lib.LIB_PATH), "..", "..", "include", "mmscore.h")


def test_plan_symbols_are_exported_and_listed():
    so = ctypes.CDLL(lib.LIB_PATH)
    for n in ("mms_score_ensemble_plan", "mms_cascade_safe_workspace_bytes", "mms_cascade_select_safe"):
        assert hasattr(so, n) and n in lib.EXPORTS, n
    assert lib.ABI_VERSION >= 16 and lib.load().mms_version() == lib.ABI_VERSION


def test_header_names_revision_16_and_the_contract():
    text = open(HEADER, encoding="utf-8").read()
    assert "#define MMS_ABI_VERSION %d" % lib.ABI_VERSION in text and "r16: 16" in text
    for n in ("mms_score_ensemble_plan", "mms_cascade_safe_workspace_bytes", "mms_cascade_select_safe", "#define MMS_MEMBER_ZK 1", "#define MMS_MEMBER_LDS 2",
              "#define MMS_MEMBER_LX 4", "#define MMS_PLAN_MAX_STAGES 3", "BIT-EQUALITY RULE", "GUARANTEES"):
        assert n in text, n
    assert (lib.MEMBER_ZK, lib.MEMBER_LDS, lib.MEMBER_LX, lib.PLAN_MAX_STAGES) == (1, 2, 4, 3)
    assert ensemble.PLAN_MEMBERS == {"zk": lib.MEMBER_ZK, "lds": lib.MEMBER_LDS, "lxmert": lib.MEMBER_LX} and ensemble.PLAN_MAX_STAGES == lib.PLAN_MAX_STAGES


def test_plan_stage_matches_the_c_layout(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mmscore.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mms_plan_stage), '
                 'offsetof(mms_plan_stage, members), offsetof(mms_plan_stage, keep), offsetof(mms_plan_stage, safe_k), offsetof(mms_plan_stage, reserved)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    st = lib.PlanStage
    assert got == [ctypes.sizeof(st)] + [getattr(st, n).offset for n, _ in st._fields_] == [16, 0, 4, 8, 12]


def test_workspace_bytes():
    l = lib.load()
    prev = 0
    for n in (0, 1, 5, 511, 512, 513, 28000, 120000, 1000000, MAX_ROWS):
        b = l.mms_cascade_safe_workspace_bytes(n)
        assert b > 0 and b % 256 == 0 and b >= prev and b > l.mms_cascade_workspace_bytes(n), (n, b)      # one more image per row
        prev = b
    assert l.mms_cascade_safe_workspace_bytes(-1) == -1 and l.mms_cascade_safe_workspace_bytes(1 << 31) == -1
    assert l.mms_cascade_safe_workspace_bytes(MAX_ROWS + 1) == 256     # beyond the limit nothing is compared: every row is kept (flag)


def test_argument_errors_name_the_function_and_launch_nothing():
    l = lib.load()
    A = 0x10000                                     # a 256-byte aligned dummy address; never dereferenced
    n = 100
    ws = l.mms_cascade_safe_workspace_bytes(n)
    good = dict(g=A, lo=A, up=A, n=n, k=3, kept=A, lst=A, st=A, ws=A, wsb=ws, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return l.mms_cascade_select_safe(a["g"], a["lo"], a["up"], a["n"], a["k"], a["kept"], a["lst"], a["st"], a["ws"], a["wsb"], a["stream"])

    bad = [dict(n=-1), dict(n=1 << 31), dict(k=0), dict(k=-5), dict(g=None), dict(lo=None), dict(up=None), dict(kept=None), dict(lst=None), dict(st=None),
           dict(ws=None), dict(wsb=ws - 1), dict(wsb=l.mms_cascade_workspace_bytes(n)), dict(wsb=0), dict(ws=A + 128), dict(ws=A + 8), dict(n=0, st=None),
           dict(n=0, k=0)]
    for kw in bad:
        assert call(**kw) == 1, kw                  # MMS_ERR_ARG
        assert b"mms_cascade_select_safe" in l.mms_global_error(), kw


def test_plan_refuses_null_handles_before_reading_anything():
    l = lib.load()
    b = lib.EnsembleBatch()
    st = (lib.PlanStage * 1)(lib.PlanStage(7, 0, 0, 0))
    w = (ctypes.c_float * 4)(0.2, 0.2, 0.3, 0.3)
    assert l.mms_score_ensemble_plan(None, None, None, ctypes.byref(b), None, st, 1, w, None, None, None, None, None) == 1
