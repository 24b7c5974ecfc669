"""Submission ranking (uniqueness filter + top-5) on the device against the host form, same arrays, same box.
usage (GPU box): python tools/rank_bench.py [rows, comma list] [--one ROWS]
Per size (default 28000,120000,240000,1000000; 30 candidates per query, product ids from rows / 2 values, distinct within a query, fp32 scores):
  device time of mms_rank_submission (hipEvent, mean of 20 after 3 warm-ups), wall time of ensemble.submission_rows_device including its one
  read-back (best of 5), wall time of ensemble.submission_rows (best of 3).  The rows of the two forms are compared before anything is timed.
--one ROWS: a single untimed-by-this-script device call on ROWS rows after one warm-up (the process to put under rocprofv3 --kernel-trace --stats).
The host form is single-threaded numpy; the first output line states how many CPUs the process may use."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble as E  # noqa: E402
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib  # noqa: E402

K = 30
DEV = torch.device("cuda", 0)


def table(n, seed=1):
    rng = np.random.default_rng(seed)
    nq, pool = n // K, n // 2
    q = np.repeat(np.arange(nq, dtype=np.int64) + 1, K)
    # K distinct ids per query: a random start plus strictly increasing offsets whose sum stays below the pool size
    p = (rng.integers(0, pool, (nq, 1)) + np.cumsum(rng.integers(1, pool // K + 1, (nq, K)), 1)) % pool
    s = rng.random(nq * K, dtype=np.float32)
    return q, p.reshape(-1).astype(np.int64), s


def device_ms(dq, dp, ds, reps=20, warm=3):
    l = lib.load()
    n = ds.shape[0]
    wsb = l.mms_rank_workspace_bytes(n)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    oq, op, oc = torch.empty((n,), dtype=torch.int64, device=DEV), torch.empty((n, 5), dtype=torch.int64, device=DEV), torch.empty((n,), dtype=torch.int32, device=DEV)
    st = torch.empty((4,), dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    call = lambda: l.mms_rank_submission(dq.data_ptr(), dp.data_ptr(), ds.data_ptr(), None, n, E.GAP, E.TIE, ws.data_ptr(), wsb, n, oq.data_ptr(), op.data_ptr(),
                                         oc.data_ptr(), st.data_ptr(), stream)
    for _ in range(warm):
        assert call() == 0
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); assert call() == 0; e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.mean(ms)), float(np.min(ms)), wsb, st.cpu().tolist()


def main():
    if "--one" in sys.argv:
        n = int(sys.argv[sys.argv.index("--one") + 1])
        q, p, s = table(n)
        dq, dp, ds = (torch.from_numpy(x).to(DEV) for x in (q, p, s))
        for _ in range(2):
            st = E.rank_device(dq, dp, ds)[3]
            torch.cuda.synchronize()
        print("one call, %d rows: status %s" % (n, st.cpu().tolist()))
        return
    sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [28000, 120000, 240000, 1000000]
    print("%s, torch %s, %d CPUs visible to this process (of %d)" % (torch.cuda.get_device_name(0), torch.__version__, len(os.sched_getaffinity(0)), os.cpu_count()))
    print("rows      queries  out rows  device ms (mean of 20 / min)  workspace MB  submission_rows_device ms (best of 5, with read-back)  submission_rows ms (host, best of 3)  host / device")
    for n in sizes:
        q, p, s = table(n)
        n = len(q)
        dq, dp, ds = (torch.from_numpy(x).to(DEV) for x in (q, p, s))
        info = {}
        got = E.submission_rows_device(dq, dp, ds, info=info)
        t_host = []
        for _ in range(3):
            t0 = time.perf_counter(); want = E.submission_rows(q, p, s); t_host.append(time.perf_counter() - t0)
        assert info == {"path": "device", "flags": 0} and list(got) == list(want) and got == want, info
        mean_ms, min_ms, wsb, st = device_ms(dq, dp, ds)
        t_dev = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); E.submission_rows_device(dq, dp, ds); t_dev.append(time.perf_counter() - t0)
        print("%-9d %-8d %-9d %8.3f / %-8.3f            %-13.1f %-55.2f %-37.1f %.1fx"
              % (n, st[3], st[0], mean_ms, min_ms, wsb / 1e6, min(t_dev) * 1e3, min(t_host) * 1e3, min(t_host) / min(t_dev)), flush=True)


if __name__ == "__main__":
    main()
