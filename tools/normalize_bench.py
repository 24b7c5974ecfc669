"""The per-query normalisation against what it precedes, one process, one run (profiles/rd20_normalize.txt):
  (a) mms_normalize_members per mode, hipEvent time of the enqueued call (workspace and output allocated once), median of 20, on a valid-like table
      (491 queries, 14 720 rows, 4 members) and on a 240 000-row table (8 000 queries of 30 rows);
  (b) ensemble.fit_joint at 1 771 x 102 grid points on the valid-like table with and without normalize="zscore": hipEvent time around the whole
      call (the sweep, the pre-pass, the one synchronising read), median / min / max of 20;
  (c) ensemble.normalize_members, the host form, on the same tables (perf_counter, median of 5).
  python tools/normalize_bench.py
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table(rows_per_query, seed):
    """-> (query_id, product_id, members fp32 [4, n], answer key): rows interleaved at random, products from a pool of n / 3 (no pair twice), three
    relevant products per query; member scales as unrelated as the ensemble's (a cosine with margin, a probability, a probability, a logit)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = int(sum(rows_per_query))
    pool = np.arange(max(n // 3, max(rows_per_query) + 8), dtype=np.int64) + 100000
    q = np.repeat(np.arange(len(rows_per_query), dtype=np.int64) * 7 + 1000, rows_per_query)
    start = np.cumsum(np.r_[0, rows_per_query[:-1]])
    j = np.arange(n) - np.repeat(start, rows_per_query)                       # place inside the query
    p = pool[(np.repeat(rng.integers(0, len(pool), len(start)), rows_per_query) + j * 7919) % len(pool)]      # distinct inside a query
    key = {int(q[s]): [int(x) for x in p[s:s + min(3, r)]] for s, r in zip(start.tolist(), rows_per_query)}
    z = rng.standard_normal((4, n))
    mem = np.stack([30.0 * np.tanh(z[0]), 1 / (1 + np.exp(-z[1])), 1 / (1 + np.exp(-3 * z[2])), 4.0 * z[3]]).astype(np.float32)
    perm = rng.permutation(n)
    return q[perm], p[perm], np.ascontiguousarray(mem[:, perm]), key


def main():
    import torch

    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, lib, ndcg
    dev = torch.device("cuda", 0)
    l = lib.load()

    def timed(call, n=20, warm=3):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    tables = {"valid-like": table([30] * 481 + [29] * 10, 1), "240k": table([30] * 8000, 2)}
    print("(a) mms_normalize_members, 4 members, hipEvent time of the enqueued call: median (min .. max) of 20   |   (c) the host form, median of 5")
    for name, (q, p, mem, key) in tables.items():
        n = len(q)
        dq, dmem = torch.from_numpy(q).to(dev), torch.from_numpy(mem).to(dev)
        out, status = torch.empty_like(dmem), torch.zeros(4, dtype=torch.int32, device=dev)
        ws_bytes = l.mms_normalize_workspace_bytes(n, 4)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for mode in ensemble.NORMALIZE[1:]:
            def call():
                rc = l.mms_normalize_members(dq.data_ptr(), dmem.data_ptr(), 4, n, ensemble.NORMALIZE.index(mode), out.data_ptr(), status.data_ptr(),
                                             ws.data_ptr(), ws_bytes, stream)
                assert rc == 0
            med, lo, hi = timed(call)
            host = []
            for _ in range(5):
                t = time.perf_counter()
                want = ensemble.normalize_members(q, mem, mode)
                host.append((time.perf_counter() - t) * 1e3)
            same = out.cpu().numpy().tobytes() == want.tobytes()
            print("  %-10s %7d rows  %-7s %8.3f ms (%.3f .. %.3f)  status %s  |  host %8.2f ms  bit-equal %s"
                  % (name, n, mode, med, lo, hi, status.cpu().tolist(), statistics.median(host), same))
    q, p, mem, key = tables["valid-like"]
    dq, dp, dmem = torch.from_numpy(q).to(dev), torch.from_numpy(p).to(dev), torch.from_numpy(mem).to(dev)
    akey = ndcg.AnswerKey(key, dev)
    grid, filters = ensemble.weight_grid(4, 20), ensemble.filter_grid()
    print("(b) ensemble.fit_joint at %d x %d on the valid-like table, hipEvent time around the call: median (min .. max) of 20" % (len(grid), len(filters)))
    res = {}
    for mode in ("none", "zscore", "none", "zscore"):                         # twice each, interleaved: the second pair shows the drift
        med, lo, hi = timed(lambda: res.__setitem__(mode, ensemble.fit_joint(dq, dp, dmem, akey, grid, filters, normalize=mode)))
        print("  normalize=%-7s %9.3f ms (%.3f .. %.3f)   winner %s %s value %.6f" % (mode, med, lo, hi, res[mode][0], res[mode][1], res[mode][2]))
    med, lo, hi = timed(lambda: ensemble.normalize_members_device(dq, dmem, "zscore"))
    print("  normalize_members_device(zscore) alone, with its allocations and its status read: %.3f ms (%.3f .. %.3f)" % (med, lo, hi))


if __name__ == "__main__":
    main()
