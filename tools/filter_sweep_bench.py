"""Timing of the filter sweep (mms_filter_sweep, csrc/filter_sweep.hip) beside the two ways to search (gap, tie) without it.
usage (GPU box): python tools/filter_sweep_bench.py [k [grid steps ...]]      (default: 5 0 100 10000 -> G = 1, 102, 10 002; steps 0 = the "no filter" row alone)
                 python tools/filter_sweep_bench.py --one TABLE STEPS          (TABLE: valid-like | testB-sized; one warm-up and five calls of the k = 5 sweep
                                                                                on that table and grid, nothing else: the process to put under rocprofv3 --kernel-trace --stats)
  Two tables of fp64 merged scores -- valid-like: 14 720 rows, 491 key queries; testB-sized: 240 000 rows, 8 000 queries, all of them in the key --
  whose products come from a pool of a fifth of the rows (most products occur under several queries, as the filter needs).  Per table and grid:
    device   hipEvent time of ONE ndcg.filter_sweep_device call (median of 20 after 3 warm-ups; device-resident inputs, prebuilt AnswerKey), as
             ensemble.fit_filter issues it (values and histograms) and, in a second series, with the [G, key queries] code matrix written as well
    (a)      ndcg.filter_sweep_host: wall time, measured on at most 4 filters of the grid (extrapolated per filter)
    (b)      what the library offered before: per filter one ensemble.rank_device call (mms_rank_submission), enqueued back to back, ONE read-back of
             all the output rows at the end, then the host grading of every filter's rows against the key (ndcg.codes_of_rows) -- wall time, measured
             on at most 102 filters (extrapolated per filter)
  The device codes of the filters that (a) and (b) ran are checked entry for entry against them."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg  # noqa: E402

DEV = torch.device("cuda", 0)
ONE = sys.argv[2:4] if sys.argv[1:2] == ["--one"] else None
K = int(sys.argv[1]) if len(sys.argv) > 1 and not ONE else 5
STEPS = [int(ONE[1])] if ONE else [int(x) for x in sys.argv[2:]] or [0, 100, 10000]


def table(nq, per, n, seed):
    rng = np.random.default_rng(seed)
    q = np.repeat(np.arange(nq, dtype=np.int64) + 7, per)[:n]
    pool = 1000000 + np.arange(max(n // 5, 2 * per), dtype=np.int64)
    p = np.concatenate([rng.choice(pool, per, replace=False) for _ in range(nq)])[:n]          # no repeated (query, product) pair
    s = rng.random(n)
    key = {int(7 + i): rng.choice(p[i * per:min((i + 1) * per, n)], 5, replace=False).tolist() for i in range(nq) if i * per < n}
    return q, p, s, key


def rows_of(host, g, n_out):
    qs = host[4:4 + n_out].tolist()
    cnt = host[4 + g:4 + g + n_out].tolist()
    prods = host[4 + 2 * g:4 + 2 * g + 5 * n_out].tolist()
    return {str(qq): [str(x) for x in prods[5 * i:5 * i + cnt[i]]] for i, qq in enumerate(qs)}


def loop_b(dq, dp, ds, filters, key, present, room):
    """one mms_rank_submission per filter back to back, one read-back, the host grading"""
    torch.cuda.synchronize(); t0 = time.perf_counter()
    packs = []
    for gap, tie in filters:
        out_query, out_products, out_count, status = ensemble.rank_device(dq, dp, ds, gap, tie)
        packs.append(torch.cat([status.to(torch.int64), out_query[:room], out_count[:room].to(torch.int64), out_products[:room].reshape(-1)]))
    host = torch.stack(packs).cpu().numpy()                                  # the one synchronising read
    t1 = time.perf_counter()
    codes = np.stack([ndcg.codes_of_rows(rows_of(h, room, int(h[0])), present, key, K, False) for h in host])
    return t1 - t0, time.perf_counter() - t1, codes


def timed(call):
    ms = []
    for i in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return ms, out


for name, (nq, per, n) in (("valid-like", (491, 30, 14720)), ("testB-sized", (8000, 30, 240000))):
    if ONE and name != ONE[0]:
        continue
    q, p, s, key = table(nq, per, n, 1)
    ak = ndcg.AnswerKey(key, DEV)
    present = set(np.unique(q).tolist())
    dq, dp, ds = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (q, p, s))
    print("%s table: %d rows, %d key queries, k = %d" % (name, len(q), len(key), K), flush=True)
    if ONE:
        dgrid = torch.from_numpy(ensemble.filter_grid(STEPS[0]) if STEPS[0] else ensemble.filter_grid(1)[:1]).to(DEV)
        for i in range(6):
            ndcg.filter_sweep_device(dq, dp, ds, dgrid, ak, K)
        torch.cuda.synchronize()
        print("6 calls, G = %d" % len(dgrid), flush=True)
        continue
    loop_b(dq, dp, ds, ensemble.filter_grid(2), key, present, len(key))     # warm-up: allocator, kernels
    for steps in STEPS:
        grid = ensemble.filter_grid(steps) if steps else ensemble.filter_grid(1)[:1]
        G = len(grid)
        dgrid = torch.from_numpy(grid).to(DEV)
        ms, _ = timed(lambda: ndcg.filter_sweep_device(dq, dp, ds, dgrid, ak, K))
        ms_c, (values, hist, status, codes) = timed(lambda: ndcg.filter_sweep_device(dq, dp, ds, dgrid, ak, K, want_codes=True))
        assert status.tolist()[2] == 0
        codes, values = codes.cpu().numpy(), values.cpu().numpy()
        sa = np.unique(np.linspace(0, G - 1, min(G, 4)).astype(int))
        t0 = time.perf_counter(); hv, hh, hc = ndcg.filter_sweep_host(q, p, s, grid[sa], key, K); t_a = (time.perf_counter() - t0) / len(sa)
        assert values[sa].tobytes() == hv.tobytes() and np.array_equal(codes[sa], hc) and np.array_equal(hist.cpu().numpy()[sa], hh)
        sb = np.unique(np.linspace(0, G - 1, min(G, 102)).astype(int))
        t_dev, t_grade, bc = loop_b(dq, dp, ds, grid[sb], key, present, len(key))
        assert np.array_equal(codes[sb], bc)
        per_b = (t_dev + t_grade) / len(sb)
        med, best = float(np.median(ms)), int(np.argmax(values))
        print("G = %6d: mms_filter_sweep %.3f ms (median of 20, min %.3f, max %.3f) = %.3f us per filter, with the codes written %.3f ms; (a) filter_sweep_host %.2f s (%.1f ms per filter, "
              "measured on %d); (b) mms_rank_submission per filter + read-back + host grading %.3f s (%.3f ms per filter: %.3f enqueue and read, %.3f grading; "
              "measured on %d); device vs (a) x%.0f, vs (b) x%.0f; best %s -> %.6f"
              % (G, med, min(ms), max(ms), 1e3 * med / G, float(np.median(ms_c)), t_a * G, t_a * 1e3, len(sa), per_b * G, per_b * 1e3, 1e3 * t_dev / len(sb), 1e3 * t_grade / len(sb),
                 len(sb), t_a * G * 1e3 / med, per_b * G * 1e3 / med, tuple(grid[best].tolist()), float(values[best])), flush=True)
