"""Timing of the weight sweep (mms_ndcg_weight_sweep, csrc/ndcg_sweep.hip) beside the two ways to search the weights without it.
usage (GPU box): python tools/weight_sweep_bench.py [k [grid steps ...]]      (default: 5 4 20 100)
  A valid-like table (14 720 rows, 491 key queries, 4 members = a random score plus noise, fp32) and the simplex grids of 35 / 1 771 / 176 851
  weight vectors (ensemble.weight_grid(4, 4 / 20 / 100)).  Per grid:
    device   hipEvent time of ONE ndcg.ndcg_sweep_device call (median of 20 after 3 warm-ups; device-resident inputs, prebuilt AnswerKey)
    (a)      ndcg.ndcg_sweep_host: wall time, measured on the whole grid of 35 and on 50 vectors of the larger grids (extrapolated per vector)
    (b)      what the library offered before: per vector a torch double merge of the members and one ndcg.ndcg_codes_device call, enqueued back
             to back, one synchronisation at the end (wall time; measured on the grids of 35 and 1 771, extrapolated per vector for 176 851)
  The device values of the vectors that (a) ran are checked bit for bit against it."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg  # noqa: E402

DEV = torch.device("cuda", 0)
K = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = [int(x) for x in sys.argv[2:]] or [4, 20, 100]


def table(nq, per, seed):
    rng = np.random.default_rng(seed)
    q = np.repeat(np.arange(nq, dtype=np.int64) + 7, per)
    p = (1000000 + rng.integers(0, 40 * per, nq * per)).astype(np.int64)
    s = rng.random(nq * per)
    key = {int(7 + i): p[i * per + rng.choice(per, 5, replace=False)].tolist() for i in range(nq)}
    return q, p, s, key, rng


q, p, s, key, rng = table(496, 30, 1)
q, p, s = q[:14720], p[:14720], s[:14720]                 # the valid set's size; the key keeps the queries that still have rows
key = {kq: t for kq, t in key.items() if kq <= int(q[-1])}
mem = np.stack([(s + f * s.std() * rng.standard_normal(len(s))).astype(np.float32) for f in (0.8, 0.8, 1.0, 1.2)])
ak = ndcg.AnswerKey(key, DEV)
dq, dp, dmem = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (q, p, mem))
print("valid-like table: %d rows, %d key queries, %d members, k = %d" % (len(q), len(key), len(mem), K), flush=True)


def merge(w):
    acc = dmem[0].double() * float(w[0])
    for m in range(1, 4):
        acc = acc + dmem[m].double() * float(w[m])
    return acc


def loop_b(grid):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    hists = [ndcg.ndcg_codes_device(dq, dp, merge(w), ak, K)[2] for w in grid]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, hists


loop_b(ensemble.weight_grid(4, 4))                         # warm-up: allocator, kernels
per_b = loop_b(ensemble.weight_grid(4, 20))[0] / 1771
for steps in STEPS:
    grid = ensemble.weight_grid(4, steps)
    W = len(grid)
    dgrid = torch.from_numpy(grid).to(DEV)
    ms = []
    for i in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        values, hist, status = ndcg.ndcg_sweep_device(dq, dp, dmem, dgrid, ak, K)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    assert status.tolist()[2] == 0
    sample = np.arange(W) if W <= 50 else np.sort(np.random.default_rng(steps).choice(W, 50, replace=False))
    t0 = time.perf_counter(); hv, hh = ndcg.ndcg_sweep_host(q, p, mem, grid[sample], key, K); t_a = (time.perf_counter() - t0) / len(sample)
    assert values.cpu().numpy()[sample].tobytes() == hv.tobytes() and np.array_equal(hist.cpu().numpy()[sample], hh)
    if W <= 2000:
        t_b, hists = loop_b(grid)
        assert all(torch.equal(h, hist[v]) for v, h in enumerate(hists))
        per_b, how_b = t_b / W, "measured"
    else:
        how_b = "extrapolated from 1771"
    best = int(np.argmax(values.cpu().numpy()))
    med = float(np.median(ms))
    print("W = %6d: mms_ndcg_weight_sweep %.3f ms (median of 20, min %.3f, max %.3f) = %.3f us per vector; (a) ndcg_sweep_host %.2f s (%.2f ms per vector, %s); "
          "(b) torch merge + mms_ndcg_at_k per vector %.4f s (%.3f ms per vector, %s); device vs (a) x%.0f, vs (b) x%.1f; best %s -> %.6f (bit-equal to (a) on %d vectors)"
          % (W, med, min(ms), max(ms), 1e3 * med / W, t_a * W, t_a * 1e3, "measured" if W <= 50 else "extrapolated from 50", per_b * W, per_b * 1e3, how_b,
             t_a * W * 1e3 / med, per_b * W * 1e3 / med, tuple(grid[best].tolist()), float(values[best]), len(sample)), flush=True)
