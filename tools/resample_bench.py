"""Timing of the resampled joint fit (mms_joint_sweep_codes + mms_resample_select, csrc/resample.hip) beside the per-replicate loop it replaces.
usage (GPU box): python tools/resample_bench.py                 (both grids: 35 x 52 and 1 771 x 102; 20, 200 and 1 000 replicates)
  The valid-like table of tools/joint_sweep_bench.py: 14 720 rows, 491 key queries of 30 rows, 4 members, k = 5.  hipEvent times, median of 20 after 3
  warm-ups, device-resident inputs, a prebuilt AnswerKey; one box, one run.  Per pair of grids:
    (i)    ndcg.joint_codes_device (mms_joint_sweep_codes) against ndcg.joint_sweep_device (mms_joint_sweep), values only: what writing the codes costs
    (ii)   ndcg.resample_select_device (mms_resample_select) with one probe on 20 replicates (5-fold x 4), 200 and 1 000 (bootstrap), and its cost per
           (replicate, item, key query)
    (b)    what the library offered before, on the 20 k-fold replicates: per replicate an AnswerKey of the training key queries, mms_joint_sweep on it,
           a read-back of the values, the arg-max on the host, and a second mms_joint_sweep of the winner alone on the held-out key queries (cheaper
           than a second full sweep); wall time, median of 3 runs.  A bootstrap replicate repeats key queries, which a key cannot: the 200 and 1 000
           replicate figures of (b) are 20-replicate time x R / 20, EXTRAPOLATED.
  The winners and held-out values of (b) are compared with (ii)'s (its per-fold value sums the histogram in bin order, (ii) the key queries in key
  order: the two can differ in the last bit, so the agreement is reported, not asserted)."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tools"))
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import ensemble, ndcg  # noqa: E402

DEV = torch.device("cuda", 0)
K = 5


def table(nq, per, n, seed):
    rng = np.random.default_rng(seed)
    q = np.repeat(np.arange(nq, dtype=np.int64) + 7, per)[:n]
    pool = 1000000 + np.arange(max(n // 5, 2 * per), dtype=np.int64)
    p = np.concatenate([rng.choice(pool, per, replace=False) for _ in range(nq)])[:n]          # no repeated (query, product) pair
    mem = rng.random((4, n), dtype=np.float32)
    key = {int(7 + i): rng.choice(p[i * per:min((i + 1) * per, n)], 5, replace=False).tolist() for i in range(nq) if i * per < n}
    return q, p, mem, key


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
    return float(np.median(ms)), min(ms), max(ms), out


def loop_b(dq, dp, dmem, dw, df, weights, filters, key, count_fit):
    """per replicate: training sub-key, full sweep, read-back, host arg-max, a sweep of the winner alone on the held-out sub-key"""
    names = list(key)
    G = len(filters)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    winners, held = [], []
    for row in count_fit:
        fit_key = ndcg.AnswerKey({names[i]: key[names[i]] for i in np.flatnonzero(row)}, DEV)
        values = ndcg.joint_sweep_device(dq, dp, dmem, dw, df, fit_key, K, allow_missing=True)[0].cpu().numpy()      # the synchronising read
        best = int(np.argmax(values))
        eval_key = ndcg.AnswerKey({names[i]: key[names[i]] for i in np.flatnonzero(row == 0)}, DEV)
        v = ndcg.joint_sweep_device(dq, dp, dmem, dw[best // G:best // G + 1], df[best % G:best % G + 1], eval_key, K, allow_missing=True)[0]
        winners.append(best)
        held.append(float(v.cpu().numpy()[0, 0]))
    return time.perf_counter() - t0, np.array(winners), np.array(held)


q, p, mem, key = table(491, 30, 14720, 1)
ak = ndcg.AnswerKey(key, DEV)
Qa = len(key)
dq, dp, dmem = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (q, p, mem))
print("valid-like table: %d rows, %d key queries, %d members, k = %d; hipEvent, median of 20 after 3 warm-ups" % (len(q), Qa, len(mem), K), flush=True)
SCHEMES = [("5-fold x 4", ensemble.kfold_counts(Qa, 5, 4, 0)), ("bootstrap", ensemble.bootstrap_counts(Qa, 200, 0)), ("bootstrap", ensemble.bootstrap_counts(Qa, 1000, 0))]
for wsteps, fsteps in ((4, 50), (20, 100)):
    weights, filters = ensemble.weight_grid(4, wsteps), ensemble.filter_grid(fsteps)
    W, G = len(weights), len(filters)
    dw, df = torch.from_numpy(weights).to(DEV), torch.from_numpy(filters).to(DEV)
    ms_plain, lo_p, hi_p, (values_p, _, _) = timed(lambda: ndcg.joint_sweep_device(dq, dp, dmem, dw, df, ak, K))
    ms_codes, lo_c, hi_c, (values, _, status, codes) = timed(lambda: ndcg.joint_codes_device(dq, dp, dmem, dw, df, ak, K))
    assert status.tolist()[2] == 0 and values.cpu().numpy().tobytes() == values_p.cpu().numpy().tobytes()
    whole = int(np.argmax(values.cpu().numpy()))
    print("W x G = %5d x %3d = %6d items, code matrix %.1f MB: (i) mms_joint_sweep %.3f ms (min %.3f, max %.3f), mms_joint_sweep_codes %.3f ms (min %.3f, max %.3f): "
          "the codes cost %.3f ms = %.1f %%" % (W, G, W * G, codes.numel() / 1e6, ms_plain, lo_p, hi_p, ms_codes, lo_c, hi_c, ms_codes - ms_plain,
                                                100 * (ms_codes - ms_plain) / ms_plain), flush=True)
    ms_20 = None
    for name, (cf, ce) in SCHEMES:
        reps = len(cf)
        dcf, dce = torch.from_numpy(cf).to(DEV), torch.from_numpy(ce).to(DEV)
        probe = torch.tensor([whole], dtype=torch.int64, device=DEV)
        ms, lo, hi, out = timed(lambda: ndcg.resample_select_device(codes, W, dcf, dce, K, probe))
        best, fv, ev = (t.cpu().numpy() for t in out[:3])
        assert out[5].tolist()[2] == 0
        triples = reps * W * G * Qa
        print("    (ii) mms_resample_select, %4d replicates (%s): %.3f ms (min %.3f, max %.3f) = %.2f ps per (replicate, item, key query), %.1f G multiply-adds/s; "
              "held-out %.4f, optimism %.4f, agreement %.2f" % (reps, name, ms, lo, hi, 1e9 * ms / triples, triples / ms / 1e6, float(np.nanmean(ev)),
                                                                float(np.nanmean(fv - ev)), float(np.mean(best == whole))), flush=True)
        if reps == 20:
            ms_20, best_20, ev_20 = ms, best, ev
            loop_b(dq, dp, dmem, dw, df, weights, filters, key, cf[:1])      # warm-up
            runs = [loop_b(dq, dp, dmem, dw, df, weights, filters, key, cf) for _ in range(3)]
            t_b = float(np.median([r[0] for r in runs]))
            same_w, same_v = int((runs[0][1] == best_20).sum()), int((runs[0][2] == ev_20).sum())
            print("    (b) per replicate: sub-key, mms_joint_sweep, read-back, host arg-max, the winner's sweep on the held-out sub-key: %.1f ms for 20 replicates "
                  "(wall, median of 3; %.2f ms per replicate); (i) + (ii) = %.3f ms: x%.1f faster; %d / 20 winners and %d / 20 held-out values identical to (ii)'s"
                  % (1e3 * t_b, 1e3 * t_b / 20, ms_codes + ms_20, 1e3 * t_b / (ms_codes + ms_20), same_w, same_v), flush=True)
            assert ms_codes + ms_20 < 1e3 * t_b, "the resampled fit must beat the per-replicate loop at 20 replicates"
        else:
            print("    (b) EXTRAPOLATED to %d replicates (20-replicate time x %d / 20; not measured): %.0f ms; (i) + (ii) = %.3f ms: x%.0f"
                  % (reps, reps, 1e3 * t_b * reps / 20, ms_codes + ms, 1e3 * t_b * reps / 20 / (ms_codes + ms)), flush=True)
