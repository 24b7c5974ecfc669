"""The cascade against its yardstick, mms_score_ensemble in the same process on the same batch: hipEvent time of the full fused call and of
mms_score_ensemble_cascade at keep in {5, 10, 15, 30} on the 1000 x 30 bench batch (full models, precision 2), median of 20 calls each.
  python tools/cascade_bench.py                  the table (profiles/rd16_cascade.txt)
  python tools/cascade_bench.py --trace KEEP     warm-up + 5 cascade calls at KEEP and nothing else: the workload of a kernel trace
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cas -- python tools/cascade_bench.py --trace 10
  python tools/cascade_bench.py --stats CSV      the share of that trace's kernel time spent in select + gather + merge
"""
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OVERHEAD = ("k_cas_", "k_cascade_", "k_gather_rows")      # (k_gather_rows also serves the second zk member's changed pairs: an upper bound)


def stats(path):
    total = over = 0.0
    rows = []
    for r in csv.DictReader(open(path)):
        ns = float(r["TotalDurationNs"])
        total += ns
        if any(t in r["Name"] for t in OVERHEAD):
            over += ns
            rows.append((ns, int(r["Calls"]), r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]))
    print("kernel trace of the cascade at the traced keep: %.1f ms of kernels, %.3f ms (%.2f %%) in select + gather + merge:" % (total / 1e6, over / 1e6, 100 * over / total))
    for ns, calls, name in sorted(rows, reverse=True):
        print("  %9.3f ms  %5d calls  %s" % (ns / 1e6, calls, name))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        return stats(sys.argv[2])
    import torch

    import bench
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import scorers, synth, weights
    dev = torch.device("cuda", 0)
    cfgs = {n: bench.CFGS[n]() for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), precision=2, device=0) for n, c in cfgs.items()}
    ens = scorers.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
    ps = synth.make_pairs(1000, 30, tag="/bench0", with_feats=False)
    feed = bench.device_feed("ensemble", cfgs, ps, bench.device_feats(ps, dev, 20200823), dev)
    gid = torch.as_tensor(ps.query_id, dtype=torch.int64).to(dev)
    B = ps.n
    prep = ens.prepare(feed)

    def timed(call, n):
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms)

    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        keep = int(sys.argv[2])
        for _ in range(2 + 5):
            ens.score_prepared(prep, True, cascade=(gid, keep))
        torch.cuda.synchronize()
        return
    full = lambda: ens.score_prepared(prep, True)
    for _ in range(3):
        full()
    torch.cuda.synchronize()
    f_med, f_min = timed(full, 20)
    print("batch: %d queries x 30 candidates = %d pairs, full models, precision 2, median (min) of 20 hipEvent-timed calls" % (1000, B))
    print("mms_score_ensemble                        %8.2f ms (%8.2f)  %7.0f pairs/s" % (f_med, f_min, B / f_med * 1e3))
    for keep in (5, 10, 15, 30):
        call = lambda: ens.score_prepared(prep, True, cascade=(gid, keep))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        med, mn = timed(call, 20)
        print("mms_score_ensemble_cascade keep=%-2d n_kept=%-6d %8.2f ms (%8.2f)  %7.0f pairs/s  %.2fx the full call" %
              (keep, ens.last_kept, med, mn, B / med * 1e3, f_med / med))
    f_med2, _ = timed(full, 20)
    print("mms_score_ensemble again (drift check)    %8.2f ms" % f_med2)
    ens.close()


if __name__ == "__main__":
    main()
