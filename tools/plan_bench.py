"""Ensemble plans against their yardsticks, mms_score_ensemble and mms_score_ensemble_cascade(keep=10) in the same process on the same batch: hipEvent
time of each on the 1000 x 30 bench batch (full models, precision 2), median of 20 calls each, with the pairs every stage scored.
  python tools/plan_bench.py                 the table (profiles/rd21_plan.txt)
  python tools/plan_bench.py --trace         warm-up + 5 calls of the plan lxmert(10) -> zk(5) -> lds and nothing else: the workload of a kernel trace
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o plan -- python tools/plan_bench.py --trace
  python tools/plan_bench.py --stats CSV     the share of that trace's kernel time spent in select + scatter + gather
The model weights are seeded, not trained: the times and the counts of the keep rules do not depend on them, the count a safe rule prunes does (it is
printed, whatever it is), and what a plan costs in nDCG needs trained checkpoints (ensemble.plan_curve on a valid set).
"""
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (k_gather_rows also serves the second zk member's changed pairs: an upper bound; k_plan_scan and k_zk_plan_* are the token plan's, not these plans')
OVERHEAD = ("k_cas_", "k_plan_scatter", "k_plan_bounds", "k_plan_merge", "k_gather_rows")
TRACED = [("lxmert", 10), ("zk", 5), ("lds", None)]

PLANS = [
    ("all members (overhead over the full call)", [("zk+lds+lxmert", None)]),
    ("the cascade's plan, keep 10", [("lxmert", 10), ("zk+lds", None)]),
    ("zk+lxmert alone", [("zk+lxmert", None)]),
    ("lxmert(10) -> zk(5) -> lds", TRACED),
    ("lxmert(15) -> zk(5) -> lds", [("lxmert", 15), ("zk", 5), ("lds", None)]),
    ("lxmert+zk(safe 5) -> lds", [("lxmert+zk", ("safe", 5)), ("lds", None)]),
]


def stats(path):
    total = over = 0.0
    rows = []
    for r in csv.DictReader(open(path)):
        ns = float(r["TotalDurationNs"])
        total += ns
        if any(t in r["Name"] for t in OVERHEAD):
            over += ns
            rows.append((ns, int(r["Calls"]), r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]))
    print("kernel trace of the plan lxmert(10) -> zk(5) -> lds: %.1f ms of kernels, %.3f ms (%.2f %%) in select + scatter + gather:" % (total / 1e6, over / 1e6, 100 * over / total))
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
        return statistics.median(ms), min(ms), max(ms)

    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        for _ in range(2 + 5):
            ens.score_prepared(prep, True, plan=(gid, TRACED))
        torch.cuda.synchronize()
        return

    def measure(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return timed(call, 20)

    full = lambda: ens.score_prepared(prep, True)
    f_med, f_min, f_max = measure(full)
    print("batch: %d queries x 30 candidates = %d pairs, full models (seeded weights), precision 2, median (min .. max) of 20 hipEvent-timed calls" % (1000, B))
    print("%-46s %8.2f ms (%8.2f .. %8.2f)  %7.0f pairs/s" % ("mms_score_ensemble", f_med, f_min, f_max, B / f_med * 1e3))
    c_med, c_min, c_max = measure(lambda: ens.score_prepared(prep, True, cascade=(gid, 10)))
    print("%-46s %8.2f ms (%8.2f .. %8.2f)  %7.0f pairs/s  n_kept=%d" % ("mms_score_ensemble_cascade keep=10", c_med, c_min, c_max, B / c_med * 1e3, ens.last_kept))
    for name, plan in PLANS:
        med, mn, mx = measure(lambda: ens.score_prepared(prep, True, plan=(gid, plan)))
        print("%-46s %8.2f ms (%8.2f .. %8.2f)  %7.0f pairs/s  %.2fx the full call, %.2fx the cascade  scored=%s" %
              ("plan " + name, med, mn, mx, B / med * 1e3, f_med / med, c_med / med, ens.last_scored))
    f_med2, f_min2, f_max2 = timed(full, 20)
    print("%-46s %8.2f ms (%8.2f .. %8.2f)" % ("mms_score_ensemble again (drift check)", f_med2, f_min2, f_max2))
    ens.close()


if __name__ == "__main__":
    main()
