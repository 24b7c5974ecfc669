"""bench.py -- pairs scored per second on the headline workload of BASELINE.json.

Default workload (config.workload; BASELINE.json config 2, the configuration the metric is quoted on): imagebert_zk, full
12-layer / 768 / 3072 model, 1000 synthetic queries x 30 candidates PER GPU (<= 10 boxes x 2048-d fp32 features), inputs resident
in HBM before the timed region.  One "step" = one scoring pass over the rank's whole pair set -- feed preparation (struct
building, on-device label-tuple de-duplication), every kernel of the forward -- plus the all-gather of scores when N > 1
(queries are sharded by rank).  Prints ONE JSON line on rank 0.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--model zk|lds|lxmert|ensemble] [--precision 1|2|3|4]
                  [--workload bench|bench-strong|testB|valid] [--dense] [--all-boxes] [--dump-outputs DIR]
                  [--full [--no-cpu] [--no-secondary]]

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step, and the roofline read from the
same timed steps).  --full adds everything that takes runs of its own: the `cpu_baseline` (CPU port of the same forward, also a
check of the HIP logits), the `secondary` lines (H2D-inclusive and TSV-fed rates, precision 3, lds, lxmert, padded layout, box
sweep, shard rates, call latency) and, with --gpus N > 1, the `strong` accounting.  --no-cpu / --no-secondary drop parts of --full.
--dump-outputs DIR: after the timed steps, what the last step returned, as DIR/<name>.npy (float32): `scores` (the step's per-pair
score, gathered over the ranks when N > 1) and, for one model at N = 1, that call's `logits` and `probs` (pairs x 2).  Inputs and
weights are seeded, so two builds run with the same arguments can be compared output for output.

--gpus N > 1 without WORLD_SIZE in the environment: this process spawns the N ranks itself (one process per GPU, RCCL);
under torchrun / torch.distributed.run it uses the ranks it is given (and refuses a --gpus that contradicts WORLD_SIZE).
--workload bench-strong: the metric's own job -- ONE 1000-query x 30-candidate set -- cut into N contiguous query blocks (3750 pairs
per rank at N = 8: "candidate sets shard by query across the 8 GPUs").  With --gpus N > 1 --full the default (weak) run ALSO times
this job and reports it as `strong` in the same JSON line, so one invocation shows both accountings.
--workload testB | valid: the reference's file shapes -- 994 queries x 8..30 candidates (testB) / 496 x 9..30 (valid; zk then gets
the ground-truth label fed to its AM-softmax head, load_data_v4.py:259-263) = ONE job cut into contiguous query blocks (ragged
shards, strong scaling; run_pretraining_predict_score.py:566, prediction_result/*.txt).
--model ensemble: BASELINE.json config 5 -- zk, zk on the sen2forest rewrite, lds and lxmert on the same pairs through the
fused entry point (mms_score_ensemble); a "pair scored" then means scored by all four members and merged.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from kddcup_2020_multimodalitiesrecall_2nd_place_amd import scorers, sharding, synth, weights  # noqa: E402
from kddcup_2020_multimodalitiesrecall_2nd_place_amd.config import (FEAT_DIM, N_BOX, LdsConfig, LxmertConfig,  # noqa: E402
                                                                    ZkConfig, flops_per_pair)

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_FP8_TFLOPS = 5000.0   # dense MX-scaled fp8 MFMA peak (same guide): what precision mode 4's GEMMs are priced against
BASELINE_FLOPS = {"zk": 5.174e9, "lds": 6.886e9, "lxmert": 6.829e9}
CFGS = {"zk": ZkConfig, "lds": LdsConfig, "lxmert": LxmertConfig}
DTYPES = {1: "bf16 MFMA operands, 1 pass (weights bf16; activations bf16)",
          2: "bf16 MFMA operands (weights bf16; activations split hi+lo bf16, 2 passes), fp32 accumulate/residual/LN/softmax",
          3: "bf16 MFMA operands (weights and activations split hi+lo bf16, 3 passes), fp32 accumulate/residual/LN/softmax",
          4: "fp8 e4m3 MFMA operands on the encoder GEMMs, MX-scaled v_mfma_scale_f32_16x16x128_f8f6f4 (weights: per-channel hardware scale; "
             "activations e4m3), rest as mode 2"}


def device_feats(ps, device, seed):
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    f = torch.randn((ps.n, N_BOX, FEAT_DIM), device=device, dtype=torch.float32, generator=g).clamp_(min=0)
    live = torch.arange(N_BOX, device=device)[None, :] < torch.as_tensor(ps.num_boxes, device=device)[:, None]
    return f * live[:, :, None]


def device_feed(cfg_name, cfgs, ps, feats, dev, valid=False):
    """The rank's feed, every array already on the device in the dtype the library reads (so a step's prepare() is struct
    building only -- what a caller that keeps its candidate store in HBM pays per call)."""
    ps.feats = feats

    def dv(b):
        return {k: (torch.as_tensor(v).to(dev) if isinstance(v, np.ndarray) and v.dtype.kind in "fiu" else v) for k, v in b.items()}
    if cfg_name == "ensemble":
        lab = "valid" if valid else "testB"
        zb = synth.zk_batch(ps, cfgs["zk"].text_len, lab)
        zb2 = synth.zk_batch(synth.sen2forest_variant(ps), cfgs["zk"].text_len, lab)
        xb = synth.lxmert_batch(ps, cfgs["lxmert"].text_len)
        from kddcup_2020_multimodalitiesrecall_2nd_place_amd.pipeline import ensemble_feed
        f = ensemble_feed(zb, zb2, xb)
        f = {k: (v if torch.is_tensor(v) else torch.as_tensor(v).to(dev)) for k, v in f.items()}
        for k in ("num_boxes", "label_ids", "query_ids", "len_query", "s2f_query_ids", "s2f_len_query", "lx_input_ids", "lx_input_mask"):
            f[k] = f[k].to(torch.int32)
        return f
    b = dv(synth.batch_for(cfgs[cfg_name], ps, labels="valid") if (cfg_name == "zk" and valid) else synth.batch_for(cfgs[cfg_name], ps))
    key = {"zk": "np_images_features", "lds": "features", "lxmert": "feats"}[cfg_name]
    b[key] = feats
    return b


def prepare(scorer, name, b):
    if name == "ensemble":
        return scorer.prepare(b)
    if name == "zk":
        return scorer.prepare(b["num_boxes"], b["np_boxes_5"], b["np_images_features"], b["np_idx_class_labels"], b["np_idx_query_"],
                              b["len_query_"], b["labels"], b["segment_ids"])
    if name == "lds":
        return scorer.prepare(b)
    return scorer.prepare(b["input_ids"], b["boxes_label_input_ids"], b["input_mask"], b["feats"], b["boxes"],
                          b["visual_attention_mask"])


def live_fraction(name, cfgs, ps, dense):
    """Token rows the kernels execute / rows of the reference's padded graph (1.0 when token packing is off)."""
    if dense or name == "ensemble":
        return 1.0 if dense else None
    b0 = synth.batch_for(cfgs[name], ps)
    if name == "zk":
        live = (np.minimum(b0["len_query_"], cfgs["zk"].text_len) + np.minimum(b0["num_boxes"], N_BOX)).sum()
        return round(float(live) / (ps.n * cfgs["zk"].seq), 4)
    if name == "lxmert":
        return round(float(b0["input_mask"].sum() + b0["visual_attention_mask"].sum()) / (ps.n * (cfgs["lxmert"].text_len + N_BOX)), 4)
    # lds: rows kept after merging a pair's identical feature / label tokens (rowops.hip k_lds_plan_*)
    lab = b0["labelfeat"]
    nb = np.minimum(ps.num_boxes, N_BOX)
    distinct = np.array([len({tuple(t) for t in lab[i]}) for i in range(ps.n)])
    return round(float((cfgs["lds"].text_len + nb + (nb < N_BOX) + distinct).sum()) / (ps.n * cfgs["lds"].seq), 4)


def _host_topology():
    """(logical CPUs this process may use, physical cores among them, CPUs of NUMA node 0 among them)."""
    cpus = sorted(os.sched_getaffinity(0))
    phys, node0 = set(), []
    for c in cpus:
        try:
            phys.add(open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read().strip())
        except OSError:
            phys.add(str(c))
    try:
        txt = open("/sys/devices/system/node/node0/cpulist").read().strip()
        for part in txt.split(","):
            lo, _, hi = part.partition("-")
            node0 += [c for c in range(int(lo), int(hi or lo) + 1) if c in cpus]
    except (OSError, ValueError):
        node0 = list(cpus)
    return cpus, len(phys), node0 or list(cpus)


def _pin_all_threads(cpus):
    """CPU affinity of every thread of this process (OpenMP / BLAS workers exist already and keep theirs otherwise)."""
    for tid in os.listdir("/proc/self/task"):
        try:
            os.sched_setaffinity(int(tid), cpus)
        except OSError:
            pass


def cpu_baseline(cfg, w, hip_logits_fn=None, budget_s=20.0):
    """the oracle's fp32 port of the same forward on this box's host cores, on BASELINE.json config 1's shape (100
    queries x 30 candidates, batch 256), bounded to ~budget_s of CPU work.  Round 5 ran it on torch's default thread count (= every physical
    core of a two-socket host) and got HALF the rate of an 8-vCPU container: the port's batch-256 GEMMs do not feed 128 cores across two NUMA
    nodes.  Now: one batch per thread count in {8, 16, 32, 64 on one NUMA node; all physical cores}, then whole batches on the fastest
    setting until the budget is spent.  ``value`` / ``cores`` = that setting (the threads actually used); ``all_physical_cores`` = the
    protocol's "N = all physical cores" figure beside it.  The weights are converted once, outside the timed calls.  The sample's logits
    also serve as a CHECK of the HIP path (hip_logits_fn), never as its output."""
    from oracle import np_models, torch_models  # checker / baseline only
    ps = synth.make_pairs(100, 30, tag="/cpu")     # config 1: 3000 pairs
    b = synth.batch_for(cfg, ps)
    if cfg.name != "lxmert":
        tw = torch_models.prepare(w)
        run = lambda bb: torch_models.forward(cfg, tw, bb)
        blas = None
    else:
        run = lambda bb: np_models.forward(cfg, w, bb, np.float32)
        from threadpoolctl import threadpool_limits as blas
    cut = lambda lo, hi: {k: (v[lo:hi] if hasattr(v, "__len__") and len(v) == ps.n else v) for k, v in b.items()}
    cpus, n_phys, node0 = _host_topology()
    torch_default = torch.get_num_threads()

    def timed(threads, on_cpus, lo, hi):
        _pin_all_threads(on_cpus)
        torch.set_num_threads(threads)
        try:
            if blas is not None:
                with blas(limits=threads):
                    t0 = time.time(); out = run(cut(lo, hi)); dt = time.time() - t0
            else:
                t0 = time.time(); out = run(cut(lo, hi)); dt = time.time() - t0
        finally:
            _pin_all_threads(cpus)
            torch.set_num_threads(torch_default)
        return dt, np.asarray(out[0], np.float64)

    timed(min(8, len(cpus)), cpus, 0, 16)           # thread-pool / allocator warm-up, untimed
    settings = [(t, node0, "%d threads on NUMA node 0" % t) for t in (16, 8, 32, 64) if t <= len(node0) and t < n_phys]      # 16 first: the usual winner, measured even on a tight budget
    settings.append((n_phys, cpus, "%d threads = all physical cores" % n_phys))
    spent, sweep, probe = 0.0, [], min(256, ps.n)
    for k, (t, on, label) in enumerate(settings):
        if k and spent > 0.6 * budget_s:            # a slow host: keep what has been measured
            break
        dt, ref0 = timed(t, on, 0, probe)
        spent += dt
        sweep.append({"threads": t, "placement": label, "value": round(probe / dt, 2)})
    best = max(range(len(sweep)), key=lambda i: sweep[i]["value"])
    bt, bon, blabel = settings[best]
    done, dt_best, ref = probe, probe / sweep[best]["value"], [ref0 if best == len(sweep) - 1 else None]
    if ref[0] is None:                               # the best setting's own logits of the first batch (any setting's agree to fp32 round-off)
        ref = [timed(bt, bon, 0, probe)[1]]
    while done < ps.n and spent < budget_s:
        hi = min(done + 256, ps.n)
        dt, out = timed(bt, bon, done, hi)
        spent += dt; dt_best += dt
        ref.append(out)
        done = hi
    allp = [s_ for s_ in sweep if s_["threads"] == n_phys]
    res = {"value": round(done / dt_best, 2), "unit": "pairs/s", "cores": bt, "kind": "port",
           "best_threads": bt, "best_value": round(done / dt_best, 2), "placement": blabel,
           "all_physical_cores": ({"value": allp[0]["value"], "cores": n_phys} if allp else None), "thread_sweep": sweep,
           "host": {"logical_cpus": len(cpus), "physical_cores": n_phys, "numa_node0_cpus": len(node0)},
           "sample": "%d of config 1's 3000 pairs (100 queries x 30 candidates) in batches of 256, %s fp32 restatement of %s, %s (the fastest of "
                     "a one-batch sweep over %s threads), weights converted once outside the timed calls, %.1f s of CPU work in all"
                     % (done, "numpy (BLAS)" if cfg.name == "lxmert" else "torch", cfg.name, blabel, [s_["threads"] for s_ in sweep], spent)}
    if hip_logits_fn is not None:
        got = hip_logits_fn(cut(0, done))
        ref = np.concatenate(ref)
        res["hip_vs_port_max_vecrel"] = float((np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())
    return res


def make_members(name, a, local):
    """-> (scorer, {member name: (cfg, weights, member scorer)})"""
    kw = dict(device=local, chunk_pairs=a.chunk, **({} if a.fuse_ln < 0 else {"fuse_layernorm": a.fuse_ln}), fuse_attention="auto" if a.fuse_attn < 0 else a.fuse_attn)
    if name != "ensemble":
        cfg = CFGS[name]()
        w = weights.make_weights(cfg, bf16_matrices=not a.fp32_weights)
        s = scorers.make_scorer(cfg, w, precision=a.precision, pack_tokens=not a.dense, **kw)
        return s, {name: (cfg, w, s)}
    mem = {}
    for n in ("zk", "lds", "lxmert"):
        cfg = CFGS[n]()
        w = weights.make_weights(cfg, bf16_matrices=not a.fp32_weights)
        mem[n] = (cfg, w, scorers.make_scorer(cfg, w, precision=a.precision, pack_tokens=not a.dense, **kw))
    return scorers.EnsembleScorer(mem["zk"][2], mem["lds"][2], mem["lxmert"][2]), mem


def run_timed(step, steps, warmup, world, dev, handles):
    """W untimed + exactly K timed steps between barrier + synchronize, MAX over ranks; also one hipEvent pair per step on the
    stream the kernels run on (torch's current stream is the one handed to the library)."""
    for i in range(warmup):
        step(first=(i == 0))
    for h in handles:
        h.gemm_timing(True, True)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(steps):
        ev[i][0].record()
        step()
        ev[i][1].record()
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    dt = time.perf_counter() - t0
    per = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2])
    gms = gn = gfl = 0.0
    fused = [0.0, 0.0, 0.0]
    cls = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]           # GEMM launches by epilogue class: plain / fused LayerNorm
    side_fl = 0.0
    for h in handles:
        side_fl += h.side_lane_flops()                  # lxmert's distinct-query stage on the side lane: counted, not timed (before the reset below)
        for i, v in enumerate(h.fused_timing()):       # before the reset below
            fused[i] += v
        for c in (0, 1):
            for i, v in enumerate(h.gemm_timing_class(c)):
                cls[c][i] += v
        ms, n, fl = h.gemm_timing(False, True, read=True)
        gms += ms; gn += n; gfl += fl
    if dist.is_initialized():
        t = torch.tensor([dt, med], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, med = float(t[0].item()), float(t[1].item())
    return dt, med, gms, gn, gfl, fused + [cls, side_fl]


DUMP_BYTES = 64 << 20


def dump_outputs(path, last, world):
    """--dump-outputs: the arrays the last timed step returned, as float32 DIR/<name>.npy.  Past DUMP_BYTES in all, every array keeps
    the same seeded sample of pair rows (their indices in sample_rows.npy)."""
    torch.cuda.synchronize()
    arrs = {k: v.detach().float().cpu().numpy() for k, v in last.items() if world == 1 or k == "scores"}
    n = len(arrs["scores"])
    total = sum(x.nbytes for x in arrs.values())
    if total > DUMP_BYTES:
        keep = int(DUMP_BYTES // (total // n + 8))
        rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrs = {k: x[rows] for k, x in arrs.items()}
        arrs["sample_rows"] = rows.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, x in arrs.items():
        np.save(os.path.join(path, k + ".npy"), np.ascontiguousarray(x))


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: one child per GPU with the torchrun environment contract."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    for p in procs:
        rc = p.wait() or rc
    sys.exit(rc)


def batch_sweep(a, local, dev):
    """the three drop-in call surfaces at the reference's own call sizes -- zk 1 pair per sess.run
    (evaluate_normal.py:15,216), lds 5 (run_pretraining_predict_score.py:523), lxmert 256 (lxmert/src/param.py:46) -- and upwards.
    Inputs are device tensors (what a caller that keeps its candidate store in HBM passes); every call is followed by a stream
    synchronisation, so ms_per_call is the latency a caller sees, pairs/s = B / that."""
    out = {}
    sizes = (1, 5, 256, 1024, 4096, 30000)
    for name in ("zk", "lds", "lxmert"):
        cfg = CFGS[name]()
        w = weights.make_weights(cfg)
        s = scorers.make_scorer(cfg, w, precision=a.precision, device=local)
        whole = synth.make_pairs(1000, 30, tag="/bench0", with_feats=False)
        feats = device_feats(whole, dev, 20200823)
        rows = []
        for B in sizes:
            ps = whole.take(slice(0, B))
            fd = device_feed(name, {name: cfg}, ps, feats[:B], dev)

            def call():
                if name == "zk":
                    return s(fd["num_boxes"], fd["np_boxes_5"], fd["np_images_features"], fd["np_idx_class_labels"], None, fd["np_idx_query_"],
                             fd["len_query_"], fd["labels"], fd["segment_ids"])
                if name == "lds":
                    return s(fd)
                return s.forward(fd["input_ids"], fd["boxes_label_input_ids"], None, fd["input_mask"], None, None, fd["feats"], fd["boxes"],
                                 fd["visual_attention_mask"])
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            n, t0 = 0, time.perf_counter()
            while True:
                call()
                torch.cuda.synchronize()
                n += 1
                dt = time.perf_counter() - t0
                if (dt > 0.5 and n >= 3) or n >= 200:
                    break
            rows.append({"pairs_per_call": B, "calls": n, "ms_per_call": round(dt / n * 1e3, 4), "pairs_per_s": round(B * n / dt, 1)})
        big = rows[-1]["pairs_per_s"]
        for r in rows:
            r["of_large_batch_rate"] = round(r["pairs_per_s"] / big, 4)
        out[name] = rows
        s.close()
        del feats
    # ... and the fused three-model call (mms_score_ensemble: zk, zk on the rewritten query, lds, lxmert and the main.py:59 merge) at the same sizes
    cfgs = {n: CFGS[n]() for n in ("zk", "lds", "lxmert")}
    sc = {n: scorers.make_scorer(c, weights.make_weights(c), precision=a.precision, device=local) for n, c in cfgs.items()}
    ens = scorers.EnsembleScorer(sc["zk"], sc["lds"], sc["lxmert"])
    whole = synth.make_pairs(1000, 30, tag="/bench0", with_feats=False)
    feats = device_feats(whole, dev, 20200823)
    rows = []
    for B in (5, 256, 1024, 30000):
        fd = device_feed("ensemble", cfgs, whole.take(slice(0, B)), feats[:B], dev)
        for _ in range(2):
            ens.score_prepared(ens.prepare(fd), members=False)
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            ens.score_prepared(ens.prepare(fd), members=False)
            torch.cuda.synchronize()
            n += 1
            dt = time.perf_counter() - t0
            if (dt > 0.5 and n >= 3) or n >= 200:
                break
        rows.append({"pairs_per_call": B, "calls": n, "ms_per_call": round(dt / n * 1e3, 4), "pairs_per_s": round(B * n / dt, 1)})
    for r in rows:
        r["of_large_batch_rate"] = round(r["pairs_per_s"] / rows[-1]["pairs_per_s"], 4)
    out["ensemble"] = rows
    ens.close()
    del feats
    print(json.dumps({"metric": "per-call latency and pairs/s of the drop-in call surfaces by batch size", "unit": "pairs/s", "n_gpus": 1,
                      "precision_mode": a.precision, "data": "synthetic", "call_surface": {"zk": "ZkScorer.__call__ (13-argument model_attention_channel_e order)",
                      "lds": "LdsScorer.__call__(features)", "lxmert": "LxmertScorer.forward (KDDModel.forward order)",
                      "ensemble": "EnsembleScorer.score_prepared (mms_score_ensemble: four members + merge)"},
                      "reference_call_sizes": {"zk": 1, "lds": 5, "lxmert": 256}, "sweep": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="zk", choices=["zk", "lds", "lxmert", "ensemble"])
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--workload", default="bench", choices=["bench", "bench-strong", "testB", "valid"])
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--cands", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="also measure what takes runs of its own: cpu_baseline, the secondary lines and (N > 1) the strong-scaling job")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step returned to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of host CPU work spent on the cpu_baseline sample (default 20; the contract test uses less)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary lines (precision 3 on fp32 weights, lds, lxmert, H2D-inclusive)")
    ap.add_argument("--fp32-weights", action="store_true", help="seeded weights NOT rounded to bf16 (what a real checkpoint looks like)")
    ap.add_argument("--fuse-attn", type=int, default=-1, help="mms_config.fuse_attention (default: the LIBRARY default, scorers.make_scorer's \"auto\": 2 in precision mode 2, 1 in mode 3): QKV projection + attention in one kernel; 1 = exact-fp32 attention MFMAs (bit-identical to the two-kernel route), 2 = split-bf16 MFMAs")
    ap.add_argument("--box-mu", type=float, default=1.1, help="location of the lognormal box count of the synthetic pairs (1.1 = the documented workload, mean 3.5 boxes)")
    ap.add_argument("--batch-sweep", action="store_true", help="instead of the headline run: pairs/s and per-call latency of the three drop-in call surfaces at the reference's own call sizes")
    ap.add_argument("--fuse-ln", type=int, nargs="?", const=3, default=-1, help="LayerNorm fused into the N = 768 GEMM epilogues (mms_config.fuse_layernorm mask: 1 attention output, 2 FFN down, 3 both; default: the library default)")
    ap.add_argument("--dense", action="store_true", help="keep padded tokens (reference layout) instead of packing live tokens")
    ap.add_argument("--all-boxes", action="store_true", help="worst case: every pair has 10 boxes")
    a = ap.parse_args()
    a.fuse_attn_arg = a.fuse_attn
    if a.steps < 1:
        ap.error("--steps must be at least 1")

    if a.batch_sweep:
        torch.cuda.set_device(0)
        batch_sweep(a, 0, torch.device("cuda", 0))
        return
    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        spawn_ranks(a.gpus, sys.argv[1:])
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if world != a.gpus:
        sys.exit("bench.py: --gpus %d contradicts WORLD_SIZE=%d" % (a.gpus, world))
    if os.environ.get("MMS_BENCH_SHARE_GPU") or os.environ.get("MMS_BENCH_FORCE_LOCAL0"):
        # N ranks on ONE device: SHARE_GPU exercises the N > 1 path on a single-GPU box (tests); FORCE_LOCAL0 alone imitates a launcher
        # that failed to give each rank its own GPU -- the device check below must refuse it
        local = 0
    torch.cuda.set_device(local)
    # under a launcher (RANK / MASTER_PORT set) the process group comes up even for ONE rank and the step's score gather goes through the
    # collective: `torchrun --nproc-per-node 1 bench.py --gpus 1` runs the RCCL calls of an N-GPU job on a single-GPU box
    use_pg = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # backend "nccl" == RCCL over xGMI; MMS_BENCH_BACKEND=gloo (+ MMS_BENCH_SHARE_GPU=1) only exists for single-GPU test boxes
        # the process-group backends announce themselves on stdout ("[Gloo] Rank 0 is connected to ..."): the contract is ONE line
        sys.stdout.flush()
        keep = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group(os.environ.get("MMS_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(keep, 1)
            os.close(keep)
    dev = torch.device("cuda", local)
    backend = os.environ.get("MMS_BENCH_BACKEND", "nccl")
    gather_dev = dev if backend == "nccl" else torch.device("cpu")
    # N > 1: the line proves where its ranks ran -- every rank reports the device it holds; two "nccl" ranks on one device is an error
    # (only the single-GPU test mode, MMS_BENCH_SHARE_GPU + gloo, may share), not a silently meaningless scaling number
    rank_devices = None
    if use_pg:
        pr = torch.cuda.get_device_properties(local)
        me = {"rank": rank, "hip_device": local, "name": pr.name,
              "pci_bus_id": "%04x:%02x:%02x" % (getattr(pr, "pci_domain_id", 0), getattr(pr, "pci_bus_id", 0xff), getattr(pr, "pci_device_id", 0xff)),
              "uuid": str(getattr(pr, "uuid", "")), "host": socket.gethostname(), "pid": os.getpid()}
        rank_devices = [None] * world
        dist.all_gather_object(rank_devices, me)
        distinct = len({(d["host"], d["pci_bus_id"], d["uuid"]) for d in rank_devices})
        if distinct < world and not os.environ.get("MMS_BENCH_SHARE_GPU"):
            if rank == 0:
                print("bench.py: %d ranks resolved to %d distinct devices: %s" % (world, distinct, json.dumps(rank_devices)), file=sys.stderr)
            dist.destroy_process_group()
            sys.exit(3)

    scorer, members = make_members(a.model, a, local)
    fa_members = {n: (m[2].fuse_attention if a.precision in (2, 3) else 0) for n, m in members.items()}     # what the library default resolved to
    a.fuse_attn = fa_members["zk" if a.model == "ensemble" else a.model]
    cfgs = {n: m[0] for n, m in members.items()}
    handles = [m[2].handle for m in members.values()]
    def one_job(kind):
        """ONE job cut into contiguous query blocks per rank (strong scaling): testB 994 queries x 8..30 candidates, valid 496 x 9..30
        (prediction_result/*.txt / validscore_imagebert.txt; ragged shards), bench-strong = the metric's own 1000 x 30 set."""
        NQ, cr = {"testB": (994, (8, 30)), "valid": (496, (9, 30)), "bench-strong": (a.queries, a.cands)}[kind]
        whole = synth.make_pairs(NQ, cr, tag="/bench0" if kind == "bench-strong" else "/" + kind, with_feats=False, all_boxes=a.all_boxes, box_mu=a.box_mu)
        qop = whole.query_id - whole.query_id.min()
        lo, hi = sharding.query_block(NQ, world, rank)
        s, e = sharding.pair_slice_for_queries(qop, lo, hi)
        desc = ("%d queries x %d candidates (%d pairs)" % (NQ, cr, whole.n) if kind == "bench-strong" else
                "%s-like: %d queries x %d..%d candidates (%d pairs)" % (kind, NQ, cr[0], cr[1], whole.n))
        return whole.take(slice(s, e)), sharding.shard_sizes(qop, NQ, world), whole.n, desc + " cut into %d contiguous query blocks" % world

    if a.workload != "bench":
        ps, counts, total_pairs, wl = one_job(a.workload)
        scaling = "strong"
    else:
        # rank r owns queries [r*Q, (r+1)*Q) of the logical N*Q-query job (weak scaling)
        ps = synth.make_pairs(a.queries, a.cands, tag="/bench%d" % rank, with_feats=False, query_offset=rank * a.queries,
                              all_boxes=a.all_boxes, box_mu=a.box_mu)
        counts = [ps.n] * world
        total_pairs = ps.n * world
        scaling = "weak"
        wl = "%d queries x %d candidates per GPU" % (a.queries, a.cands)
    def make_step(ps_, counts_, valid=False):
        feats_ = device_feats(ps_, dev, 20200823 + rank)
        feed_ = device_feed(a.model, cfgs, ps_, feats_, dev, valid=valid)
        qid = torch.as_tensor(ps_.query_id, device=gather_dev)
        pid = torch.as_tensor(ps_.product_id, device=gather_dev)

        def score():
            prep = prepare(scorer, a.model, feed_)            # per-call feed preparation is part of the step
            if a.model == "ensemble":
                merged, _ = scorer.score_prepared(prep, members=False)
                return merged
            last["logits"], last["probs"] = scorer.score_prepared(prep)
            return last["probs"][:, 1].contiguous()

        def step(first=False):
            sc = score()
            if use_pg:
                sc = sc.to(gather_dev)
                out = sharding.gather_scores(sc, qid if first else None, pid if first else None, counts=counts_, force_collective=True)
            else:
                out = sc, None, None
            last["scores"] = out[0]
            return out
        return step, feats_, feed_

    last = {}               # what the most recent step returned (--dump-outputs)
    step, feats, feed = make_step(ps, counts, valid=a.workload == "valid")
    dt, med, gemm_ms, gemm_n, gemm_fl, fused = run_timed(step, a.steps, a.warmup, world, dev, handles)
    value = total_pairs * a.steps / dt
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, last, world)
    strong = None
    if world > 1 and a.workload == "bench" and a.full:
        # the same invocation, strong-scaling accounting: the metric's own 1000-query x 30-candidate job cut over the N ranks
        # (every rank takes part, so this runs on all ranks; rank 0 reports it)
        ps_s, counts_s, total_s, wl_s = one_job("bench-strong")
        step_s, _f, _fd = make_step(ps_s, counts_s)
        dt_s, med_s, _gm, _gn, _gf, _fu = run_timed(step_s, a.steps, a.warmup, world, dev, handles)
        strong = {"value": round(total_s * a.steps / dt_s, 1), "unit": "pairs/s", "scaling": "strong", "ms_per_step": round(dt_s / a.steps * 1e3, 3),
                  "workload": wl_s, "pairs_per_gpu": [int(c) for c in counts_s], "pairs_total": int(total_s)}
        del _f, _fd

    if rank == 0:
        achieved = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        fpp = sum(BASELINE_FLOPS[n] * (2 if n == "zk" and a.model == "ensemble" else 1) for n in members)
        for n, (cfg, _, _) in members.items():
            assert abs(flops_per_pair(cfg) / BASELINE_FLOPS[n] - 1) < 5e-3
        live_frac = live_fraction(a.model, cfgs, ps, a.dense)
        # HBM bytes per GEMM launch: NOT measured in this run (PMC passes need rocprofv3 around the process) -- the committed result of
        # tools/pmc_traffic.sh on this very workload, labelled as such
        traffic = traffic_src = fused_traffic = None
        tp = os.path.join(ROOT, "profiles", "pmc_traffic_%s.json" % a.model)
        if os.path.exists(tp) and not a.dense and a.precision == 2 and a.workload == "bench" and \
                json.load(open(tp)).get("fuse_attention", 0) == a.fuse_attn and \
                json.load(open(tp)).get("fuse_layernorm", 0) == next(iter(members.values()))[2].fuse_layernorm:
            traffic = round(json.load(open(tp))["hbm_bytes_per_launch"], 1)
            fused_traffic = json.load(open(tp)).get("fused_hbm_bytes_per_launch")
            traffic_src = "profiles/pmc_traffic_%s.json (builder's rocprofv3 --pmc run of this workload, FETCH_SIZE x 2 + WRITE_SIZE; not re-measured here)" % a.model
        avg_launch_s = gemm_ms * 1e-3 / max(gemm_n, 1)
        kern = {1: "gemm_pp_kernel<1,*,0,true> 256x256 ping-pong phases, persistent", 2: "gemm_pp_kernel<2,*,0,true> 256x256 ping-pong phases, persistent",
                3: "gemm_ppw_kernel<*> 256x128 ping-pong phases, 3 passes", 4: "gemm_mx8_kernel<*> 256x256 ping-pong phases, 128-k super-stages of MX-scaled fp8 MFMAs"}[a.precision]
        peak = PEAK_FP8_TFLOPS if a.precision == 4 else PEAK_BF16_TFLOPS
        res = {
            "metric": "query-image pairs scored/sec (whole node)", "value": round(value, 1), "unit": "pairs/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
            "ms_per_step_median_hipevent": round(med, 3),
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": DTYPES[a.precision] + ("; fused self-attention: Q K^T / P V on split-bf16 MFMAs (hi + lo operands, 3 products)" if a.fuse_attn == 2 and a.precision in (2, 3) else ""),
            "data": "synthetic",
            "config": {"workload": ("imagebert_%s 12-layer, " % a.model if a.model in ("zk", "lds") else
                                    "lxmert 9/5/5, " if a.model == "lxmert" else
                                    "3-model ensemble (imagebert_zk on the query and on its sen2forest rewrite + imagebert_lds + lxmert, fused entry point), ")
                                   + wl + " (<=10 boxes x 2048-d), seeded weights%s, inputs HBM-resident" % (" (fp32, not bf16-rounded)" if a.fp32_weights else ""),
                       "pairs_per_gpu": ps.n, "pairs_total": total_pairs, "precision_mode": a.precision,
                       "parallelism": "query-sharded dp%d" % world,
                       "token_packing": not a.dense, "live_token_fraction": live_frac},
            # pairs/s x the reference graph's padded-shape FLOPs/pair.  With token packing the
            # kernels EXECUTE fewer FLOPs than that (padded tokens are skipped), so this is an equivalent rate, not
            # a utilisation; roofline.achieved below counts executed FLOPs only.
            "reference_graph_tflops_per_gpu": round(value / world * fpp / 1e12, 2),
            "roofline": {"bound": "mfma", "kernel": kern + (" (all dense contractions" if not a.fuse_attn else " (attention-output / FFN / box and label projections; Q|K|V projections: fused_qkv_attention below") + "; small GEMMs: gemm_tile_kernel)",
                         "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_src,
                         # the second resource of the same launches: traffic / 6.3 TB/s (achievable HBM rate, MI355X_MICROARCH.md) over the
                         # average launch -- MFMA issue time and this add up to most of a launch
                         "hbm_time_frac": round(traffic / 6.3e12 / avg_launch_s, 4) if traffic and avg_launch_s > 0 else None,
                         # SURVEY.md section 8(d)'s literal accounting: pairs/s x the PADDED reference graph's FLOPs per pair / peak.  Token packing
                         # skips the padded rows, so this is an equivalent rate of the reference graph, not a utilisation of this chip
                         "frac_reference_graph": round(value / world * fpp / 1e12 / peak, 4),
                         "launches": int(gemm_n), "avg_launch_ms": round(gemm_ms / max(gemm_n, 1), 4),
                         "algorithmic_flops_per_launch": round(gemm_fl / max(gemm_n, 1), 1),
                         "note": "achieved = sum over GEMM launches of executed 2*M_live*N*K (device-counted) / sum of hipEvent "
                                 "launch durations in the timed region (rank 0); traffic = PMC HBM bytes per launch from profiles/"},
        }
        res["config"]["fuse_attention"] = a.fuse_attn if a.model != "ensemble" else fa_members
        res["config"]["fuse_layernorm"] = next(iter(members.values()))[2].fuse_layernorm if a.precision == 2 else 0
        if fused[1] > 0:
            # mms_config.fuse_attention: the QKV projections run inside qkv_attn_kernel, whose launches also do the attention of their
            # pairs -- timed apart from the GEMM launches above, priced on the projection FLOPs alone
            f_ach = fused[2] / (fused[0] * 1e-3) / 1e12
            res["roofline"]["fused_qkv_attention"] = {
                "kernel": ("qkv_attn2_kernel (8 x 1 waves) 256x192 tile (one head of [Q|K|V]) + in-LDS split-bf16 attention" if a.fuse_attn == 2 and a.precision == 2
                           else "qkv_attn_kernel<*,%s> 256x192 tile (one head of [Q|K|V]) + in-LDS attention" % ("true" if a.fuse_attn == 2 else "false")),
                "launches": int(fused[1]), "avg_launch_ms": round(fused[0] / fused[1], 4),
                "achieved": round(f_ach, 2), "frac": round(f_ach / peak, 4),
                "traffic": round(fused_traffic, 1) if fused_traffic else None,
                "note": "projection FLOPs (2*M_live*2304*768) / launch duration INCLUDING the attention of the tile's pairs"}
            res["roofline"]["achieved_incl_fused"] = round((gemm_fl + fused[2]) / ((gemm_ms + fused[0]) * 1e-3) / 1e12, 2)
            res["roofline"]["frac_incl_fused"] = round(res["roofline"]["achieved_incl_fused"] / peak, 4)
        cls = fused[3]
        if cls[1][1] > 0:
            # mms_config.fuse_layernorm: the attention-output / FFN-down projections run with the bias + residual + LayerNorm epilogue; those
            # launches' duration includes the eight residual K stages and the LayerNorm (work the two-kernel route does in k_ln_to_planes),
            # their FLOP count the projection alone -- reported apart so that `plain_epilogue` stays comparable with earlier rounds
            for key, c, what in (("plain_epilogue", cls[0], "gemm_pp_kernel<2,ACT,0,true,false>: FFN-up (+GELU), box / label projections, small launches"),
                                 ("layernorm_fused", cls[1], "gemm_pp_kernel<2,0,0,true,true>: attention-output and FFN-down projections + residual + LayerNorm in one launch")):
                if c[1] > 0:
                    t = c[2] / (c[0] * 1e-3) / 1e12
                    res["roofline"][key] = {"kernel": what, "launches": int(c[1]), "avg_launch_ms": round(c[0] / c[1], 4), "achieved": round(t, 2), "frac": round(t / peak, 4)}
                    if key == "layernorm_fused" and traffic is not None:
                        res["roofline"][key]["traffic"] = json.load(open(tp)).get("ln_fused_hbm_bytes_per_launch")
        # the whole step on the same terms: every executed dense-contraction FLOP (device-counted) over the barrier-bracketed step time
        step_fl = (gemm_fl + fused[2] + fused[4]) / max(a.steps, 1)      # (fused[4]: launches on a side lane -- in the step's work, in no per-launch sum)
        res["roofline"]["whole_step"] = {"executed_flops": round(step_fl, 1), "ms_per_step": round(dt / a.steps * 1e3, 3),
                                         "achieved": round(step_fl / (dt / a.steps) / 1e12, 2), "frac": round(step_fl / (dt / a.steps) / 1e12 / peak, 4),
                                         "note": "all kernels of the step (GEMMs, fused QKV + attention, row kernels, bookkeeping) in the denominator"}
        if strong is not None:
            res["strong"] = strong
        if use_pg:
            try:
                ccl = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
            except Exception:        # noqa: BLE001 -- a version string is not worth a failed bench
                ccl = None
            res["ranks"] = rank_devices
            res["distributed"] = {"backend": backend + (" (RCCL)" if backend == "nccl" else ""), "rccl_version": ccl,
                                  "distinct_devices": len({(d["host"], d["pci_bus_id"], d["uuid"]) for d in rank_devices}),
                                  "shared_device_test_mode": bool(os.environ.get("MMS_BENCH_SHARE_GPU")),
                                  "gather": "one all_gather_into_tensor of fp32 scores per step on %s tensors" % ("device" if backend == "nccl" else "host")}
        if a.full and world == 1 and not a.no_secondary and a.workload == "bench":
            res["secondary"] = secondary(a, local, dev, ps, feats, members, scorer, feed, value)
            if "precision3" in res["secondary"]:
                # the real-checkpoint mode as a top-level value of the line: the same batch scored by a zk handle whose
                # weights are NOT bf16-rounded (precision "auto" -> mode 3), with its parity against the oracle's fp32 port on the timed batch
                res["value_fp32_checkpoint"] = res["secondary"]["precision3"]
        if a.full and world == 1 and not a.no_cpu:
            n0 = "zk" if a.model == "ensemble" else a.model
            cfg0, w0, s0 = members[n0]

            def hip_logits(bb):
                lg, _ = scorers.score_batch(s0, bb)
                return lg.double().cpu().numpy()
            res["cpu_baseline"] = cpu_baseline(cfg0, w0, hip_logits, budget_s=a.cpu_budget)
        print(json.dumps(res), flush=True)
    scorer.close()
    if use_pg:
        dist.destroy_process_group()


def tsv_pipeline_rate(scorer, records=120000):
    """The caller-side pipeline with every stage overlapped (pipeline.stream_scores_tsv): a synthetic valid/testB-like TSV file
    (the reference's wire format, load_data_v4.py:133-163; mean 3.8 boxes per record) -> libmmfeat decode threads -> rotating
    pinned buffers -> H2D on a copy stream -> the scorer.  This is the PCIe-inclusive rate a file-fed caller sees; never `value`."""
    import tempfile
    from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer as F, pipeline
    D = os.path.join(ROOT, "tests", "golden", "featurizer")
    vocab, table = os.path.join(D, "vocab_small.txt"), F.load_label_table(os.path.join(D, "labels.txt"))
    rng = np.random.default_rng(1)
    words = [w for w in open(vocab, encoding="utf-8").read().split() if not w.startswith("[") and w.isascii()]
    classes = [int(k) for k in table]
    pool = np.maximum(rng.standard_normal((64, N_BOX, FEAT_DIM)), 0).astype(np.float32)
    fd, path = tempfile.mkstemp(suffix=".tsv", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        with os.fdopen(fd, "w") as f:
            f.write("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n")
            for i in range(records):
                nb = int(np.clip(round(rng.lognormal(1.2, 0.5)), 1, N_BOX))
                h, w = int(rng.integers(200, 1000)), int(rng.integers(200, 1000))
                boxes = np.sort(rng.uniform(0, 1, (nb, 4)), axis=1) * np.array([h, w, h, w])
                f.write(F.encode_record(i, h, w, boxes, pool[i % 64, :nb], rng.choice(classes, nb),
                                        " ".join(rng.choice(words, int(rng.integers(2, 9)))), i // 30) + "\n")
        size = os.path.getsize(path)
        best, host = 0.0, {}
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stt = {}
            _q, _p, sc = pipeline.stream_scores_tsv(scorer, path, vocab, table, batch_pairs=16384, stats=stt)
            torch.cuda.synchronize()
            rate = len(sc) / (time.perf_counter() - t0)
            if rate > best:
                best, host = rate, {k: round(v * 1e3, 1) for k, v in stt.items() if k.endswith("_s")}
        # the host side alone: the same file through libmmfeat into reused pinned buffers, nothing consuming them
        from kddcup_2020_multimodalitiesrecall_2nd_place_amd.featurizer_native import NativeFeaturizer
        nf = NativeFeaturizer(vocab, table, scorer.cfg.name, pinned=True, reuse_buffers=True, pools=3)
        feat = 0.0
        for _ in range(3):
            t0 = time.perf_counter()
            k = sum(len(b_["query_id"]) for b_ in nf.iter_file(path, 8192))
            feat = max(feat, k / (time.perf_counter() - t0))
        nf.close()
        # ... and the device side alone on the same records (what the file-fed rate is to be compared with: these records carry 3.8 boxes each)
        nf = NativeFeaturizer(vocab, table, scorer.cfg.name)
        devb = []
        for b_ in nf.iter_file(path, 8192):
            devb.append({k: (torch.from_numpy(np.array(v)).to(scorer.device) if isinstance(v, np.ndarray) and v.dtype.kind in "fiu" else v)
                         for k, v in b_.items() if k not in ("query_id", "product_id", "keep")})
            if len(devb) == 3:
                break
        nf.close()
        resident = 0.0
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _r in range(3):
                for d_ in devb:
                    scorers.score_batch(scorer, d_)
            torch.cuda.synchronize()
            resident = max(resident, 9 * 8192 / (time.perf_counter() - t0))
        del devb
    finally:
        os.remove(path)
    return {"value": round(best, 1), "unit": "pairs/s", "featurizer_alone_records_per_s": round(feat, 1),
            "device_resident_same_records": round(resident, 1), "fraction_of_device_resident": round(best / resident, 4),
            "host_ms": host,      # of the best pass: waiting for a decoded batch / for its H2D copy / enqueueing (incl. the call's one read-back) / final drain
            "note": "TSV file (%d records, %.2f GB) -> native featurizer threads -> pinned buffers -> H2D on a copy stream -> scorer, all "
                    "overlapped (pipeline.stream_scores_tsv, batches of 16384 after a 1024 / 2048 / 4096 / 8192 ramp); %d host threads, the decode on "
                    "up to 32 of them" % (records, size / 1e9, os.cpu_count())}


def secondary(a, local, dev, ps, feats, members, scorer, feed, value):
    """Numbers the driver would otherwise never see (N = 1 only, a few seconds each): the H2D-inclusive rate of the headline
    workload, the fp32-checkpoint-faithful mode on UNROUNDED weights with its measured parity, and the other two models."""
    out = {}
    # ---- headline workload, features copied from pinned host memory inside the step (not overlapped) ----
    key = {"zk": "np_images_features", "lds": "features", "lxmert": "feats", "ensemble": "feats"}[a.model]
    host = torch.empty(feats.shape, dtype=torch.float32, pin_memory=True)
    host.copy_(feats)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        f2 = dict(feed)
        f2[key] = host.to(dev, non_blocking=True)
        p = prepare(scorer, a.model, f2)
        scorer.score_prepared(p, members=False) if a.model == "ensemble" else scorer.score_prepared(p)
    torch.cuda.synchronize()
    out["value_incl_h2d"] = {"value": round(ps.n * reps / (time.perf_counter() - t0), 1), "unit": "pairs/s",
                             "note": "same step + H2D of the fp32 box features (%.2f GB per pass) from pinned memory, not overlapped" % (feats.numel() * 4 / 1e9)}
    del host
    if a.model != "zk" or a.precision != 2:
        return out
    out["tsv_to_scores_overlapped"] = tsv_pipeline_rate(scorer)

    def oracle_parity(cfg, w, s, fd, n):
        """checker: the oracle's fp32 port on 64 pairs OF THE TIMED BATCH ITSELF (the logits the big-M engines just produced -- a separate
        small batch would run the small-tile engines instead)"""
        from oracle import np_models, torch_models
        sel = np.linspace(0, n - 1, 64).astype(np.int64)
        tsel = torch.as_tensor(sel, device=dev)
        sub = {k: (v[tsel].cpu().numpy() if torch.is_tensor(v) and v.shape[:1] == (n,) else v) for k, v in fd.items()}
        if cfg.name == "lxmert":
            ref = np.asarray(np_models.forward(cfg, w, sub, np.float32)[0], np.float64)
        else:
            ref = np.asarray(torch_models.forward(cfg, w, sub)[0], np.float64)
        got = s.logits[tsel].double().cpu().numpy()
        return float((np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())

    def timed(s, name, cfg, ps_, feats_, steps=3):
        fd = device_feed(name, {name: cfg}, ps_, feats_, dev)
        def st(first=False):
            s.score_prepared(prepare(s, name, fd))
        dt, med, gms, gn, gfl, _fu = run_timed(st, steps, 1, 1, dev, [s.handle])
        return fd, {"value": round(ps_.n * steps / dt, 1), "unit": "pairs/s", "precision_mode": s.precision, "fuse_attention": s.fuse_attention,
                    "gemm_tflops": round(gfl / (gms * 1e-3) / 1e12, 1), "frac": round(gfl / (gms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)}

    def quick(name, precision, fp32_weights, note=None, cpu=False, **skw):
        cfg = CFGS[name]()
        w = weights.make_weights(cfg, bf16_matrices=not fp32_weights)
        s = scorers.make_scorer(cfg, w, precision=precision, device=local, chunk_pairs=a.chunk,
                                fuse_attention="auto" if a.fuse_attn_arg < 0 else a.fuse_attn_arg, **skw)
        fd, r = timed(s, name, cfg, ps, feats)
        r["parity_max_vecrel_vs_fp32_port"] = oracle_parity(cfg, w, s, fd, ps.n)
        r["parity_sample"] = "64 pairs of the timed %d-pair launch (its own logits)" % ps.n
        if note:
            r["weights"] = note
        s.close()
        if cpu and not a.no_cpu:
            # VERDICT r4 item 7 / BASELINE.md section 3: the same model's CPU restatement timed on this box's host cores (bounded sample, as the line's cpu_baseline)
            r["cpu_port"] = cpu_baseline(cfg, w, None, budget_s=max(2.0, a.cpu_budget / 2))
        return r
    out["precision3"] = quick("zk", "auto", True, "seeded fp32, NOT bf16-rounded (a real checkpoint's situation); precision auto -> mode 3")
    out["lds"] = quick("lds", 2, False, cpu=True)
    out["lxmert"] = quick("lxmert", 2, False, cpu=True)
    # ---- SURVEY.md section 8(d)'s other workload shapes on the same code: the reference's padded layout, the all-10-boxes worst case, and
    # how the rate moves with the box count (live_token_fraction is a property of the synthetic distribution, not of the kernels) ----
    zcfg, zw, zs = members["zk"]
    out["dense"] = quick("zk", 2, False, pack_tokens=False)
    out["dense"]["live_token_fraction"] = 1.0
    sweep = []
    for mu in (0.3, 1.1, 1.8, 2.2, None):          # None: every pair has 10 boxes
        if mu == 1.1:
            ps_, f_ = ps, feats
        else:
            ps_ = synth.make_pairs(a.queries, a.cands, tag="/bench0", with_feats=False, all_boxes=mu is None, box_mu=mu or 1.1)
            f_ = device_feats(ps_, dev, 20200823)
        fd, r = timed(zs, "zk", zcfg, ps_, f_)
        r.update({"box_mu": mu, "mean_boxes_per_pair": round(float(np.minimum(ps_.num_boxes, N_BOX).mean()), 2),
                  "live_token_fraction": live_fraction("zk", {"zk": zcfg}, ps_, False)})
        if mu is None:
            r["parity_max_vecrel_vs_fp32_port"] = oracle_parity(zcfg, zw, zs, fd, ps_.n)
            out["all_boxes"] = r
        sweep.append(r)
        del fd, f_
    out["box_sweep"] = sweep
    # ---- one GPU's share of the strong-scaling jobs at N = 8 (the metric's 1000 x 30 set: 125 queries = 3750 pairs; testB: 994 queries /
    # 8 ranks): what a rank of the 8-GPU run does per step, so that the SCALE line has a stated expectation ----
    shard = {}
    for kind, NQ, cr in (("bench_strong_n8", a.queries, a.cands), ("testB_n8", 994, (8, 30))):
        whole = synth.make_pairs(NQ, cr, tag="/bench0" if kind.startswith("bench") else "/testB", with_feats=False)
        qop = whole.query_id - whole.query_id.min()
        lo, hi = sharding.query_block(NQ, 8, 0)
        s0, e0 = sharding.pair_slice_for_queries(qop, lo, hi)
        ps_ = whole.take(slice(s0, e0))
        f_ = device_feats(ps_, dev, 20200823)
        fd, r = timed(zs, "zk", zcfg, ps_, f_, steps=10)
        shard[kind] = {"pairs_rank0": ps_.n, "value_one_gpu": r["value"], "predicted_strong_8": round(8 * r["value"], 1), "unit": "pairs/s",
                       "note": "rank 0's query block of the N = 8 job scored alone on this GPU; 8 x that = the 8-GPU rate if ranks do not disturb each other (the gather is 15 KB per rank)"}
        del fd, f_
    out["shard_rates"] = shard
    # ---- the reference's own call sizes through the same handle (zk scores ONE pair per sess.run, evaluate_normal.py:15; lds 5, lxmert 256): latency of a
    # synchronised call; `--batch-sweep` has the three models and the larger sizes ----
    whole = synth.make_pairs(9, 30, tag="/bench0", with_feats=False)
    f_all = device_feats(whole, dev, 20200823)
    calls = {}
    for B in (1, 5, 256):
        ps_ = whole.take(slice(0, B))
        fd = device_feed("zk", {"zk": zcfg}, ps_, f_all[:B], dev)
        for _ in range(3):
            zs.score_prepared(prepare(zs, "zk", fd))
        torch.cuda.synchronize()
        n, t0 = 100, time.perf_counter()
        for _ in range(n):
            zs.score_prepared(prepare(zs, "zk", fd))
            torch.cuda.synchronize()
        calls[str(B)] = round((time.perf_counter() - t0) / n * 1e3, 4)
    out["call_latency_ms"] = {"model": "zk", "pairs_per_call": calls, "note": "one synchronised scoring call of B pairs (device-resident inputs); small launches run on gemm_skinny.hip / split-K tiles (DESIGN.md section 3)"}
    return out


if __name__ == "__main__":
    main()
