"""Timing of the device nDCG path (csrc/ndcg.hip) beside the host form, and of the file-fed valid pass.
usage (GPU box): python tools/ndcg_bench.py [records of the TSV part, 0 = skip] [model]
  1. hipEvent time of mms_ndcg_at_k (ndcg.ndcg_codes_device: median of 20 after 3 warm-ups, device-resident inputs, prebuilt AnswerKey) and wall
     time of ndcg.ndcg_from_arrays (once) / ndcg.ndcg_device (one read-back included, best of 5) on the same arrays: a valid-like table (496 queries, 14 720 rows)
     and a 2^22-row table (139 810 queries of 30).
  2. pipeline.evaluate_tsv_native in pairs/s on one synthetic TSV (the file of tools/e2e_tsv_bench.py) with both metrics and both label feeds,
     beside pipeline.stream_scores_tsv on the same file (best of 3 each)."""
import os
import sys
import time

import numpy as np
import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import featurizer as F, ndcg, pipeline, scorers, weights  # noqa: E402
from kddcup_2020_multimodalitiesrecall_2nd_place_amd.config import LdsConfig, LxmertConfig, ZkConfig  # noqa: E402

DEV = torch.device("cuda", 0)


def table(nq, per, seed):
    rng = np.random.default_rng(seed)
    q = np.repeat(np.arange(nq, dtype=np.int64) + 7, per)
    p = (1000000 + rng.integers(0, 40 * per, nq * per)).astype(np.int64)
    s = rng.random(nq * per, dtype=np.float32)
    key = {int(7 + i): p[i * per + rng.choice(per, 5, replace=False)].tolist() for i in range(nq)}
    return q, p, s, key


def time_table(name, q, p, s, key):
    ak = ndcg.AnswerKey(key, DEV)
    dq, dp, ds = (torch.from_numpy(x).to(DEV) for x in (q, p, s))
    ms = []
    for i in range(23):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ndcg.ndcg_codes_device(dq, dp, ds, ak, 5)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    t_dev = []
    for _ in range(5):
        t0 = time.perf_counter(); dev = ndcg.ndcg_device(dq, dp, ds, ak, 5); t_dev.append(time.perf_counter() - t0)
    t_dev = min(t_dev)
    t0 = time.perf_counter(); host = ndcg.ndcg_from_arrays(q, p, s, key, 5); t_host = time.perf_counter() - t0
    assert dev == host
    print("%s: %d rows, %d key queries: mms_ndcg_at_k %.3f ms (median of 20, min %.3f, max %.3f); ndcg_device incl. read-back %.2f ms (best of 5); "
          "ndcg_from_arrays %.1f ms; nDCG@5 %.6f (bit-equal)" % (name, len(q), len(key), float(np.median(ms)), min(ms), max(ms), t_dev * 1e3, t_host * 1e3, dev),
          flush=True)


q, p, s, key = table(496, 30, 1)
q, p, s = q[:14720], p[:14720], s[:14720]                 # the valid set's size; the key keeps the queries that still have rows
time_table("valid-like", q, p, s, {kq: t for kq, t in key.items() if kq <= int(q[-1])})
q, p, s, key = table(139810, 30, 2)
time_table("2^22-row", q, p, s, key)

n = int(sys.argv[1]) if len(sys.argv) > 1 else 14720
name = sys.argv[2] if len(sys.argv) > 2 else "zk"
if n > 0:
    D = os.path.join(R, "tests", "golden", "featurizer")
    VOCAB, TABLE = os.path.join(D, "vocab_small.txt"), F.load_label_table(os.path.join(D, "labels.txt"))
    path = "/tmp/ndcg_bench_%d.tsv" % n
    rng = np.random.default_rng(1)
    words = [w for w in open(VOCAB, encoding="utf-8").read().split() if not w.startswith("[") and w.isascii()]
    classes = [int(k) for k in TABLE]
    with open(path, "w") as f:
        f.write("product_id\timage_h\timage_w\tnum_boxes\tboxes\tfeatures\tclass_labels\tquery\tquery_id\n")
        feats_pool = np.maximum(rng.standard_normal((64, 10, 2048)), 0).astype(np.float32)
        for i in range(n):
            nb = int(np.clip(round(rng.lognormal(1.2, 0.5)), 1, 10))
            h, w = int(rng.integers(200, 1000)), int(rng.integers(200, 1000))
            boxes = np.sort(rng.uniform(0, 1, (nb, 4)), axis=1) * np.array([h, w, h, w])
            f.write(F.encode_record(i, h, w, boxes, feats_pool[i % 64, :nb], rng.choice(classes, nb), " ".join(rng.choice(words, int(rng.integers(2, 9)))), i // 30) + "\n")
    key = {int(g): rng.choice(np.arange(g * 30, min(n, g * 30 + 30)), min(5, n - g * 30), replace=False).tolist() for g in range((n + 29) // 30)}
    cfg = {"zk": ZkConfig, "lds": LdsConfig, "lxmert": LxmertConfig}[name]()
    sc = scorers.make_scorer(cfg, weights.make_weights(cfg), device=0)
    ak = ndcg.AnswerKey(key, DEV)

    def best(fn):
        out = []
        for _ in range(3):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            v = fn()
            out.append(time.perf_counter() - t0)
        return min(out), v

    pipeline.stream_scores_tsv(sc, path, VOCAB, TABLE)            # warm-up: featurizer lease, allocator
    t, _ = best(lambda: pipeline.stream_scores_tsv(sc, path, VOCAB, TABLE))
    print("%s, %d records: stream_scores_tsv %.0f pairs/s" % (name, n, n / t), flush=True)
    for metric in ("device", "host"):
        for labels in ("answer", "ones"):
            t, v = best(lambda: pipeline.evaluate_tsv_native(sc, path, VOCAB, TABLE, ak, metric=metric, labels=labels))
            print("%s, %d records: evaluate_tsv_native(metric=%s, labels=%s) %.0f pairs/s, nDCG@5 %.6f" % (name, n, metric, labels, n / t, v), flush=True)
    sc.close()
    os.remove(path)
