"""Predict drivers: TSV records -> featurizer -> HIP scorer -> score file, i.e. what ``code/main.py`` launches per
sub-model (code/imagebert_zk/evaluate_normal.py:222-252, code/imagebert_lds/src/run_pretraining_predict_score.py:566-589,
code/lxmert/src/tasks/kdd_model.py:46-129), batched instead of 1 / 5 / 256 pairs per framework call.
The written files are what ``ensemble.ensemble`` (main.py's merge) consumes.
"""
from __future__ import annotations

import contextlib
import os
import queue
import threading
import time

import numpy as np
import torch

from . import featurizer as F
from . import scorefile
from .featurizer_native import FEAT_TEXT_KEYS, NativeFeaturizer, decode_features
from .scorers import score_batch


def score_records(scorer, records, batch_pairs: int = 8192):
    """Returns (query_id[B], product_id[B], score[B]) with score = softmax(logit)[:, 1]
    (evaluate_normal.py:242-243 / run_pretraining_predict_score.py:573-575 / kdd_model.py:102-112)."""
    name = scorer.cfg.name
    make = {"zk": F.zk_batch, "lds": F.lds_batch, "lxmert": F.lxmert_batch}[name]
    scores = []
    for s in range(0, len(records), batch_pairs):
        chunk = records[s:s + batch_pairs]
        _, probs = score_batch(scorer, make(chunk, scorer.cfg.text_len))
        scores.append(probs[:, 1].float().cpu().numpy())
    qid = np.array([r.query_id for r in records], np.int64)
    pid = np.array([r.product_id for r in records], np.int64)
    return qid, pid, (np.concatenate(scores) if scores else np.zeros(0, np.float32))


def predict_tsv(scorer, tsv_lines, label_table, tokenizer, out_path, sen2forest: bool = False, batch_pairs: int = 8192):
    """Featurise TSV lines (header lines containing 'product_id' are skipped like kdd_data.py:70-71), score, write."""
    records = [F.read_line(l, label_table, tokenizer, sen2forest) for l in tsv_lines if l.strip() and "product_id" not in l]
    qid, pid, score = score_records(scorer, records, batch_pairs)
    if scorer.cfg.name == "lxmert":
        scorefile.write_score_csv(out_path, qid, pid, score)
    else:
        scorefile.write_score_tsv(out_path, qid, pid, score)
    return qid, pid, score


def kdd_predict(scorer, tsv_lines, label_table, tokenizer, save_path=None, batch_pairs: int = 8192):
    """``KDD.predict(mod, save)`` of the lxmert sub-model (code/lxmert/src/tasks/kdd_model.py:46-129) over already-read TSV lines:
    returns ``(match_pred, match_label, rank_score_pred)`` -- the arg-max class per pair (``:112``), the fed target (1 for every
    row, kdd_data.py:74) and ``{query_id: [(product_id, softmax(logit)[-1]), ...]}`` (``:107-110``) -- and with ``save_path``
    writes the ``query-id,product-id,score`` CSV of ``:114-128`` grouped by query in first-seen order like the reference's dict walk."""
    import collections
    records = [F.read_line(l, label_table, tokenizer) for l in tsv_lines if l.strip() and "product_id" not in l]
    qid, pid, score = score_records(scorer, records, batch_pairs)
    match_pred = [int(s > 0.5) for s in score]           # argmax of a two-class softmax
    match_label = [1] * len(records)
    rank_score_pred = collections.defaultdict(list)
    for q, p, s in zip(qid, pid, score):
        rank_score_pred[int(q)].append((int(p), float(s)))
    if save_path is not None:
        rows = [(q, p, s) for q, items in rank_score_pred.items() for p, s in items]
        scorefile.write_score_csv(save_path, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    return match_pred, match_label, rank_score_pred


_FEATURIZERS: dict = {}                  # key -> NativeFeaturizer, least recently used first
_FEATURIZER_CACHE = 6
_BUSY: set = set()                       # keys of the cached featurizers that a pass holds
_CACHE_LOCK = threading.Lock()
_COPY_STREAMS: dict = {}


def _copy_stream(dev):
    """ONE H2D stream per device for the life of the process: torch's caching allocator keeps a pool per stream, so a fresh stream per call would reserve
    a fresh set of batch buffers per call (2.6 GB per pass of stream_scores_tsv, never reused: tools/soak_tsv.py)."""
    key = (dev.type, dev.index)
    if key not in _COPY_STREAMS:
        _COPY_STREAMS[key] = torch.cuda.Stream(dev)
    return _COPY_STREAMS[key]


@contextlib.contextmanager
def _lease(vocab_path, label_table, threads, *specs):
    """-> the NativeFeaturizers of ``specs`` ((model, want_feats, feat_decode) each), busy until the block ends, by an exception or not.  One is
    cached per (vocabulary, label table, model, threads, want_feats, feat_decode) -- helper threads + three pinned buffer sets, ~2 GB at 8192-record
    batches, as costly to make as decoding 30 000 records --, at most ``_FEATURIZER_CACHE``, the least recently used evicted first.  A busy one is
    never evicted nor handed out twice: a busy key, or a miss with no idle entry to evict, gets a private featurizer, closed when the block ends."""
    labels = tuple(sorted((int(k), v) for k, v in label_table.items()))
    held = []                            # (featurizer, its cache key or None: a private one)
    try:
        with _CACHE_LOCK:
            for model, want_feats, feat_decode in specs:
                key = (os.path.abspath(vocab_path), os.path.getmtime(vocab_path), model, threads, want_feats, feat_decode, labels)
                nf = None if key in _BUSY else _FEATURIZERS.pop(key, None)
                if nf is None:
                    idle = [] if key in _BUSY else [k for k in _FEATURIZERS if k not in _BUSY]
                    for k in idle[:max(0, len(_FEATURIZERS) + 1 - _FEATURIZER_CACHE)]:     # make room, least recently used first
                        _FEATURIZERS.pop(k).close()
                    nf = NativeFeaturizer(vocab_path, label_table, model, threads=threads, pinned=True, reuse_buffers=True, pools=3,
                                          want_feats=want_feats, feat_decode=feat_decode)
                cached = key not in _BUSY and len(_FEATURIZERS) < _FEATURIZER_CACHE
                if cached:
                    _FEATURIZERS[key] = nf       # (re)inserted last: the most recently used
                    _BUSY.add(key)
                held.append((nf, key if cached else None))
        yield [nf for nf, _ in held]
    finally:
        with _CACHE_LOCK:
            for nf, key in held:
                if key is None:
                    nf.close()
                _BUSY.discard(key)


@contextlib.contextmanager
def _background(source):
    """``with _background(source) as items: for x in items: ...`` -- ``source`` (an iterable) runs on a producer thread one item ahead of the
    consumer (a depth-1 queue: one item waiting, one being produced, one being consumed -- the featurizers' three buffer sets); a producer error
    is raised in the consumer.  However the block ends, the producer is told to stop, the queue drained and the thread joined; ``source``'s
    iterator is closed on the producer thread (a generator's ``finally`` runs there: ``iter_spans`` unmaps its file)."""
    q, stop, it, end = queue.Queue(maxsize=1), threading.Event(), iter(source), object()

    def produce():
        try:
            for x in it:
                q.put(x)
                if stop.is_set():
                    return
            q.put(end)
        except BaseException as e:       # surfaced in the consumer
            q.put(e)
        finally:
            getattr(it, "close", lambda: None)()

    def consume():
        while (x := q.get()) is not end:
            if isinstance(x, BaseException):
                raise x
            yield x

    th = threading.Thread(target=produce, daemon=True)
    th.start()
    try:
        yield consume()
    finally:
        stop.set()
        while th.is_alive():             # unblock a pending put until the producer has seen the stop
            with contextlib.suppress(queue.Empty):
                q.get(timeout=0.01)
        th.join()


def _overlapped_pass(batches, dev, feat_key, score):
    """The three overlapped stages of the file-fed drivers (``stream_scores_tsv``).  ``batches`` (run by ``_background``): (query_id copy,
    product_id copy, dict of host arrays) per batch; a dict with ``FEAT_TEXT_KEYS`` gets ``decode_features``' output under ``feat_key``;
    ``score(device dict)`` enqueues the batch's kernels.  -> (query_id, product_id, [score(d) per batch], stats); raises on a bad device-decoded
    record.  However the pass ends, the producer has stopped and the copy stream is synchronised before this returns or raises."""
    copy_stream = _copy_stream(dev)
    clock = time.perf_counter
    qids, pids, outs, bads = [], [], [], []
    t_get = t_h2d = t_enq = 0.0          # host seconds waiting for a decoded batch / for its H2D copy / enqueueing its kernels
    h2d_bytes = 0
    with _background(batches) as items:
        try:
            while True:
                t0 = clock()
                item = next(items, None)
                t_get += clock() - t0
                if item is None:
                    break
                qids.append(item[0])
                pids.append(item[1])
                with torch.cuda.stream(copy_stream):
                    d = {k: (torch.from_numpy(v).to(dev, non_blocking=True) if isinstance(v, np.ndarray) and v.dtype.kind in "fiu" else v)
                         for k, v in item[2].items()}
                h2d_bytes += sum(t.numel() * t.element_size() for t in d.values() if torch.is_tensor(t))
                t0 = clock()
                copy_stream.synchronize()    # the pinned set may be refilled from here on; the scoring stream is still busy with the previous batch
                t1 = clock()
                for t in d.values():         # allocated on the copy stream, consumed on the scoring one: defer reuse of the memory
                    if torch.is_tensor(t):
                        t.record_stream(torch.cuda.current_stream(dev))
                if FEAT_TEXT_KEYS[0] in d:   # on the scoring stream, in front of the scorer's kernels: no host thread waits for it
                    d[feat_key], bad = decode_features(d, dev)
                    bads.append(bad)
                outs.append(score(d))
                t_h2d += t1 - t0
                t_enq += clock() - t1
        finally:
            copy_stream.synchronize()        # no DMA still reads a pinned set when the featurizer goes back to the cache
    t0 = clock()
    torch.cuda.current_stream(dev).synchronize()
    hit = torch.nonzero(torch.cat(bads)).flatten().tolist() if bads else []         # the device decode's per-batch bad flags, one read-back
    if hit:
        raise ValueError("record %d of the pass (product_id %d): bad base64 in features (decoded on the device; %d bad record(s))"
                         % (hit[0], int(np.concatenate(pids)[hit[0]]), len(hit)))
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
    return cat(qids), cat(pids), outs, dict(wait_decode_s=t_get, wait_h2d_s=t_h2d, enqueue_s=t_enq, drain_s=clock() - t0, batches=len(outs),
                                            h2d_bytes=h2d_bytes)


def tsv_shard(nf, tsv_path, rank: int, world: int):
    """A rank's share of a TSV file that all ranks of a node read (BASELINE.json config 4): contiguous QUERY blocks
    (``sharding.query_block`` over the file's queries in file order -- valid.tsv / testB.tsv are grouped by query), found from the records'
    last field alone (``NativeFeaturizer.query_ids``: line split, no decode).  -> ((first record, end record), records per rank): every rank
    computes the same list, so the score gather needs no size exchange (``sharding.gather_scores(counts=...)``)."""
    from . import sharding
    qid = nf.query_ids(tsv_path)
    if qid.size == 0:
        return (0, 0), [0] * world
    first = np.concatenate([[0], np.flatnonzero(qid[1:] != qid[:-1]) + 1, [qid.size]])       # record index at which each query group starts (+ the end)
    n_groups = len(first) - 1
    bounds = [sharding.query_block(n_groups, world, r) for r in range(world)]
    counts = [int(first[hi] - first[lo]) for lo, hi in bounds]
    lo, hi = bounds[rank]
    return (int(first[lo]), int(first[hi])), counts


def decode_threads_for(world: int) -> int:
    """libmmfeat threads of ONE rank when ``world`` ranks share the host (one featurizer per rank, each decoding only its shard): half of an equal share
    of the physical cores, at most the single-consumer default (32), at least 4 -- on the MI355X box's 128-core host 32 / 32 / 16 / 8 threads for 1 / 2 / 4 /
    8 ranks.  More is slower there: eight ranks decode 763 / 584-690 / 400 k records/s in all with 8 / 16 / 32 threads each (profiles/rd6_feat_sweep.txt)."""
    import os as _os
    cpus = len(_os.sched_getaffinity(0)) if hasattr(_os, "sched_getaffinity") else (_os.cpu_count() or 8)
    return int(max(4, min(32, cpus // 4 // max(world, 1))))


def stream_scores_tsv(scorer, tsv_path, vocab_path, label_table, sen2forest: bool = False, batch_pairs: int = 32768, threads: int = 0,
                      ramp: int = 1024, shard=None, shard_by: str = "bytes", stats: dict = None, feat_decode: str = "host"):
    """TSV file -> (query_id, product_id, score) with the three stages overlapped:

      producer thread   libmmfeat decodes batch i+2 into one of three pinned buffer sets (ctypes releases the GIL)
      copy stream       H2D of batch i+1 (pinned -> device, waited for on the host, which then frees that buffer set)
      main stream       the scorer's kernels for batch i (asynchronous; nothing on the host waits for them until the end)

    ``ramp``: the first batches hold ramp, 2 ramp, 4 ramp ... records (0: every batch ``batch_pairs``): the GPU starts after ~4 ms of
    host work instead of the ~27 ms a 8192-record batch takes to decode and copy -- 4 % of a 150 000-record file, a fifth of testB.
    The featurizer (its helper threads and pinned buffer sets) is kept per (vocabulary, model, threads) between calls.

    ``shard = (rank, world)``: this process scores only its share of the file with ``decode_threads_for(world)`` decode threads unless ``threads``
    says otherwise, and returns a 4th value ``counts`` for ``sharding.gather_scores``.  ``shard_by="bytes"`` (default): the file is cut at query
    boundaries near size * r / world (``NativeFeaturizer.byte_shard``: O(1) per rank, shards balanced by decode work; ``counts`` is None -- the gather
    exchanges the sizes).  ``shard_by="queries"``: equal numbers of queries per rank (``tsv_shard``: every rank indexes the whole file first -- an
    index pass per rank that costs more than the decode from ~4 ranks on, profiles/rd6_feat_sweep.txt -- and gets the static ``counts`` list).

    ``feat_decode="device"``: the featurizer gathers the box features' base64 text instead of decoding it (~42 KB per record over PCIe instead
    of 80 KB), the copy stream carries it with the other arrays, and ``featurizer_native.decode_features`` runs on the scoring stream in front of
    the scorer's kernels.  Scores are bit-identical to the host mode's; a record whose text is not base64 raises ValueError (naming it) before
    the pass returns.
    """
    qid, pid, probs, counts = _model_pass(scorer, tsv_path, vocab_path, label_table, sen2forest, batch_pairs, threads, ramp, shard, shard_by, stats,
                                          feat_decode)
    score = torch.cat(probs).float().cpu().numpy() if probs else np.zeros(0, np.float32)
    if shard is not None:
        return qid, pid, score, counts
    return qid, pid, score


def _answer_labels(key):
    """-> a hook for the passes below: the batch's ``labels`` feed (zk's AM-softmax margin reads it) becomes the ground-truth 0/1 of the batch's own
    (query, product) ids against the answer key, computed on the scoring stream in front of the scorer's kernels (``ndcg.relevance_device``) --
    what the reference feeds on valid (load_data_v4.py:259-263).  A feed without ``labels`` (lds, lxmert) is left as it is."""
    from . import ndcg

    def hook(d):
        if "labels" in d:
            d["labels"] = ndcg.relevance_device(d["_query_id"], d["_product_id"], key)
        return d
    return hook


def _relabel(labels, rank_label, device, fed=True):
    """-> (rank_label, relabel): with ``labels == "answer"`` (and a model that is ``fed`` labels) the key as an ``ndcg.AnswerKey`` on ``device`` and
    the ``_answer_labels`` hook on it; otherwise the key as it came and no hook."""
    from . import ndcg
    if labels != "answer" or not fed:
        return rank_label, None
    key = rank_label if isinstance(rank_label, ndcg.AnswerKey) else ndcg.AnswerKey(rank_label, device)
    return key, _answer_labels(key)


def _model_pass(scorer, tsv_path, vocab_path, label_table, sen2forest, batch_pairs, threads, ramp, shard, shard_by, stats, feat_decode, relabel=None):
    """The overlapped pass of ``stream_scores_tsv`` with the scores left on the device: -> (query_id, product_id, [softmax(logit)[:, 1] per batch],
    counts).  ``relabel`` (``_answer_labels``): the batch's ids travel to the device with it and the hook rewrites the device feed before scoring."""
    if feat_decode not in ("host", "device"):
        raise ValueError("feat_decode must be 'host' or 'device', not %r" % (feat_decode,))
    if shard is not None and threads <= 0:
        threads = decode_threads_for(shard[1])
    with _lease(vocab_path, label_table, threads, (scorer.cfg.name, True, feat_decode)) as (nf,):
        before = dict(nf.stats)
        records = counts = byte_range = None
        if shard is not None and shard_by == "queries":
            records, counts = tsv_shard(nf, tsv_path, shard[0], shard[1])
        elif shard is not None:
            byte_range = nf.byte_shard(tsv_path, shard[0], shard[1])

        def batches():
            for b in nf.iter_file(tsv_path, batch_pairs, sen2forest, ramp=ramp, records=records, byte_range=byte_range):
                q, pr = b.pop("query_id").copy(), b.pop("product_id").copy()
                if relabel is not None:
                    b = {**b, "_query_id": q, "_product_id": pr}
                yield q, pr, b

        score = (lambda d: score_batch(scorer, d)[1][:, 1]) if relabel is None else (lambda d: score_batch(scorer, relabel(d))[1][:, 1])
        qid, pid, probs, st = _overlapped_pass(batches(), scorer.device, nf.FEAT_KEY[nf.model], score)
        if stats is not None:
            stats.update(st, featurizer={k: v - before.get(k, 0.0) for k, v in nf.stats.items()})
    return qid, pid, probs, counts


def _metric(qid, pid, score, rank_label, k, metric, sharded, info):
    """nDCG@k of a pass: ``metric="device"``: ``ndcg.ndcg_device`` on the device scores (one small read); ``"host"``: ``ndcg.ndcg_from_arrays`` on
    their copy.  The same value.  ``sharded``: -> (histogram, key queries evaluated) of this rank's rows for ``sharding.reduce_ndcg``."""
    from . import ndcg
    if metric == "device":
        return ndcg.ndcg_device(qid, pid, score, rank_label, k, info=info, allow_missing=sharded, return_hist=sharded)
    label_dict = rank_label.rank_label if isinstance(rank_label, ndcg.AnswerKey) else rank_label
    host = score.cpu().numpy()
    if info is not None:
        info.update(path="host", flags=0)
    if sharded:
        codes = ndcg.ndcg_codes(qid, pid, host, label_dict, k, allow_missing=True)
        return ndcg.hist_from_codes(codes, k), int((codes >= 0).sum())
    return ndcg.ndcg_from_arrays(qid, pid, host, label_dict, k)


def _check_eval_args(metric, labels):
    if metric not in ("host", "device"):
        raise ValueError("metric must be 'host' or 'device', not %r" % (metric,))
    if labels not in ("answer", "ones"):
        raise ValueError("labels must be 'answer' or 'ones', not %r" % (labels,))


def evaluate_tsv_native(scorer, tsv_path, vocab_path, label_table, rank_label, k: int = 5, metric: str = "device", labels: str = "answer",
                        sen2forest: bool = False, batch_pairs: int = 32768, threads: int = 0, ramp: int = 1024, shard=None, shard_by: str = "bytes",
                        stats: dict = None, feat_decode: str = "host", info: dict = None, scores_out: dict = None):
    """A valid TSV file -> nDCG@k against the answer key ``rank_label`` (``{query: [products]}`` or an ``ndcg.AnswerKey``), the reference's valid
    protocol: the pass of ``stream_scores_tsv`` (same streaming arguments) with the scores left on the device.

    ``labels="answer"`` (default): the label feed of the model -- zk's AM-softmax margin depends on it -- is the ground truth of each batch's
    own ids, looked up in the answer key on the GPU (``ndcg.relevance_device``), as the reference feeds it on valid; ``labels="ones"`` keeps the
    testB convention of ``stream_scores_tsv`` (every label 1).  lds and lxmert read no label: the same scores either way.
    ``metric="device"``: ranking per key query on the GPU (``ndcg.ndcg_device``), one small host read; ``metric="host"``: ``ndcg.ndcg_from_arrays``
    on the copied scores.  Both return the same float, bit for bit.
    ``shard = (rank, world)``: this rank's rows only; the result is ``(histogram, key queries evaluated)`` for ``sharding.reduce_ndcg`` +
    ``ndcg.ndcg_from_hist`` instead of the float.  ``info`` receives the metric's ``{"path", "flags"}``; ``scores_out`` (a dict) receives
    ``query_id`` / ``product_id`` (numpy) and ``score`` (device fp32)."""
    _check_eval_args(metric, labels)
    rank_label, relabel = _relabel(labels, rank_label, scorer.device, scorer.cfg.name == "zk")
    qid, pid, probs, _ = _model_pass(scorer, tsv_path, vocab_path, label_table, sen2forest, batch_pairs, threads, ramp, shard, shard_by, stats,
                                     feat_decode, relabel)
    score = torch.cat(probs).float() if probs else torch.zeros(0, dtype=torch.float32, device=scorer.device)
    if scores_out is not None:
        scores_out.update(query_id=qid, product_id=pid, score=score)
    return _metric(qid, pid, score, rank_label, k, metric, shard is not None, info)


def predict_tsv_native(scorer, tsv_path, vocab_path, label_table, out_path, sen2forest: bool = False, batch_pairs: int = 32768,
                       threads: int = 0, feat_decode: str = "host"):
    """``predict_tsv`` with the native featurizer (libmmfeat), decode / H2D / scoring overlapped -- same scores, same file
    (``feat_decode``: see ``stream_scores_tsv``)."""
    qid, pid, score = stream_scores_tsv(scorer, tsv_path, vocab_path, label_table, sen2forest, batch_pairs, threads, feat_decode=feat_decode)
    (scorefile.write_score_csv if scorer.cfg.name == "lxmert" else scorefile.write_score_tsv)(out_path, qid, pid, score)
    return qid, pid, score


def ensemble_feed(zk_feed: dict, s2f_feed: dict, lx_feed: dict) -> dict:
    """The fused entry point's feed (``scorers.EnsembleScorer.prepare``) from the three per-model featurizer batches of the
    SAME records: image side and label ids once (zk layout), the two zk query variants, the lxmert-flavour query."""
    return {"feats": zk_feed["np_images_features"], "boxes_5": zk_feed["np_boxes_5"], "num_boxes": zk_feed["num_boxes"],
            "label_ids": zk_feed["np_idx_class_labels"], "query_ids": zk_feed["np_idx_query_"], "len_query": zk_feed["len_query_"],
            "s2f_query_ids": s2f_feed["np_idx_query_"], "s2f_len_query": s2f_feed["len_query_"], "labels": zk_feed["labels"],
            "lx_input_ids": lx_feed["input_ids"], "lx_input_mask": lx_feed["input_mask"]}


class EnsembleScorer:
    """BASELINE.json config 5, TSV records -> merged scores: the three models score the same pair shard on the same GPU in ONE
    library call (``scorers.EnsembleScorer`` -> ``mms_score_ensemble``) and are merged pre-gather with main.py:59's weights, so
    the exchange step stays one fp32 per pair.

    ``zk`` is used twice -- once on the query as given, once on the ``sen2forest`` rewrite (evaluate_normal_sen2fs.py,
    load_data_v4.py:153-154) -- exactly the four tables main.py merges.  The product-uniqueness filter is global over
    queries and therefore runs on rank 0 after the gather (``ensemble.uniqueness_filter``).

    The fused call reads ONE label-id tensor; the TF-flavour and the lxmert-flavour tokenizer must therefore agree on the class
    names (they differ only in ``max_input_chars_per_word`` and the never-split specials, neither of which a class name hits);
    ``score_lines`` checks it on every batch.
    """

    WEIGHTS = (0.2, 0.2, 0.3, 0.3)

    def __init__(self, zk, lds, lxmert, weights=None):
        from .scorers import EnsembleScorer as Fused
        self.zk, self.lds, self.lxmert = zk, lds, lxmert
        self.fused = Fused(zk, lds, lxmert, self.WEIGHTS if weights is None else weights)

    @property
    def weights(self):
        return self.fused.weights

    def set_weights(self, w):
        """The merge weights of the following passes (``scorers.EnsembleScorer.set_weights``), e.g. the winner of ``fit_weights_tsv_native``."""
        self.fused.set_weights(w)

    def _score(self, zk_feed, s2f_feed, lx_feed, cascade=None, plan=None):
        merged, mem = self.fused(ensemble_feed(zk_feed, s2f_feed, lx_feed), cascade=cascade, plan=plan)[:2]
        return merged.double().cpu().numpy(), tuple(m for m in mem.cpu().numpy())

    @staticmethod
    def _cascade_info(info, kept, offsets):
        if info is not None:
            info.update(cascade_kept=int(kept), cascade_pairs=int(offsets[-1]), batch_offsets=[int(o) for o in offsets])

    @staticmethod
    def _check_plan(plan, cascade_keep=None, normalize="none"):
        """``plan=`` of the drivers -> the normalised plan (``ensemble.plan``) or None; not together with ``cascade_keep`` or a normalisation."""
        if plan is None:
            return None
        from . import ensemble
        if cascade_keep is not None:
            raise ValueError("plan= with cascade_keep: the cascade is the plan [(\"lxmert\", keep), (\"zk+lds\", None)]; give one")
        if normalize != "none":
            raise ValueError("plan= with normalize=%r: a member that was not computed is zero, which has no meaning on a normalised scale" % (normalize,))
        return ensemble.plan(plan)

    @staticmethod
    def _plan_info(info, scored, offsets):
        if info is not None:
            info.update(plan_scored=[int(c) for c in scored], batch_offsets=[int(o) for o in offsets])

    def score_lines(self, tsv_lines, label_table, tok_tf, tok_hf, batch_pairs: int = 8192, cascade_keep: int = None, info: dict = None, plan=None):
        """tok_tf: WordPieceTokenizer as the TF sub-projects build it; tok_hf: the lxmert (HF) flavour.
        ``cascade_keep``: the cascade form of the fused call (``scorers.EnsembleScorer.score_prepared(cascade=)``) with each batch's query ids;
        ``info`` then receives ``cascade_kept`` / ``cascade_pairs`` (pairs through stage 2 / all pairs) and ``batch_offsets``.
        ``plan``: the plan form (``score_prepared(plan=)``; stages as ``ensemble.plan`` takes them) with each batch's query ids; ``info`` then
        receives ``plan_scored`` (the pairs each stage scored, summed over the batches) and ``batch_offsets``.  Not together with ``cascade_keep``."""
        plan = self._check_plan(plan, cascade_keep)
        scored = [0] * len(plan or ())
        lines = [l for l in tsv_lines if l.strip() and "product_id" not in l]
        rec = [F.read_line(l, label_table, tok_tf) for l in lines]
        rec_s2f = [F.read_line(l, label_table, tok_tf, sen2forest=True) for l in lines]
        rec_hf = [F.read_line(l, label_table, tok_hf) for l in lines]
        merged, parts = [], [[], [], [], []]
        kept_pairs = 0
        for s in range(0, len(rec), batch_pairs):
            zf = F.zk_batch(rec[s:s + batch_pairs], self.zk.cfg.text_len)
            lf = F.lxmert_batch(rec_hf[s:s + batch_pairs], self.lxmert.cfg.text_len)
            if not np.array_equal(zf["np_idx_class_labels"], lf["boxes_label_input_ids"]):
                raise ValueError("the two tokenizer flavours disagree on a class name: the fused entry point takes one label-id tensor")
            cascade = None if cascade_keep is None else (np.array([r.query_id for r in rec[s:s + batch_pairs]], np.int64), cascade_keep)
            pl = None if plan is None else (np.array([r.query_id for r in rec[s:s + batch_pairs]], np.int64), plan)
            m, p4 = self._score(zf, F.zk_batch(rec_s2f[s:s + batch_pairs], self.zk.cfg.text_len), lf, cascade, pl)
            kept_pairs += self.fused.last_kept if cascade is not None else 0
            if plan is not None:
                scored = [a + b for a, b in zip(scored, self.fused.last_scored)]
            merged.append(m)
            for k in range(4):
                parts[k].append(p4[k])
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        qid = np.array([r.query_id for r in rec], np.int64)
        pid = np.array([r.product_id for r in rec], np.int64)
        if cascade_keep is not None:
            self._cascade_info(info, kept_pairs, list(range(0, len(rec), batch_pairs)) + [len(rec)])
        if plan is not None:
            self._plan_info(info, scored, list(range(0, len(rec), batch_pairs)) + [len(rec)])
        return qid, pid, cat(merged, np.float64), tuple(cat(x, np.float32) for x in parts)

    def _tsv_pass(self, tsv_path, vocab_path, label_table, batch_pairs, threads, feat_decode, members, relabel=None, cascade_keep=None, info=None,
                  plan=None):
        """The overlapped pass of the file-fed ensemble drivers with the outputs left on the device: -> (query_id, product_id, per batch: (merged,
        member scores or None without ``members``)).  ``relabel``: see ``_answer_labels``.  ``cascade_keep``: the batch's query ids go to the device
        with the feed and the fused call runs in its cascade form (a query cut by a batch boundary is selected per part); ``info`` receives
        ``cascade_kept`` / ``cascade_pairs`` and the pass's ``batch_offsets``.  ``plan`` (normalised, ``_check_plan``): the same with the plan form;
        ``info`` receives ``plan_scored`` and ``batch_offsets``."""
        if feat_decode not in ("host", "device"):
            raise ValueError("feat_decode must be 'host' or 'device', not %r" % (feat_decode,))
        # (kept between calls like stream_scores_tsv's; the fused feed reads the 2048-d features from the first pass only, the other two flavours skip their decode)
        with _lease(vocab_path, label_table, threads, ("zk", True, feat_decode), ("zk", False, "host"), ("lxmert", False, "host")) as (nf_zk, nf_s2f, nf_lx):

            def batches():
                for span in nf_zk.iter_spans(tsv_path, batch_pairs, ramp=1024):      # (ramp: the first fused call starts after 1024 records)
                    zf = nf_zk.featurize_spans(*span)
                    feed = ensemble_feed(zf, nf_s2f.featurize_spans(*span, True), nf_lx.featurize_spans(*span))
                    q, pr = zf["query_id"].copy(), zf["product_id"].copy()
                    ids = {} if relabel is None else {"_query_id": q, "_product_id": pr}
                    if cascade_keep is not None or plan is not None:
                        ids["_query_id"] = q
                    yield q, pr, {**feed, **{k: zf[k] for k in FEAT_TEXT_KEYS if k in zf}, **ids}

            def score(d):
                prep = self.fused.prepare(d if relabel is None else relabel(d))
                if plan is not None:
                    res = self.fused.score_prepared(prep, members, plan=(d["_query_id"], plan))
                    scored[:] = [a + b for a, b in zip(scored, self.fused.last_scored)]
                    offsets.append(offsets[-1] + int(res[0].shape[0]))
                    return res[:2]
                if cascade_keep is None:
                    return self.fused.score_prepared(prep) if members else self.fused.score_prepared(prep, False)
                res = self.fused.score_prepared(prep, members, cascade=(d["_query_id"], cascade_keep))
                kept[0] += self.fused.last_kept
                offsets.append(offsets[-1] + int(res[0].shape[0]))
                return res[:2]

            kept, offsets, scored = [0], [0], [0] * len(plan or ())
            qid, pid, out, _ = _overlapped_pass(batches(), self.zk.device, "feats", score)
            if cascade_keep is not None:
                self._cascade_info(info, kept[0], offsets)
            if plan is not None:
                self._plan_info(info, scored, offsets)
        return qid, pid, out

    def _merged_pass(self, tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out, metric="device",
                     cascade_keep=None, info=None, plan=None):
        """A pass over a valid file that leaves the MERGED scores on the device, the zk members' label feed as ``labels`` says: -> (query_id,
        product_id, score fp64 [n], the relabelled key); ``scores_out`` receives ``query_id`` / ``product_id`` / ``score``."""
        _check_eval_args(metric, labels)
        rank_label, relabel = _relabel(labels, rank_label, self.zk.device)
        qid, pid, out = self._tsv_pass(tsv_path, vocab_path, label_table, batch_pairs, threads, feat_decode, members=False, relabel=relabel,
                                       cascade_keep=cascade_keep, info=info, plan=plan)
        score = torch.cat([m for m, _ in out]).double() if out else torch.zeros(0, dtype=torch.float64, device=self.zk.device)
        if scores_out is not None:
            scores_out.update(query_id=qid, product_id=pid, score=score)
        return qid, pid, score, rank_label

    def _member_pass(self, tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out):
        """The same pass with the four MEMBER scores left on the device: -> (query_id, product_id, members fp32 [4, n], the pass's batch offsets,
        the relabelled key); ``scores_out`` receives ``query_id`` / ``product_id`` / ``members``."""
        _check_eval_args("device", labels)
        rank_label, relabel = _relabel(labels, rank_label, self.zk.device)
        qid, pid, out = self._tsv_pass(tsv_path, vocab_path, label_table, batch_pairs, threads, feat_decode, members=True, relabel=relabel)
        mem = torch.cat([m for _, m in out], 1) if out else torch.zeros((4, 0), dtype=torch.float32, device=self.zk.device)
        if scores_out is not None:
            scores_out.update(query_id=qid, product_id=pid, members=mem)
        return qid, pid, mem, np.cumsum([0] + [int(m.shape[0]) for m, _ in out]).tolist(), rank_label

    @staticmethod
    def _check_normalize(normalize, cascade_keep=None):
        from . import ensemble
        ensemble._check_normalize(normalize)
        if normalize != "none" and cascade_keep is not None:
            raise ValueError("normalize=%r with cascade_keep: a pruned pair's zero members have no meaning on a normalised scale" % (normalize,))

    def _normalized_merge(self, qid, mem, normalize, info=None):
        """The merge the fits grade, on the device: the members [4, n] of a WHOLE file normalised per query (``ensemble.normalize_members_device``: a
        query cut by a batch boundary is still one group), then ``ndcg.merge_members``'s arithmetic with the scorer's weights in fp64 -- one
        elementwise kernel per product and per sum, so nothing can be contracted.  -> device fp64 [n]."""
        from . import ensemble
        nm = ensemble.normalize_members_device(qid, mem, normalize)
        if info is not None:
            info["normalize"] = normalize
        w = [float(x) for x in self.weights]
        acc = nm[0].double() * w[0]
        for m in range(1, nm.shape[0]):
            prod = nm[m].double() * w[m]
            acc = acc + prod
        return acc

    def evaluate_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, k: int = 5, metric: str = "device", labels: str = "answer",
                            batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", info: dict = None, scores_out: dict = None,
                            cascade_keep: int = None, normalize: str = "none", plan=None):
        """A valid TSV file -> nDCG@k of the merged scores against the answer key (``pipeline.evaluate_tsv_native``, which see, for the ensemble):
        the pass of ``score_tsv_native`` with the merged scores left on the device, the zk members' label feed from the answer key
        (``labels="answer"``) or all ones (``labels="ones"``, today's feed), the metric on the GPU (``metric="device"``) or by
        ``ndcg.ndcg_from_arrays`` on the fp64 copy of the scores (``metric="host"``) -- the same float.  ``cascade_keep``: the cascade form of
        the fused call (``_tsv_pass``); ``info`` also receives ``cascade_kept`` / ``cascade_pairs`` / ``batch_offsets``.
        ``normalize`` (one of ``ensemble.NORMALIZE``) other than ``"none"``: the pass leaves the four MEMBER scores on the device, they are
        normalised per query over the whole file and merged in double with the scorer's weights (``_normalized_merge``) -- the merge
        ``fit_joint_tsv_native(normalize=)`` graded, not the fused call's fp32 merge --, and the metric runs on that score; ``scores_out`` then
        receives ``members`` too.  Not together with ``cascade_keep`` (``ValueError``).  ``plan``: the plan form of the fused call (``_tsv_pass``); ``info``
        also receives ``plan_scored`` / ``batch_offsets``; not together with ``cascade_keep`` or a normalisation (``ValueError``)."""
        self._check_normalize(normalize, cascade_keep)
        plan = self._check_plan(plan, cascade_keep, normalize)
        if normalize != "none":
            _check_eval_args(metric, labels)
            qid, pid, mem, _, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out)
            score = self._normalized_merge(qid, mem, normalize, info)
            if scores_out is not None:
                scores_out["score"] = score
            return _metric(qid, pid, score, rank_label, k, metric, False, info)
        qid, pid, score, rank_label = self._merged_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out,
                                                        metric, cascade_keep, info, plan)
        return _metric(qid, pid, score, rank_label, k, metric, False, info)

    def fit_weights_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, grid=None, k: int = 5, labels: str = "answer",
                               batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", info: dict = None, scores_out: dict = None,
                               normalize: str = "none"):
        """A valid TSV file -> the merge weights that maximise nDCG@k against the answer key: ONE pass of ``evaluate_tsv_native`` with the four member
        scores left on the device, then ``ensemble.fit_weights`` over ``grid`` (default ``ensemble.weight_grid(4, 20)``, 1 771 vectors) in one
        library call (``mms_ndcg_weight_sweep``).  -> (weights tuple, value, index, values numpy [W]), the tuple of ``fit_weights``.
        The scorer's own weights are NOT changed: call ``set_weights(best)`` before the testB pass.  ``labels``: the zk members' label feed, as
        in ``evaluate_tsv_native``.  ``scores_out`` (a dict) receives ``query_id`` / ``product_id`` (numpy) and ``members`` (device fp32 [4, n]).
        The value of a weight vector is that of main.py's DOUBLE merge of the fp32 member scores; ``evaluate_tsv_native`` ranks the fp32 merge
        of the fused call, which can differ on a near tie.  ``normalize``: ``ensemble.fit_weights``'s keyword (the members of the whole file are
        normalised per query in front of the sweep)."""
        from . import ensemble
        self._check_normalize(normalize)
        qid, pid, mem, _, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out)
        return ensemble.fit_weights(qid, pid, mem, rank_label, grid, k, info=info, normalize=normalize)

    def fit_filter_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, filters=None, k: int = 5, labels: str = "answer",
                              batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", info: dict = None, scores_out: dict = None):
        """A valid TSV file -> the uniqueness filter ``(gap, tie)`` that maximises the nDCG@k of the SUBMISSION rows against the answer key: ONE pass
        as ``evaluate_tsv_native`` (merged scores left on the device, the zk members' label feed as ``labels`` says), then ``ensemble.fit_filter`` over
        ``filters`` (default ``ensemble.filter_grid()``, 102 rows) on the fp64 copy of the merged scores in one library call (``mms_filter_sweep``).
        -> ((gap, tie), value, index, values numpy [G]), the tuple of ``fit_filter``; pass the winner to ``submission_tsv_native(gap=, tie=)``.
        ``scores_out`` (a dict) receives ``query_id`` / ``product_id`` (numpy) and ``score`` (device fp64)."""
        from . import ensemble
        qid, pid, score, rank_label = self._merged_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out)
        return ensemble.fit_filter(qid, pid, score, rank_label, filters, k, info=info)

    def fit_joint_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, grid=None, filters=None, k: int = 5, labels: str = "answer",
                             batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", info: dict = None, scores_out: dict = None,
                             normalize: str = "none"):
        """A valid TSV file -> the merge weights AND the uniqueness filter ``(gap, tie)`` that TOGETHER maximise the nDCG@k of the SUBMISSION rows
        against the answer key: ONE pass as ``fit_weights_tsv_native`` (the four member scores left on the device, the zk members' label feed as
        ``labels`` says), then ``ensemble.fit_joint`` over ``grid`` x ``filters`` (defaults ``ensemble.weight_grid(4, 20)`` x
        ``ensemble.filter_grid()``: 1 771 x 102 pairs) in one library call (``mms_joint_sweep``).
        -> (weights tuple, (gap, tie), value, (iw, ig), values numpy [W, G]), the tuple of ``fit_joint``; pass the winner to ``set_weights`` and to
        ``submission_tsv_native(gap=, tie=)``.  The scorer's own weights are NOT changed.  ``scores_out`` (a dict) receives ``query_id`` /
        ``product_id`` (numpy) and ``members`` (device fp32 [4, n]).  The value is that of main.py's DOUBLE merge of the fp32 member scores; the
        fused call ranks the fp32 merge, which can differ on a near tie -- unless both sides normalise: with ``normalize`` other than ``"none"``
        (``ensemble.fit_joint``'s keyword) the winner goes to ``set_weights`` and ``submission_tsv_native(normalize=, gap=, tie=)``, which ranks
        exactly the merge graded here."""
        from . import ensemble
        self._check_normalize(normalize)
        qid, pid, mem, _, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out)
        return ensemble.fit_joint(qid, pid, mem, rank_label, grid, filters, k, info=info, normalize=normalize)

    def fit_joint_resampled_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, grid=None, filters=None, k: int = 5, labels: str = "answer",
                                       batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", info: dict = None, scores_out: dict = None,
                                       normalize: str = "none", **resample):
        """``fit_joint_tsv_native`` AND the held-out estimate of its winner: ONE pass as there, then ``ensemble.fit_joint_resampled`` on the member
        scores left on the device (``mms_joint_sweep_codes`` + ``mms_resample_select``, one synchronising read).  ``resample``: its keywords
        (``scheme``, ``folds``, ``repeats``, ``replicates``, ``seed``, ``counts``, ``probes``, ``code_budget``).  -> the dict of
        ``fit_joint_resampled``: ``whole`` is the tuple of ``fit_joint_tsv_native``; ``heldout``, ``optimism`` and ``agreement`` say how far to trust
        it.  The scorer's own weights are NOT changed.  ``scores_out`` and ``normalize`` as in ``fit_joint_tsv_native``."""
        from . import ensemble
        self._check_normalize(normalize)
        qid, pid, mem, _, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode, scores_out)
        return ensemble.fit_joint_resampled(qid, pid, mem, rank_label, grid, filters, k, info=info, normalize=normalize, **resample)

    def cascade_curve_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, keeps, gap: float = None, tie: float = None, k: int = 5,
                                 labels: str = "answer", batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", where: str = "device",
                                 scores_out: dict = None):
        """A valid TSV file -> what each ``keep`` of ``keeps`` would cost: ONE full pass as ``fit_joint_tsv_native`` (the four member scores left on
        the device), then ``ensemble.cascade_curve`` with the scorer's merge weights, the filter ``(gap, tie)`` (``None``: main.py's) and the pass's
        batch offsets as ``parts`` -- per ``keep`` the kept fraction, the nDCG@k of the submission rows the cascade would produce and the queries
        whose row changes.  Choose ``keep`` here, then pass it as ``cascade_keep`` to ``submission_tsv_native`` with the same ``batch_pairs``.
        ``scores_out`` receives ``query_id`` / ``product_id`` (numpy), ``members`` (device fp32 [4, n]) and ``batch_offsets``."""
        from . import ensemble
        qid, pid, mem, offsets, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode,
                                                               scores_out)
        if scores_out is not None:
            scores_out["batch_offsets"] = offsets
        gap, tie = ensemble.GAP if gap is None else gap, ensemble.TIE if tie is None else tie
        return ensemble.cascade_curve(qid, pid, mem, rank_label, keeps, self.weights, gap, tie, k, parts=offsets, where=where)

    def plan_curve_tsv_native(self, tsv_path, vocab_path, label_table, rank_label, plans, gap: float = None, tie: float = None, k: int = 5,
                              labels: str = "answer", batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host", where: str = "device",
                              scores_out: dict = None):
        """A valid TSV file -> what each plan of ``plans`` would cost: ONE full pass as ``cascade_curve_tsv_native``, then ``ensemble.plan_curve`` with the
        scorer's merge weights, the filter ``(gap, tie)`` (``None``: main.py's) and the pass's batch offsets as ``parts`` -- per plan the pairs each
        stage scores, the nDCG@k of the submission rows, the queries whose row changes and those whose top ``k`` of the merged score changes.  Choose
        a plan here, then pass it as ``plan`` to ``submission_tsv_native`` with the same ``batch_pairs``.  ``scores_out`` as there."""
        from . import ensemble
        qid, pid, mem, offsets, rank_label = self._member_pass(tsv_path, vocab_path, label_table, rank_label, labels, batch_pairs, threads, feat_decode,
                                                               scores_out)
        if scores_out is not None:
            scores_out["batch_offsets"] = offsets
        gap, tie = ensemble.GAP if gap is None else gap, ensemble.TIE if tie is None else tie
        return ensemble.plan_curve(qid, pid, mem, rank_label, plans, self.weights, gap, tie, k, parts=offsets, where=where)

    def score_tsv_native(self, tsv_path, vocab_path, label_table, batch_pairs: int = 16384, threads: int = 0, feat_decode: str = "host",
                         cascade_keep: int = None, info: dict = None, plan=None):
        """``score_lines`` on a TSV file through libmmfeat, decode and scoring overlapped: a producer thread decodes span batch i+1
        three times (zk flavour, zk with the sen2forest rewrite, lxmert flavour; ctypes releases the GIL, each featurizer rotates
        three pinned buffer sets) while the main thread copies batch i to the device and runs the ONE fused call on it.
        ``feat_decode="device"``: the zk-flavour pass gathers the features' base64 text and the GPU decodes it on the scoring stream in front of
        the fused call (``stream_scores_tsv``); same scores, a bad record raises ValueError before the pass returns.
        ``cascade_keep``: the cascade form of the fused call (``_tsv_pass``; members 0-2 of a pruned pair are zeros); ``info`` then receives
        ``cascade_kept`` / ``cascade_pairs`` / ``batch_offsets``.  ``plan``: the plan form (``_tsv_pass``; a member that was not computed for a pair is
        zero); ``info`` then receives ``plan_scored`` / ``batch_offsets``."""
        plan = self._check_plan(plan, cascade_keep)
        qid, pid, out = self._tsv_pass(tsv_path, vocab_path, label_table, batch_pairs, threads, feat_decode, members=True, cascade_keep=cascade_keep,
                                       info=info, plan=plan)
        if not out:
            return qid, pid, np.zeros(0, np.float64), tuple(np.zeros(0, np.float32) for _ in range(4))
        mem_all = torch.cat([mem for _, mem in out], 1).cpu().numpy()
        return qid, pid, torch.cat([m for m, _ in out]).double().cpu().numpy(), tuple(mem_all[k] for k in range(4))

    def submission_tsv_native(self, tsv_path, vocab_path, label_table, out_path=None, batch_pairs: int = 16384, threads: int = 0,
                              feat_decode: str = "host", rank: str = "device", gap: float = None, tie: float = None, cascade_keep: int = None,
                              info: dict = None, normalize: str = "none", plan=None):
        """TSV file -> submission rows (``{query: [p1..p5]}``, optionally written to ``out_path``): the pass of ``score_tsv_native`` with the merged
        scores left on the device -- no member scores, no score read-back --, the ids uploaded once, and the uniqueness filter + top-5 on the GPU
        (``ensemble.submission_rows_device``; ``rank="host"``: ``ensemble.submission_rows`` on the fp64 copy of the scores, what a caller of
        ``score_tsv_native`` does).  Same rows either way.  ``gap`` / ``tie``: the filter's constants (``None``: ``ensemble.GAP`` / ``ensemble.TIE``,
        main.py's), e.g. the winner of ``fit_filter_tsv_native``; both rank forms take them.  ``cascade_keep``: the cascade form of the fused call
        (``_tsv_pass``) with the ``keep`` chosen on valid (``cascade_curve_tsv_native``); ``info`` then receives ``cascade_kept`` /
        ``cascade_pairs`` / ``batch_offsets``.  ``normalize`` (one of ``ensemble.NORMALIZE``) other than ``"none"``: the pass's four member scores are
        normalised per query over the WHOLE file and merged in double with the scorer's weights on the device (``_normalized_merge``), and both rank
        forms run on that score: with the winner of ``fit_joint_tsv_native(normalize=)`` in ``set_weights`` / ``gap`` / ``tie`` the rows are those
        the fit graded.  Not together with ``cascade_keep`` (``ValueError``).  ``plan``: the plan form of the fused call (``_tsv_pass``) with the plan chosen
        on valid (``plan_curve_tsv_native``); ``info`` then receives ``plan_scored`` / ``batch_offsets``; not together with ``cascade_keep`` or a
        normalisation (``ValueError``)."""
        from . import ensemble
        self._check_normalize(normalize, cascade_keep)
        plan = self._check_plan(plan, cascade_keep, normalize)
        if feat_decode not in ("host", "device"):
            raise ValueError("feat_decode must be 'host' or 'device', not %r" % (feat_decode,))
        if rank not in ("host", "device"):
            raise ValueError("rank must be 'host' or 'device', not %r" % (rank,))
        gap, tie = ensemble.GAP if gap is None else gap, ensemble.TIE if tie is None else tie
        qid, pid, out = self._tsv_pass(tsv_path, vocab_path, label_table, batch_pairs, threads, feat_decode, members=True, cascade_keep=cascade_keep,
                                       info=info, plan=plan)
        if not out:
            rows = ensemble.submission_rows(qid, pid, np.zeros(0, np.float64), gap, tie)
        else:
            if normalize != "none":
                score = self._normalized_merge(qid, torch.cat([mem for _, mem in out], 1), normalize, info)
            else:
                score = torch.cat([m for m, _ in out]).double()
            rows = ensemble.submission_rows_device(qid, pid, score, gap, tie) if rank == "device" else ensemble.submission_rows(qid, pid, score.cpu().numpy(), gap, tie)
        if out_path is not None:
            ensemble.write_submission(out_path, rows)
        return rows
