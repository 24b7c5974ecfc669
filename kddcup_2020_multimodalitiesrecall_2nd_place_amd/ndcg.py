"""nDCG@k metric of the reference (three identical copies in the reference:
code/imagebert_lds/src/evaluation.py:4-38, code/imagebert_zk/evaluate_function.py:5-45, code/lxmert/src/utils.py:159-171).

DCG variant used there: ``r[0] + sum_{i>=1} r[i] / log2(i + 2)``; ideal vector = ones(len(ground truth));
per-query gain is 1 when the ranked product is in the query's answer set; mean over the ANSWER KEY's queries.
"""
from __future__ import annotations

import numpy as np


def dcg_at_k(r, k):
    r = np.asarray(r, dtype=float)[:k]
    if r.size:
        return float(r[0] + np.sum(r[1:] / np.log2(np.arange(3, r.size + 2))))
    return 0.0


def get_ndcg(r, ref, k):
    dcg_max = dcg_at_k(ref, k)
    if not dcg_max:
        return 0.0
    return dcg_at_k(r, k) / dcg_max


def evaluate_ndcg(rank_score_pred: dict, rank_label: dict, k: int = 5) -> float:
    """rank_score_pred: {query_id(str): [(product_id(str), score), ...]}; rank_label: {query_id: [product ids]}."""
    total = 0.0
    for q, truth in rank_label.items():
        rlist = sorted(rank_score_pred[str(q)], key=lambda x: x[1], reverse=True)  # stable, like list.sort
        gt = {str(p) for p in truth}
        pred_vec = [1.0 if str(p) in gt else 0.0 for p, _ in rlist]
        total += get_ndcg(pred_vec, [1.0] * len(gt), k)
    return total / len(rank_label)


def ndcg_from_arrays(query_id, product_id, score, rank_label: dict, k: int = 5) -> float:
    pred: dict = {}
    for q, p, s in zip(query_id, product_id, score):
        pred.setdefault(str(int(q)), []).append((str(int(p)), float(s)))
    return evaluate_ndcg(pred, rank_label, k)


# ---- integer form: per key query a CODE, the metric a function of the codes (what mms_ndcg_at_k computes on the device, csrc/ndcg.hip) ----
# code = mask | ideal << 8: bit j of mask is set when the j-th ranked row of the query is relevant (j < k), ideal = min(len(set(truth)), k);
# -1 for a key query without rows.  hist[ideal << k | mask] counts the key queries per code.
FLAG_MISSING_QUERY, FLAG_NON_FINITE, FLAG_REPEATED_KEY, FLAG_RESERVED_ID = 1, 2, 4, 8      # status[2] of mms_ndcg_at_k (include/mmscore.h)
MAX_K = 8                                                                                  # MMS_NDCG_MAX_K


def _key_lists(rank_label: dict):
    """-> (key query ids, truth lists of ints) in the key's own order."""
    return [int(q) for q in rank_label], [[int(p) for p in truth] for truth in rank_label.values()]


def ndcg_codes(query_id, product_id, score, rank_label: dict, k: int = 5, allow_missing: bool = False, return_topk: bool = False):
    """The numpy host form of the device codes: per key query a stable argsort on ``-float64(score)`` of its rows (rows in any order,
    interleaved with other queries) and ``set(truth)``.  -> int32 [len(rank_label)] in key order (and, with ``return_topk``, the ranked
    product ids int64 [len, k], -1 past a query's rows).  A key query without rows raises ``KeyError`` like ``ndcg_from_arrays``
    unless ``allow_missing`` (its code is -1 then)."""
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be in 1..%d" % MAX_K)
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    p = np.asarray(product_id).astype(np.int64).reshape(-1)
    s = np.asarray(score).astype(np.float64).reshape(-1)
    keys, truths = _key_lists(rank_label)
    by_q = np.argsort(q, kind="stable")                  # rows of a query stay in row order
    qs = q[by_q]
    codes = np.empty(len(keys), np.int32)
    topk = np.full((len(keys), k), -1, np.int64)
    for i, (kq, truth) in enumerate(zip(keys, truths)):
        rows = by_q[np.searchsorted(qs, kq, "left"):np.searchsorted(qs, kq, "right")]
        if rows.size == 0:
            if not allow_missing:
                raise KeyError(str(kq))
            codes[i] = -1
            continue
        top = rows[np.argsort(-s[rows], kind="stable")[:k]]          # -0.0 and +0.0 compare equal: a tie, kept in row order
        gt = set(truth)
        mask = sum(1 << j for j, r in enumerate(top) if int(p[r]) in gt)
        codes[i] = mask | min(len(gt), k) << 8
        topk[i, :top.size] = p[top]
    return (codes, topk) if return_topk else codes


def _code_value(code: int, k: int) -> float:
    """nDCG@k of one key query from its code -- ``get_ndcg`` on the mask's bits: the arithmetic lives in one place."""
    return get_ndcg([float(code >> j & 1) for j in range(k)], [1.0] * (code >> 8), k)


def ndcg_from_codes(codes, k: int = 5) -> float:
    """Sum of the per-query values in key order, divided by the key length: the sum ``evaluate_ndcg`` makes, term for term (bit-identical).
    Codes of -1 (key queries without rows, ``allow_missing``) add nothing."""
    total, memo = 0.0, {}
    codes = np.asarray(codes).reshape(-1).tolist()
    for c in codes:
        if c < 0:
            continue
        if c not in memo:
            memo[c] = _code_value(c, k)
        total += memo[c]
    return total / len(codes)


def hist_from_codes(codes, k: int = 5):
    """The device histogram of a code array: int64 [(k + 1) << k], bin ``ideal << k | mask``."""
    c = np.asarray(codes).reshape(-1).astype(np.int64)
    c = c[c >= 0]
    return np.bincount((c >> 8) << k | (c & 0xFF), minlength=(k + 1) << k).astype(np.int64)


def ndcg_from_hist(hist, k: int, n_queries: int) -> float:
    """sum(hist[bin] * value(bin)) / n_queries over the non-empty bins in bin order: the terms of ``ndcg_from_codes`` summed per bin, so the two
    differ by summation order only.  Histograms add (query shards: ``sharding.reduce_ndcg``); ``n_queries`` is the whole key's length."""
    h = np.asarray(hist).reshape(-1)
    if h.shape[0] != (k + 1) << k:
        raise ValueError("a k = %d histogram has %d bins, not %d" % (k, (k + 1) << k, h.shape[0]))
    total = 0.0
    for b in np.flatnonzero(h).tolist():
        total += int(h[b]) * _code_value((b >> k) << 8 | (b & ((1 << k) - 1)), k)
    return total / n_queries


class AnswerKey:
    """An answer key on the device in the CSR form of include/mmscore.h: ``key_query`` [Qa], ``key_off`` [Qa + 1], ``key_product`` [Tk] (int64
    device tensors).  Built once from the ``{query: [products]}`` dict and passed wherever ``rank_label`` is taken, it saves the upload per call."""

    def __init__(self, rank_label: dict, device=None):
        import torch
        self.rank_label = rank_label
        keys, truths = _key_lists(rank_label)
        off = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([len(t) for t in truths], out=off[1:])
        prod = np.array([p for t in truths for p in t], np.int64)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        up = lambda a: torch.from_numpy(a).to(self.device, non_blocking=True)
        self.key_query, self.key_off, self.key_product = up(np.array(keys, np.int64)), up(off), up(prod)
        self.n_queries, self.n_products = len(keys), int(prod.shape[0])


def _label_dict(rank_label):
    """The ``{query: [products]}`` dict of a ``rank_label`` argument: the dict itself, or the one an ``AnswerKey`` was built from."""
    return rank_label.rank_label if isinstance(rank_label, AnswerKey) else rank_label


def _to_np(x):
    """A tensor (wherever it lives) or an array-like as a numpy array: what the host forms take."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _key_on(rank_label, dev, what=None):
    """The answer key on ``dev``; with ``what`` (the caller's name) an empty key is an error."""
    if isinstance(rank_label, AnswerKey):
        if rank_label.device != dev:
            raise ValueError("the AnswerKey lives on %s, the rows on %s" % (rank_label.device, dev))
        key = rank_label
    else:
        key = AnswerKey(rank_label, dev)
    if what is not None and key.n_queries == 0:
        raise ValueError("%s: empty answer key" % what)
    return key


def _rows_on_device(arrays, dtypes, what):
    """The row arrays as flat contiguous device tensors (used in place when they already are), the device they live on."""
    import torch
    dev = next((t.device for t in arrays if torch.is_tensor(t) and t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    out = []
    for x, dt in zip(arrays, dtypes):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        if t.dtype not in dt:
            t = t.to(dt[0])
        out.append(t.to(dev, non_blocking=True).contiguous().reshape(-1))
    if len({t.shape[0] for t in out}) != 1:
        raise ValueError("%s: row arrays of %s entries" % (what, " / ".join(str(t.shape[0]) for t in out)))
    return out, dev


def _on_device(x, dev, dtype):
    """``x`` as a contiguous tensor of ``dtype`` on ``dev``: used in place when it already is one, a host array is copied up once."""
    import torch
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dtype, non_blocking=True).contiguous()


def _workspace(ws_bytes, n, key, dev, what):
    """The workspace of ``ws_bytes`` (what a ``mms_*_workspace_bytes`` returned: negative for a table beyond the limits) -> (tensor, ws_bytes)."""
    import torch
    if ws_bytes < 0:
        raise ValueError("%s: %d rows, %d key queries, %d key products: the device path takes at most 2^22 rows / key products and 2^20 key queries"
                         % (what, n, key.n_queries, key.n_products))
    return torch.empty((ws_bytes,), dtype=torch.uint8, device=dev), ws_bytes      # (the caching allocator returns 512-byte aligned blocks)


_ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
_key_args = lambda key: (_ptr(key.key_query), _ptr(key.key_off), _ptr(key.key_product), key.n_queries, key.n_products)      # the CSR answer key, as every entry point takes it


def _score_ptrs(s, status):
    """-> (score_f32, score_f64) of an entry point that takes exactly one of the two: a non-NULL pointer even for n == 0 (never dereferenced then)."""
    import torch
    sp = _ptr(s) or status.data_ptr()
    return (sp, None) if s.dtype == torch.float32 else (None, sp)


def _check_rc(l, rc, name):
    if rc != 0:
        from . import lib as _lib
        raise _lib.MmsError("%s failed (%d): %s" % (name, rc, l.mms_global_error().decode()))


class _DeviceCall:
    """What every wrapper of a handle-free entry point needs around its one call: the library ``l`` (for the ``*_workspace_bytes`` query too), a
    ``status`` block int32 [4] on ``dev`` (the caller's, or a fresh one the call writes), the current stream and the check of the return code.
    Where the status pointer goes among the arguments is the entry point's business."""

    def __init__(self, dev, status=None):
        import torch

        from . import lib as _lib
        self.l, self.dev = _lib.load(), dev
        self.status = torch.empty((4,), dtype=torch.int32, device=dev) if status is None else status

    def __call__(self, name, *args):
        """``l.<name>(*args, stream)``: ``args`` is everything in front of the stream, which every entry point takes last.  Only enqueues."""
        import torch
        _check_rc(self.l, getattr(self.l, name)(*args, torch.cuda.current_stream(self.dev).cuda_stream), name)


def relevance_device(query_id, product_id, rank_label, status_out: list = None):
    """The ground-truth labels of the rows on the GPU (``mms_key_relevance``): int64 device tensor [n], 1 where the row's product is in its query's
    truth list.  ``rank_label``: the ``{query: [products]}`` dict or an ``AnswerKey``.  Only enqueues on the current stream; ``status_out`` (a list)
    receives the device status tensor [4] (rows of key queries in [1], flags in [2]) for a caller that wants to read it later."""
    import torch
    (q, p), dev = _rows_on_device((query_id, product_id), ((torch.int64,), (torch.int64,)), "relevance_device")
    key = _key_on(rank_label, dev)
    n = q.shape[0]
    call = _DeviceCall(dev)
    ws, ws_bytes = _workspace(call.l.mms_ndcg_workspace_bytes(n, key.n_queries, key.n_products), n, key, dev, "relevance_device")
    labels = torch.empty((n,), dtype=torch.int64, device=dev)
    call("mms_key_relevance", _ptr(q), _ptr(p), n, *_key_args(key), ws.data_ptr(), ws_bytes, _ptr(labels), call.status.data_ptr())
    if status_out is not None:
        status_out.append(call.status)
    return labels


def ndcg_codes_device(query_id, product_id, score, rank_label, k: int = 5, allow_missing: bool = False, want_topk: bool = False):
    """``mms_ndcg_at_k`` on device tensors (used in place when int64 / fp32 or fp64 and contiguous) or host arrays (copied up once).
    -> (codes int32 [Qa], topk int64 [Qa, k] or None, hist int64 [(k + 1) << k], status int32 [4]), device tensors.  Only enqueues on the
    current stream: nothing is read back, nothing waits."""
    import torch
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be in 1..%d" % MAX_K)
    (q, p, s), dev = _rows_on_device((query_id, product_id, score), ((torch.int64,), (torch.int64,), (torch.float64, torch.float32)), "ndcg_device")
    key = _key_on(rank_label, dev)
    n = s.shape[0]
    call = _DeviceCall(dev)
    ws, ws_bytes = _workspace(call.l.mms_ndcg_workspace_bytes(n, key.n_queries, key.n_products), n, key, dev, "ndcg_device")
    codes = torch.empty((key.n_queries,), dtype=torch.int32, device=dev)
    topk = torch.empty((key.n_queries, k), dtype=torch.int64, device=dev) if want_topk else None
    hist = torch.empty(((k + 1) << k,), dtype=torch.int64, device=dev)
    call("mms_ndcg_at_k", _ptr(q), _ptr(p), *_score_ptrs(s, call.status), n, *_key_args(key), k, int(bool(allow_missing)), ws.data_ptr(), ws_bytes,
         _ptr(codes), _ptr(topk), hist.data_ptr(), call.status.data_ptr())
    return codes, topk, hist, call.status


def ndcg_device(query_id, product_id, score, rank_label, k: int = 5, info: dict = None, allow_missing: bool = False, return_hist: bool = False):
    """``ndcg_from_arrays`` with the ranking on the GPU (``mms_ndcg_at_k``): the same float, bit for bit.  The rows may be device tensors (the
    scores stay where the scorer left them) or host arrays; ``rank_label`` the ``{query: [products]}`` dict or an ``AnswerKey``.  ONE small host
    read carries the status and the codes (4 bytes per key query) -- or, with ``return_hist``, the status and the histogram, and the result is
    ``(hist int64 numpy [(k + 1) << k], key queries evaluated)`` for ``sharding.reduce_ndcg`` / ``ndcg_from_hist``.
    ``allow_missing``: key queries without rows add nothing (a rank's shard); without it they raise ``KeyError`` like the host form.
    What the device does not do -- a non-finite score, a repeated key query, an id equal to the reserved -1 -- it detects: the value then
    comes from the host form on the host arrays.  ``info`` (a dict) receives ``{"path": "device" | "host", "flags": int}``."""
    import torch
    label_dict = _label_dict(rank_label)
    if len(label_dict) == 0:
        return ndcg_from_arrays([], [], [], label_dict, k)                   # the host form's own error for an empty key
    codes, _, hist, status = ndcg_codes_device(query_id, product_id, score, rank_label, k, allow_missing)
    out = hist if return_hist else codes.to(torch.int64)
    host = torch.cat([status.to(torch.int64), out]).cpu().numpy()            # the one synchronising read
    flags, body = int(host[2]), host[4:]
    if info is not None:
        info.update(path="host" if flags & ~FLAG_MISSING_QUERY else "device", flags=flags)
    if flags & ~FLAG_MISSING_QUERY:
        qh, ph, sh = _to_np(query_id), _to_np(product_id), _to_np(score)
        if return_hist:
            c = ndcg_codes(qh, ph, sh, label_dict, k, allow_missing)
            return hist_from_codes(c, k), int((c >= 0).sum())
        if allow_missing:
            return ndcg_from_codes(ndcg_codes(qh, ph, sh, label_dict, k, True), k)
        return ndcg_from_arrays(qh, ph, sh, label_dict, k)
    if flags & FLAG_MISSING_QUERY:                                           # only without allow_missing
        if return_hist:
            raise KeyError("%d key queries have no rows" % int(host[3]))
        raise KeyError(str(_key_lists(label_dict)[0][int(np.flatnonzero(body < 0)[0])]))
    if return_hist:
        return body.copy(), int(host[0])
    return ndcg_from_codes(body, k)


# ---- weight sweep: the histogram and the value of EVERY weight vector of a grid (mms_ndcg_weight_sweep, csrc/ndcg_sweep.hip) ----
MAX_MEMBERS, MAX_WEIGHTS = 8, 1 << 20                                                      # MMS_SWEEP_MAX_MEMBERS, MMS_SWEEP_MAX_WEIGHTS
_BIN_TABLES: dict = {}


def _bin_table(k, dev):
    """``bin_values(k)`` on the device ``dev``."""
    import torch
    if (k, dev) not in _BIN_TABLES:
        _BIN_TABLES[k, dev] = torch.from_numpy(bin_values(k).copy()).to(dev)
    return _BIN_TABLES[k, dev]


def bin_values(k: int = 5):
    """float64 [(k + 1) << k]: the nDCG@k of a key query per histogram bin (``_code_value`` of the bin's code) -- the table ``mms_ndcg_weight_sweep``
    takes as ``bin_value``.  Read-only, built once per k (its device copies are kept beside it, per (k, device))."""
    if k not in _BIN_TABLES:
        t = np.array([_code_value((b >> k) << 8 | (b & ((1 << k) - 1)), k) for b in range((k + 1) << k)], np.float64)
        t.setflags(write=False)
        _BIN_TABLES[k] = t
    return _BIN_TABLES[k]


def merge_members(members, w):
    """``(...((w[0] * s0) + w[1] * s1) + ...) + w[M - 1] * s_{M-1}`` in float64, each product and each sum a numpy operation of its own (rounded on
    its own, left to right): Python's evaluation of code/main.py:59 -- the arithmetic contract of the sweep.  ``members``: float32 [M, n]."""
    acc = np.float64(w[0]) * members[0].astype(np.float64)
    for m in range(1, len(members)):
        prod = np.float64(w[m]) * members[m].astype(np.float64)
        acc = acc + prod
    return acc


def _sweep_args(members, weights, k):
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be in 1..%d" % MAX_K)
    M = int(members.shape[0]) if members.ndim == 2 else 0
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError("members must be [1..%d, n], not %s" % (MAX_MEMBERS, tuple(members.shape)))
    if weights.ndim != 2 or weights.shape[1] != M:
        raise ValueError("weights must be [W, %d], not %s" % (M, tuple(weights.shape)))
    if weights.shape[0] > MAX_WEIGHTS:
        raise ValueError("at most %d weight vectors per call" % MAX_WEIGHTS)


def ndcg_sweep_host(query_id, product_id, members, weights, rank_label: dict, k: int = 5, allow_missing: bool = False):
    """The host form of the sweep and the reference of the device form: per weight vector ``hist_from_codes(ndcg_codes(q, p, merge_members(members,
    w), ...))`` and ``ndcg_from_hist`` of it over the whole key.  ``members``: float32 [M, n] (member-major, the layout ``mms_score_ensemble`` writes),
    ``weights``: float64 [W, M].  -> (values float64 [W], hist int64 [W, (k + 1) << k]), numpy."""
    mem = _member_array(members)
    wts = np.asarray(weights, np.float64)
    _sweep_args(mem, wts, k)
    label_dict = _label_dict(rank_label)
    mem = mem.reshape(mem.shape[0], -1)
    values = np.empty(wts.shape[0], np.float64)
    hist = np.empty((wts.shape[0], (k + 1) << k), np.int64)
    for v in range(wts.shape[0]):
        hist[v] = hist_from_codes(ndcg_codes(query_id, product_id, merge_members(mem, wts[v]), label_dict, k, allow_missing), k)
        values[v] = ndcg_from_hist(hist[v], k, len(label_dict))
    return values, hist


def ndcg_sweep_device(query_id, product_id, members, weights, rank_label, k: int = 5, allow_missing: bool = False):
    """``mms_ndcg_weight_sweep``: the sweep on the GPU in one call.  ``members`` [M, n] fp32 and ``weights`` [W, M] fp64 are used in place when they
    are contiguous device tensors of that dtype (the member scores stay where ``mms_score_ensemble`` left them), host arrays are copied up once;
    ``rank_label``: the ``{query: [products]}`` dict or an ``AnswerKey``.  -> (values float64 [W], hist int64 [W, (k + 1) << k], status int32 [4]),
    device tensors, bit-equal to ``ndcg_sweep_host`` while the flag word ``status[2]`` is zero (or "missing" alone with ``allow_missing``).
    Only enqueues on the current stream: nothing is read back, nothing waits."""
    import torch
    (q, p), dev = _rows_on_device((query_id, product_id), ((torch.int64,), (torch.int64,)), "ndcg_sweep_device")
    mem, wts = _members_on(members, dev), _on_device(weights, dev, torch.float64)
    _sweep_args(mem, wts, k)
    n, M, W = q.shape[0], mem.shape[0], wts.shape[0]
    if mem.shape[1] != n:
        raise ValueError("ndcg_sweep_device: %d rows, member scores of %d" % (n, mem.shape[1]))
    key = _key_on(rank_label, dev, "ndcg_sweep_device")
    call = _DeviceCall(dev)
    ws, ws_bytes = _workspace(call.l.mms_ndcg_sweep_workspace_bytes(n, key.n_queries, key.n_products, M), n, key, dev, "ndcg_sweep_device")
    hist = torch.empty((W, (k + 1) << k), dtype=torch.int64, device=dev)
    values = torch.empty((W,), dtype=torch.float64, device=dev)
    call("mms_ndcg_weight_sweep", _ptr(q), _ptr(p), _ptr(mem), M, n, *_key_args(key), _ptr(wts), W, k, int(bool(allow_missing)),
         _bin_table(k, dev).data_ptr(), key.n_queries, ws.data_ptr(), ws_bytes, _ptr(hist), _ptr(values), call.status.data_ptr())
    return values, hist, call.status


# ---- filter sweep: nDCG@k of the SUBMISSION rows for every (gap, tie) pair of a grid (mms_filter_sweep, csrc/filter_sweep.hip) ----
# per key query a code: -1 no rows in the table, -2 rows but no output row (no survivor: main.py:91-104 never writes the query, it scores 0),
# otherwise mask | ideal << 8 over the products of its output row.
FLAG_REPEATED_PAIR = 16                                                                    # status[2] bit 4 of mms_filter_sweep
MAX_FILTERS, FILTER_MAX_K = 1 << 16, 5                                                     # MMS_FILTER_MAX, MMS_FILTER_MAX_K
CODE_MISSING, CODE_DROPPED = -1, -2


def codes_of_rows(rows: dict, present, rank_label: dict, k: int, allow_missing: bool):
    """The codes of submission rows ``{str(query): [str(product), ..]}`` against the key; ``present``: the set of query ids (int) that have table rows."""
    keys, truths = _key_lists(rank_label)
    codes = np.empty(len(keys), np.int32)
    for i, (kq, truth) in enumerate(zip(keys, truths)):
        if kq not in present:
            if not allow_missing:
                raise KeyError(str(kq))
            codes[i] = CODE_MISSING
            continue
        row = rows.get(str(kq))
        if row is None:
            codes[i] = CODE_DROPPED
            continue
        gt = set(truth)
        mask = sum(1 << j for j, pp in enumerate(row[:k]) if int(pp) in gt)
        codes[i] = mask | min(len(gt), k) << 8
    return codes


def _filter_k(k):
    if not 1 <= k <= FILTER_MAX_K:
        raise ValueError("k must be in 1..%d: a submission row holds five products" % FILTER_MAX_K)


def submission_codes(query_id, product_id, score, rank_label: dict, gap, tie, k: int = 5, allow_missing: bool = False):
    """Grades what is actually submitted: ``ensemble.submission_rows(query_id, product_id, score, gap, tie)`` -- the uniqueness filter, the
    1..4-survivor fallback, the dropped no-survivor queries -- against the answer key.  -> int32 [len(rank_label)] in key order: -1 for a key query
    without table rows (``KeyError`` unless ``allow_missing``), -2 for one with rows but no output row, otherwise ``mask | ideal << 8`` with bit j of
    ``mask`` set when the j-th product of the output row is in ``set(truth)`` (j < min(k, products written)), ``ideal = min(len(set(truth)), k)``."""
    from . import ensemble
    _filter_k(k)
    label_dict = _label_dict(rank_label)
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    rows = ensemble.submission_rows(q, np.asarray(product_id).reshape(-1), np.asarray(score).reshape(-1), gap, tie)
    return codes_of_rows(rows, set(np.unique(q).tolist()), label_dict, k, allow_missing)


def _filter_array(filters):
    f = np.ascontiguousarray(filters, np.float64)
    if f.ndim != 2 or f.shape[1] != 2:
        raise ValueError("filters must be [G, 2] rows of (gap, tie), not %s" % (tuple(f.shape),))
    if f.shape[0] > MAX_FILTERS:
        raise ValueError("at most %d filters per call" % MAX_FILTERS)
    return f


def _filters_on(filters, dev):
    """The filter grid as a float64 [G, 2] tensor on ``dev`` (a host array through ``_filter_array``'s checks first)."""
    import torch
    flt = _on_device(filters if torch.is_tensor(filters) else _filter_array(filters), dev, torch.float64)
    if flt.ndim != 2 or flt.shape[1] != 2 or flt.shape[0] > MAX_FILTERS:
        raise ValueError("filters must be [G <= %d, 2] rows of (gap, tie), not %s" % (MAX_FILTERS, tuple(flt.shape)))
    return flt


def filter_sweep_host(query_id, product_id, score, filters, rank_label: dict, k: int = 5, allow_missing: bool = False):
    """The host form of the filter sweep and the reference of the device form: per row ``(gap, tie)`` of ``filters`` (float64 [G, 2])
    ``submission_codes``, the histogram of the codes >= 0 and ``ndcg_from_hist`` of it over the WHOLE key -- a dropped or missing query costs its
    share, as a grader of the submission file charges it.  -> (values float64 [G], hist int64 [G, (k + 1) << k], codes int32 [G, Qa]), numpy."""
    f = _filter_array(filters)
    _filter_k(k)
    label_dict = _label_dict(rank_label)
    G, Qa = f.shape[0], len(label_dict)
    values = np.empty(G, np.float64)
    hist = np.empty((G, (k + 1) << k), np.int64)
    codes = np.empty((G, Qa), np.int32)
    for g in range(G):
        codes[g] = submission_codes(query_id, product_id, score, label_dict, f[g, 0], f[g, 1], k, allow_missing)
        hist[g] = hist_from_codes(codes[g], k)
        values[g] = ndcg_from_hist(hist[g], k, Qa)
    return values, hist, codes


def filter_sweep_device(query_id, product_id, score, filters, rank_label, k: int = 5, allow_missing: bool = False, want_codes: bool = False):
    """``mms_filter_sweep``: the filter sweep on the GPU in one call.  The rows are device tensors (used in place when int64 / fp32 or fp64 and
    contiguous) or host arrays (copied up once); ``filters`` [G, 2] fp64; ``rank_label``: the ``{query: [products]}`` dict or an ``AnswerKey``.
    -> (values float64 [G], hist int64 [G, (k + 1) << k], status int32 [4][, codes int32 [G, Qa] with ``want_codes``]), device tensors, equal to
    ``filter_sweep_host`` -- integers entry for entry, values bit for bit -- while the flag word ``status[2]`` is zero.
    Only enqueues on the current stream: nothing is read back, nothing waits."""
    import torch
    _filter_k(k)
    (q, p, s), dev = _rows_on_device((query_id, product_id, score), ((torch.int64,), (torch.int64,), (torch.float64, torch.float32)), "filter_sweep_device")
    flt = _filters_on(filters, dev)
    key = _key_on(rank_label, dev, "filter_sweep_device")
    n, G = s.shape[0], flt.shape[0]
    call = _DeviceCall(dev)
    ws, ws_bytes = _workspace(call.l.mms_filter_sweep_workspace_bytes(n, key.n_queries, key.n_products), n, key, dev, "filter_sweep_device")
    hist = torch.empty((G, (k + 1) << k), dtype=torch.int64, device=dev)
    values = torch.empty((G,), dtype=torch.float64, device=dev)
    codes = torch.empty((G, key.n_queries), dtype=torch.int32, device=dev) if want_codes else None
    call("mms_filter_sweep", _ptr(q), _ptr(p), *_score_ptrs(s, call.status), n, *_key_args(key), _ptr(flt), G, k, int(bool(allow_missing)),
         _bin_table(k, dev).data_ptr(), key.n_queries, ws.data_ptr(), ws_bytes, _ptr(hist), _ptr(values), _ptr(codes), call.status.data_ptr())
    return (values, hist, call.status, codes) if want_codes else (values, hist, call.status)


# ---- joint sweep: nDCG@k of the SUBMISSION rows for every (weight vector, filter) pair (mms_joint_sweep, csrc/joint_sweep.hip) ----
MAX_JOINT_ITEMS = 1 << 22                                                                  # MMS_JOINT_MAX_ITEMS
JOINT_STATS_BYTES = 256 << 20             # joint_sweep_device's default chunk: the weight tiles whose product statistics fit in this


def _member_array(members):
    """The member scores (an array or tensor [M, n], or a list of M rows, wherever they live) as one float32 numpy array."""
    mem = np.stack([_to_np(m).reshape(-1) for m in members]) if isinstance(members, (list, tuple)) and members else _to_np(members)
    return mem.astype(np.float32) if mem.dtype != np.float32 else mem


def _members_on(members, dev):
    """The member scores as one float32 tensor on ``dev``: a list of rows is stacked, a [M, n] device tensor is used in place."""
    import torch
    if isinstance(members, (list, tuple)):
        members = torch.stack([_on_device(m, dev, torch.float32).reshape(-1) for m in members]) if members else torch.zeros((0, 0))
    return _on_device(members, dev, torch.float32)


def _joint_args(members, weights, n_filters, k):
    _filter_k(k)
    _sweep_args(members, weights, k)
    if weights.shape[0] > MAX_JOINT_ITEMS or weights.shape[0] * n_filters > MAX_JOINT_ITEMS:
        raise ValueError("at most %d (weight vector, filter) pairs per call" % MAX_JOINT_ITEMS)


def _joint_host_args(members, weights, filters, rank_label, k):
    mem, wts, f = _member_array(members), np.asarray(weights, np.float64), _filter_array(filters)
    _joint_args(mem, wts, f.shape[0], k)
    return mem.reshape(mem.shape[0], -1), wts, f, _label_dict(rank_label)


def joint_sweep_host(query_id, product_id, members, weights, filters, rank_label: dict, k: int = 5, allow_missing: bool = False):
    """The host form of the joint sweep and the reference of the device form -- by definition the loop: per weight vector ``w`` of ``weights``
    (float64 [W, M]) ``filter_sweep_host`` of ``filters`` (float64 [G, 2] rows ``(gap, tie)``) on ``merge_members(members, w)``.  It composes the two
    existing contracts (the merge of the weight sweep feeds the filter sweep unchanged) and adds no arithmetic of its own.  ``members``: float32
    [M, n], member-major.  -> (values float64 [W, G], hist int64 [W, G, (k + 1) << k]), numpy."""
    mem, wts, f, label_dict = _joint_host_args(members, weights, filters, rank_label, k)
    values = np.empty((wts.shape[0], f.shape[0]), np.float64)
    hist = np.empty((wts.shape[0], f.shape[0], (k + 1) << k), np.int64)
    for v in range(wts.shape[0]):
        values[v], hist[v], _ = filter_sweep_host(query_id, product_id, merge_members(mem, wts[v]), f, label_dict, k, allow_missing)
    return values, hist


def joint_sweep_device(query_id, product_id, members, weights, filters, rank_label, k: int = 5, allow_missing: bool = False, want_hist: bool = False,
                       chunk_tiles: int = None):
    """``mms_joint_sweep``: the joint sweep on the GPU in one call.  ``members`` [M, n] fp32, ``weights`` [W, M] fp64 and ``filters`` [G, 2] fp64 are
    used in place when they are contiguous device tensors of that dtype, host arrays are copied up once; ``rank_label``: the ``{query: [products]}``
    dict or an ``AnswerKey``.  -> (values float64 [W, G], hist int64 [W, G, (k + 1) << k] or None without ``want_hist``, status int32 [4]), device
    tensors, equal to ``joint_sweep_host`` -- integers entry for entry, values bit for bit -- while the flag word ``status[2]`` is zero (or
    "missing" alone with ``allow_missing``).  The weight vectors are swept in chunks of ``chunk_tiles`` tiles of 64 (``None``: as many as keep the
    per-vector product statistics within 256 MiB, one at least); the result does not depend on it.  Without ``want_hist`` the histograms of one
    chunk live in the workspace and the full [W, G, bins] array (about 280 MB at the default grids) is never allocated.
    Only enqueues on the current stream: nothing is read back, nothing waits."""
    return _joint_sweep_call(query_id, product_id, members, weights, filters, rank_label, k, allow_missing, want_hist, chunk_tiles, False)


def _joint_sweep_call(query_id, product_id, members, weights, filters, rank_label, k, allow_missing, want_hist, chunk_tiles, want_codes):
    """``joint_sweep_device`` (``mms_joint_sweep``) or, with ``want_codes``, ``joint_codes_device`` (``mms_joint_sweep_codes``: the codes come fourth)."""
    import torch
    (q, p), dev = _rows_on_device((query_id, product_id), ((torch.int64,), (torch.int64,)), "joint_sweep_device")
    mem, wts, flt = _members_on(members, dev), _on_device(weights, dev, torch.float64), _filters_on(filters, dev)
    _joint_args(mem, wts, flt.shape[0], k)
    n, M, W, G = q.shape[0], mem.shape[0], wts.shape[0], flt.shape[0]
    if mem.shape[1] != n:
        raise ValueError("joint_sweep_device: %d rows, member scores of %d" % (n, mem.shape[1]))
    key = _key_on(rank_label, dev, "joint_sweep_device")
    if chunk_tiles is not None and chunk_tiles < 1:
        raise ValueError("joint_sweep_device: chunk_tiles must be >= 1")
    call = _DeviceCall(dev)
    bins = (k + 1) << k
    tiles = max(1, (W + 63) // 64)
    chunk = min(tiles, max(1, JOINT_STATS_BYTES // (16 * 64 * max(n, 1))) if chunk_tiles is None else int(chunk_tiles))
    ws_bytes = call.l.mms_joint_sweep_workspace_bytes(n, key.n_queries, key.n_products, M, chunk)
    if ws_bytes >= 0 and not want_hist:
        ws_bytes += chunk * ((64 * G * bins * 8 + 255) & ~255)                 # the chunk's histograms
    ws, ws_bytes = _workspace(ws_bytes, n, key, dev, "joint_sweep_device")
    hist = torch.empty((W, G, bins), dtype=torch.int64, device=dev) if want_hist else None
    values = torch.empty((W, G), dtype=torch.float64, device=dev)
    args = (_ptr(q), _ptr(p), _ptr(mem), M, n, *_key_args(key), _ptr(wts), W, _ptr(flt), G, k, int(bool(allow_missing)), _bin_table(k, dev).data_ptr(),
            key.n_queries, ws.data_ptr(), ws_bytes, _ptr(hist), _ptr(values))
    if not want_codes:
        call("mms_joint_sweep", *args, call.status.data_ptr())
        return values, hist, call.status
    codes = torch.empty((G, key.n_queries, (W + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    call("mms_joint_sweep_codes", *args, _ptr(codes), codes.numel(), call.status.data_ptr())
    return values, hist, call.status, codes


# ---- resampling the joint fit: byte codes per (vector, filter, key query) and replicates of counts over the key (mms_joint_sweep_codes,
# mms_resample_select, csrc/resample.hip) ----
# byte code: ideal << 5 | mask for a graded query (k <= 5: mask < 32), 0xFF for code -1 (no table rows), 0xFE for code -2 (rows but no output row)
BYTE_MISSING, BYTE_DROPPED = 0xFF, 0xFE
FLAG_EMPTY_FIT = 32                                                                        # status[2] bit 5 of mms_resample_select (MMS_FLAG_EMPTY_FIT)
MAX_REPLICATES, MAX_PROBES = 1 << 16, 256                                                  # MMS_RESAMPLE_MAX_REPLICATES, MMS_RESAMPLE_MAX_PROBES
_BYTE_TABLES: dict = {}


def byte_codes(codes):
    """The int32 codes of ``submission_codes`` (``mask | ideal << 8``, -1, -2) as the bytes of ``mms_joint_sweep_codes``: uint8, same shape."""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c == CODE_MISSING, BYTE_MISSING, np.where(c == CODE_DROPPED, BYTE_DROPPED, (c >> 8) << 5 | (c & 0x1F))).astype(np.uint8)


def byte_values(k: int = 5):
    """float64 [256]: the nDCG@k of a key query per code byte (``_code_value`` of the byte's code) -- the table ``mms_resample_select`` takes as
    ``byte_value``.  0.0 for the two reserved bytes and for the bytes that cannot occur at this k.  Read-only, built once per k."""
    _filter_k(k)
    if k not in _BYTE_TABLES:
        t = np.zeros(256, np.float64)
        for ideal in range(k + 1):
            for mask in range(1 << k):
                t[ideal << 5 | mask] = _code_value(mask | ideal << 8, k)
        t.setflags(write=False)
        _BYTE_TABLES[k] = t
    return _BYTE_TABLES[k]


def _byte_table(k, dev):
    import torch
    if (k, dev) not in _BYTE_TABLES:
        _BYTE_TABLES[k, dev] = torch.from_numpy(byte_values(k).copy()).to(dev)
    return _BYTE_TABLES[k, dev]


def joint_codes_host(query_id, product_id, members, weights, filters, rank_label: dict, k: int = 5, allow_missing: bool = False):
    """The host form of the code matrix of ``mms_joint_sweep_codes`` and its reference: per weight vector ``w`` and filter ``(gap, tie)`` the bytes of
    ``submission_codes`` on ``merge_members(members, w)``.  -> uint8 numpy [W, G, Qa] (item-major: ``[v, g]`` are the codes of item ``v * G + g``)."""
    mem, wts, f, label_dict = _joint_host_args(members, weights, filters, rank_label, k)
    out = np.empty((wts.shape[0], f.shape[0], len(label_dict)), np.uint8)
    for v in range(wts.shape[0]):
        merged = merge_members(mem, wts[v])
        for g in range(f.shape[0]):
            out[v, g] = byte_codes(submission_codes(query_id, product_id, merged, label_dict, f[g, 0], f[g, 1], k, allow_missing))
    return out


def _count_arrays(count_fit, count_eval, n_key_queries):
    cf, ce = np.ascontiguousarray(count_fit), np.ascontiguousarray(count_eval)
    if cf.dtype != np.uint8 or ce.dtype != np.uint8 or cf.ndim != 2 or cf.shape != ce.shape or cf.shape[1] != n_key_queries:
        raise ValueError("count_fit / count_eval must be uint8 [R, %d], not %s %s / %s %s" % (n_key_queries, cf.dtype, cf.shape, ce.dtype, ce.shape))
    if cf.shape[0] > MAX_REPLICATES:
        raise ValueError("at most %d replicates per call" % MAX_REPLICATES)
    return cf, ce


def _probe_array(probes):
    pr = np.zeros(0, np.int64) if probes is None else np.ascontiguousarray(probes, np.int64).reshape(-1)
    if pr.shape[0] > MAX_PROBES:
        raise ValueError("at most %d probes per call" % MAX_PROBES)
    return pr


def resample_select_host(codes, count_fit, count_eval, k: int = 5, probes=None, block: int = 16):
    """The host form of ``mms_resample_select`` and its reference.  ``codes``: uint8 [W, G, Qa] (``joint_codes_host``); ``count_fit`` / ``count_eval``:
    uint8 [R, Qa]; ``probes``: items ``v * G + g``.  Per replicate r and item
    ``fit = (sum_i float64(count_fit[r, i]) * byte_values(k)[code[item, i]]) / float64(sum_i count_fit[r, i])`` -- the loop over i outermost, the
    product and the sum numpy operations of their own (rounded on their own) --, the FIRST item at the maximum, and the same sum with ``count_eval``
    on the winner and on the probes.  A fit row that sums to zero: winner -1, NaN values.  -> (best int64 [R], fit_value [R], eval_value [R],
    probe_fit [R, P], probe_eval [R, P]), numpy.  ``block``: replicates per pass (memory only: the result does not depend on it)."""
    c = np.asarray(codes)
    if c.dtype != np.uint8 or c.ndim != 3:
        raise ValueError("codes must be uint8 [W, G, Qa], not %s %s" % (c.dtype, c.shape))
    W, G, Qa = c.shape
    cf, ce = _count_arrays(count_fit, count_eval, Qa)
    pr = _probe_array(probes)
    R, P, items = cf.shape[0], pr.shape[0], W * G
    vals = byte_values(k)[c.reshape(items, Qa)]                               # [items, Qa]
    sum_f, sum_e = cf.sum(1, dtype=np.int64).astype(np.float64), ce.sum(1, dtype=np.int64).astype(np.float64)
    best = np.full(R, -1, np.int64)
    fit_value, eval_value = np.full(R, np.nan), np.full(R, np.nan)
    probe_fit, probe_eval = np.full((R, P), np.nan), np.full((R, P), np.nan)

    def sums_on(rows, count, item):                                          # the sequential sum of replicates `rows` on their items `item` [len(rows)]
        acc = np.zeros(len(rows), np.float64)
        for i in range(Qa):
            prod = count[rows, i].astype(np.float64) * vals[item, i]
            acc = acc + prod
        return acc

    with np.errstate(invalid="ignore", divide="ignore"):
        for r0 in range(0, R, block):
            rows = np.arange(r0, min(R, r0 + block))
            if items:
                acc = np.zeros((len(rows), items), np.float64)
                for i in range(Qa):
                    prod = cf[rows, i].astype(np.float64)[:, None] * vals[None, :, i]
                    acc = acc + prod
                fit = acc / sum_f[rows, None]
                ok = sum_f[rows] > 0
                b = np.argmax(np.where(ok[:, None], fit, 0.0), axis=1)      # the first item at the maximum
                best[rows[ok]] = b[ok]
                fit_value[rows[ok]] = fit[ok, b[ok]]
                eval_value[rows[ok]] = sums_on(rows[ok], ce, b[ok]) / sum_e[rows[ok]]
            for j, it in enumerate(pr.tolist()):
                if 0 <= it < items:
                    item = np.full(len(rows), it, np.int64)
                    probe_fit[rows, j] = sums_on(rows, cf, item) / sum_f[rows]
                    probe_eval[rows, j] = sums_on(rows, ce, item) / sum_e[rows]
    return best, fit_value, eval_value, probe_fit, probe_eval


def joint_codes_device(query_id, product_id, members, weights, filters, rank_label, k: int = 5, allow_missing: bool = False, want_hist: bool = False,
                       chunk_tiles: int = None):
    """``mms_joint_sweep_codes``: ``joint_sweep_device`` that keeps the per-query codes.  -> (values float64 [W, G], hist or None, status int32 [4],
    codes uint8 [G, Qa, Wp] with Wp = 64 * ceil(W / 64)), device tensors; ``codes[g, i, v]`` equals ``joint_codes_host(..)[v, g, i]`` for v < W while
    the flag word is clean, and values / hist / status are those of ``joint_sweep_device``, bit for bit.  Only enqueues on the current stream."""
    return _joint_sweep_call(query_id, product_id, members, weights, filters, rank_label, k, allow_missing, want_hist, chunk_tiles, True)


def resample_select_device(codes, n_weights: int, count_fit, count_eval, k: int = 5, probes=None, status=None):
    """``mms_resample_select`` on the device codes of ``joint_codes_device`` (uint8 [G, Qa, Wp]) for the first ``n_weights`` vectors.  ``count_fit`` /
    ``count_eval``: uint8 [R, Qa] (device tensors are used in place, host arrays copied up once); ``probes``: items ``v * G + g``, a host list or an
    int64 device tensor; ``status``: the int32 [4] device block to OR the flags into (default: a zeroed one; pass the sweep's to read every flag at
    once).  -> (best int64 [R], fit_value [R], eval_value [R], probe_fit [R, P], probe_eval [R, P], status), device tensors, equal to
    ``resample_select_host`` -- winners entry for entry, values bit for bit.  Only enqueues on the current stream."""
    import torch
    _filter_k(k)
    if not torch.is_tensor(codes) or codes.dtype != torch.uint8 or codes.ndim != 3 or not codes.is_cuda or not codes.is_contiguous():
        raise ValueError("codes must be the contiguous uint8 [G, Qa, Wp] device tensor of joint_codes_device")
    dev = codes.device
    G, Qa, Wp = codes.shape
    W = int(n_weights)
    if W < 0 or Wp != (W + 63) // 64 * 64:
        raise ValueError("resample_select_device: %d weight vectors do not match codes of %s" % (W, tuple(codes.shape)))
    cf, ce = _on_device(count_fit, dev, None), _on_device(count_eval, dev, None)              # (dtype None: kept, and checked below)
    if cf.dtype != torch.uint8 or ce.dtype != torch.uint8 or cf.ndim != 2 or cf.shape != ce.shape or cf.shape[1] != Qa:
        raise ValueError("count_fit / count_eval must be uint8 [R, %d], not %s %s / %s %s" % (Qa, cf.dtype, tuple(cf.shape), ce.dtype, tuple(ce.shape)))
    R = cf.shape[0]
    pr = _on_device(probes if torch.is_tensor(probes) else _probe_array(probes), dev, torch.int64).reshape(-1)
    P = pr.shape[0]
    if R > MAX_REPLICATES or P > MAX_PROBES:
        raise ValueError("at most %d replicates and %d probes per call" % (MAX_REPLICATES, MAX_PROBES))
    call = _DeviceCall(dev, torch.zeros((4,), dtype=torch.int32, device=dev) if status is None else status)      # (the flags are ORed in)
    ws_bytes = call.l.mms_resample_workspace_bytes(W, G, Qa, R)
    if ws_bytes < 0:
        raise ValueError("resample_select_device: %d x %d items, %d key queries, %d replicates: beyond the limits of mms_resample_select" % (W, G, Qa, R))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    best = torch.empty((R,), dtype=torch.int64, device=dev)
    fit_value, eval_value = (torch.empty((R,), dtype=torch.float64, device=dev) for _ in range(2))
    probe_fit, probe_eval = (torch.empty((R, P), dtype=torch.float64, device=dev) for _ in range(2))
    call("mms_resample_select", _ptr(codes), codes.numel(), W, G, Qa, _ptr(cf), _ptr(ce), R, _byte_table(k, dev).data_ptr(), _ptr(pr), P, ws.data_ptr(),
         ws_bytes, _ptr(best), _ptr(fit_value), _ptr(eval_value), _ptr(probe_fit), _ptr(probe_eval), call.status.data_ptr())
    return best, fit_value, eval_value, probe_fit, probe_eval, call.status
