"""Score ensemble + product-uniqueness post-process + top-5 submission.

Restates ``code/main.py:41-104`` of the reference:
* merge: ``0.2*zk + 0.2*zk_sen2forest + 0.3*lds + 0.3*lxmert`` per (query, product) (:59); a product missing
  from one of the first three tables falls back to the lxmert score (:49-57);
* per product, the best merged score over ALL queries and the sorted list of its merged scores (:64-71);
* uniqueness filter (:76-86): a (query, product) survives only if it is that product's best-scoring query
  (|score - best| < 1e-5) and, when the product appears under >= 2 queries, its best beats its
  second best by >= 0.92;
* top-5 per query by merged score; a query left with < 5 survivors falls back to its unfiltered
  merged ranking (:93-104).
The filter is global over queries, so under query sharding it runs on rank 0 after the score gather.
Host-side dict work (29 k entries) exactly as in the reference (``uniqueness_filter`` / ``top5``), its array form
(``submission_rows``, the default), and the same decisions on the GPU (``rank_device`` / ``submission_rows_device``:
``mms_rank_submission``, csrc/rank.hip) for scores that are already device tensors (``sharding.gather_scores``).
"""
from __future__ import annotations

import csv
from collections import OrderedDict

WEIGHTS = (0.2, 0.2, 0.3, 0.3)
GAP = 0.92
TIE = 1e-5


def merge_scores(zk, zk_s2f, lds, lxmert, weights=WEIGHTS):
    merged: OrderedDict = OrderedDict()
    for q in zk:
        r1, r2, r3, r4 = zk[q], zk_s2f[q], lds[q], lxmert[q]
        mq = merged.setdefault(q, OrderedDict())
        for p, s4 in r4.items():
            s1, s2, s3 = r1.get(p, s4), r2.get(p, s4), r3.get(p, s4)
            mq[p] = weights[0] * s1 + weights[1] * s2 + weights[2] * s3 + weights[3] * s4
    return merged


def uniqueness_filter(merged, gap=GAP, tie=TIE):
    scores_of = {}
    for q, d in merged.items():
        for p, s in d.items():
            scores_of.setdefault(p, []).append(s)
    best, keep_product = {}, {}
    for p, lst in scores_of.items():
        lst.sort(reverse=True)
        best[p] = lst[0]
        keep_product[p] = len(lst) < 2 or not (lst[0] - lst[1] < gap)
    out: OrderedDict = OrderedDict()
    for q, d in merged.items():
        for p, s in d.items():
            if keep_product[p] and abs(s - best[p]) < tie:
                out.setdefault(q, OrderedDict())[p] = s
    return out


def top5(merged, filtered):
    """{query: [p1..p5]}: filtered ranking when it has >= 5 entries, else the unfiltered one (main.py:93-104)."""
    rows: OrderedDict = OrderedDict()
    short = []
    for q in filtered:
        r = sorted(filtered[q].items(), key=lambda kv: kv[1], reverse=True)
        if len(r) < 5:
            short.append(q)
            continue
        rows[q] = [p for p, _ in r[:5]]
    for q in short:
        r = sorted(merged[q].items(), key=lambda kv: kv[1], reverse=True)
        rows[q] = [p for p, _ in r[:5]]
    return rows


def submission_rows(query_id, product_id, score, gap=GAP, tie=TIE):
    """``top5(tab, uniqueness_filter(tab))`` for the table ``tab[q][p] = score`` given as three parallel arrays (one row per (query, product) pair, rows of a
    query in any order, first appearance = the table's query order) -- the same rows as the dict walk, computed with sorts instead of 10^5 dict operations
    (0.24 s -> ~20 ms for 120 000 pairs: a tenth of config 5's file-to-submission time was this Python loop).  Equal to the dict form on the reference's
    own tables and on random tables with ties (tests/test_ensemble_ndcg.py).  A (query, product) pair that occurs twice keeps its LAST score, like the dict."""
    import numpy as np
    q = np.asarray(query_id).astype(np.int64)
    p = np.asarray(product_id).astype(np.int64)
    s = np.asarray(score, np.float64)
    n = len(q)
    if n == 0:
        return OrderedDict()
    # table semantics: a repeated (q, p) overwrites the value but keeps its first position
    key = np.stack([q, p], 1)
    _, first_idx, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    if len(first_idx) != n:
        last = np.zeros(len(first_idx), np.int64)
        last[inv] = np.arange(n)                       # later rows win
        keep = np.sort(first_idx)
        s = s.copy()
        s[first_idx[inv]] = s[last[inv]]
        q, p, s = q[keep], p[keep], s[keep]
        n = len(q)
    # per product: best and second-best score over all queries
    order = np.lexsort((-s, p))
    ps, ss = p[order], s[order]
    start = np.flatnonzero(np.r_[True, ps[1:] != ps[:-1]])
    size = np.diff(np.r_[start, n])
    best = ss[start]
    second = np.where(size >= 2, ss[np.minimum(start + 1, n - 1)], -np.inf)
    keep_product = (size < 2) | ~(best - second < gap)
    grp = np.repeat(np.arange(len(start)), size)
    pos = np.empty(n, np.int64)
    pos[order] = grp                                   # row -> its product group
    survive = keep_product[pos] & (np.abs(s - best[pos]) < tie)
    # queries in first-appearance order; within a query a stable sort by descending score (sorted(..., reverse=True) keeps the order of equal scores)
    uq, qfirst, qinv = np.unique(q, return_index=True, return_inverse=True)
    qinv = qinv.reshape(-1)
    n_surv = np.bincount(qinv[survive], minlength=len(uq))
    rows, short = OrderedDict(), []
    rank = np.lexsort((np.arange(n), -s, qinv))        # by query, then score descending, then original position
    qs = qinv[rank]
    qstart = np.flatnonzero(np.r_[True, qs[1:] != qs[:-1]])
    qend = np.r_[qstart[1:], n]
    seg = {int(qs[a]): (a, b) for a, b in zip(qstart, qend)}
    surv_sorted = survive[rank]
    # the filtered table holds the queries that have a survivor, in the table's own query order (= first appearance of the query)
    for qi in np.argsort(qfirst, kind="stable"):
        if n_surv[qi] == 0:
            continue                                   # no survivor: the reference never writes that query (main.py:91-104 walks the filtered table only)
        a, b = seg[int(qi)]
        if n_surv[qi] >= 5:
            r = rank[a:b][surv_sorted[a:b]][:5]
            rows[str(int(uq[qi]))] = [str(int(x)) for x in p[r]]
        else:
            short.append(qi)
    for qi in short:
        a, b = seg[int(qi)]
        rows[str(int(uq[qi]))] = [str(int(x)) for x in p[rank[a:b][:5]]]
    return rows


FLAG_REPEATED_PAIR, FLAG_NON_FINITE, FLAG_OVERFLOW, FLAG_RESERVED_ID = 1, 2, 4, 8      # status[2] of mms_rank_submission (include/mmscore.h)


def rank_device(query_id, product_id, score, gap=GAP, tie=TIE):
    """The filter + top-5 of ``submission_rows`` on the GPU (``mms_rank_submission``).  ``query_id`` / ``product_id`` / ``score``: device tensors
    (used in place when int64 / fp32 or fp64 and contiguous), or numpy arrays / host tensors, copied up once.
    -> (out_query [m] int64, out_products [m, 5] int64 (-1: unused), out_count [m] int32, status [4] int32), device tensors with
    m = the row count (always enough room); status = (output rows, rows of the >= 5-survivor class -- they come first --, flags, distinct queries).
    Only enqueues on the current stream: nothing is read back, nothing waits."""
    import torch

    from .ndcg import _DeviceCall, _ptr, _rows_on_device, _score_ptrs
    (s, q, p), dev = _rows_on_device((score, query_id, product_id), ((torch.float64, torch.float32), (torch.int64,), (torch.int64,)), "rank_device")
    n = s.shape[0]
    call = _DeviceCall(dev)
    ws_bytes = call.l.mms_rank_workspace_bytes(n)
    if ws_bytes < 0:
        raise ValueError("rank_device: %d rows, the device path takes at most MMS_RANK_MAX_ROWS (2^22)" % n)
    m = n                                                                    # at most one output row per input row
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)             # (the caching allocator returns 512-byte aligned blocks)
    out_query = torch.empty((m,), dtype=torch.int64, device=dev)
    out_products = torch.empty((m, 5), dtype=torch.int64, device=dev)
    out_count = torch.empty((m,), dtype=torch.int32, device=dev)
    call("mms_rank_submission", _ptr(q), _ptr(p), *_score_ptrs(s, call.status), n, float(gap), float(tie), ws.data_ptr(), ws_bytes, m, _ptr(out_query),
         _ptr(out_products), _ptr(out_count), call.status.data_ptr())
    return out_query, out_products, out_count, call.status


def submission_rows_device(query_id, product_id, score, gap=GAP, tie=TIE, info=None):
    """``submission_rows`` with the filter and the top-5 on the GPU (``rank_device``): the same ``OrderedDict`` in the same order.  One host read
    carries the status and the first rows (room for a query per 8 input rows, at least 4096; a table with more output rows costs a second read).
    What the device does not do -- a (query, product) pair that occurs twice, a non-finite score, an id equal to the reserved -1 -- it detects:
    the rows then come from ``submission_rows`` on the host arrays.  ``info`` (a dict) receives ``{"path": "device" | "host", "flags": int}``."""
    import torch

    from . import ndcg
    out_query, out_products, out_count, status = rank_device(query_id, product_id, score, gap, tie)
    m = out_query.shape[0]
    g = min(m, max(4096, m // 8))
    pack = lambda k: torch.cat([status.to(torch.int64), out_query[:k], out_count[:k].to(torch.int64), out_products[:k].reshape(-1)])
    host = pack(g).cpu().numpy()                                             # the one synchronising read
    n_out, flags = int(host[0]), int(host[2])
    if info is not None:
        info.update(path="host" if flags else "device", flags=flags)
    if flags:
        return submission_rows(ndcg._to_np(query_id), ndcg._to_np(product_id), ndcg._to_np(score), gap, tie)
    if n_out > g:
        g = n_out
        host = pack(g).cpu().numpy()
    qs = host[4:4 + n_out].tolist()
    cnt = host[4 + g:4 + g + n_out].tolist()
    prods = host[4 + 2 * g:4 + 2 * g + 5 * n_out].tolist()
    rows = OrderedDict()
    for i, qq in enumerate(qs):
        rows[str(qq)] = [str(x) for x in prods[5 * i:5 * i + cnt[i]]]
    return rows


def ensemble(zk, zk_s2f, lds, lxmert):
    merged = merge_scores(zk, zk_s2f, lds, lxmert)
    return top5(merged, uniqueness_filter(merged))


def write_submission(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["query-id", "product1", "product2", "product3", "product4", "product5"])
        for q, ps in rows.items():
            w.writerow([q] + list(ps))


def weight_grid(members: int = 4, steps: int = 20):
    """The simplex grid of step ``1 / steps``: float64 [C(steps + members - 1, members - 1), members], the rows ``np.array(c, float64) / steps`` for
    the integer compositions ``c`` of ``steps`` into ``members`` non-negative parts, in lexicographic order ((0, .., 0, steps) first,
    (steps, 0, .., 0) last).  4 members: 35 rows at steps = 4, 1 771 at 20, 176 851 at 100."""
    import numpy as np
    if members < 1 or steps < 1:
        raise ValueError("weight_grid: members and steps must be >= 1")
    rows, c = [], [0] * members

    def fill(i, left):
        if i == members - 1:
            c[i] = left
            rows.append(tuple(c))
            return
        for x in range(left + 1):
            c[i] = x
            fill(i + 1, left - x)

    fill(0, steps)
    return np.array(rows, np.float64) / steps


def _check_where(where):
    if where not in ("host", "device"):
        raise ValueError("where must be 'host' or 'device', not %r" % (where,))


def _weight_rows(grid, M, who):
    """The weight grid of ``who`` (a ``fit_*`` function's name): float64 [W >= 1, M], ``weight_grid(M, 20)`` by default."""
    import numpy as np
    grid = weight_grid(M, 20) if grid is None else np.ascontiguousarray(grid, np.float64)
    if grid.ndim != 2 or grid.shape[0] == 0:
        raise ValueError("%s: the grid must be [W >= 1, %d]" % (who, M))
    return grid


def _filter_rows(filters, who):
    """The filter grid of ``who``: float64 [G >= 1, 2] rows ``(gap, tie)``, ``filter_grid()`` by default."""
    import numpy as np
    filters = filter_grid() if filters is None else np.ascontiguousarray(filters, np.float64)
    if filters.ndim != 2 or filters.shape[1] != 2 or filters.shape[0] == 0:
        raise ValueError("%s: the filters must be [G >= 1, 2] rows of (gap, tie)" % who)
    return filters


def _joint_result(grid, filters, values, index):
    """The tuple of ``fit_joint`` for the winner ``index`` of the flat ``values`` [W * G] (weight-major)."""
    iw, ig = divmod(index, filters.shape[0])
    return (tuple(float(x) for x in grid[iw]), (float(filters[ig, 0]), float(filters[ig, 1])), float(values[index]), (iw, ig),
            values.reshape(grid.shape[0], filters.shape[0]))


def _fit(device_call, host_call, use_device, info, soft_flags=0):
    """The common half of the ``fit_*`` functions: the values of every grid point, flat in row-major order -- from ``device_call() -> (values,
    status, *extras)`` with ONE synchronising read when ``use_device`` and the device raises no flag but "missing" and ``soft_flags``, else from
    ``host_call() -> values`` -- and the FIRST one that attains the maximum.  ``extras``: further device tensors that ride along in the read.
    -> (index, values, the extras as one flat float64 numpy array in their order; None on the host path)."""
    import numpy as np

    from . import ndcg
    values, rest, flags = None, None, 0
    if use_device:
        import torch
        dvalues, status, *extras = device_call()
        host = torch.cat([x.to(torch.float64).reshape(-1) for x in (status, dvalues, *extras)]).cpu().numpy()   # the one synchronising read
        flags = int(host[2])
        if flags & ~(ndcg.FLAG_MISSING_QUERY | soft_flags) == 0:
            if flags & ndcg.FLAG_MISSING_QUERY:                                  # only without allow_missing
                raise KeyError("%d key queries have no rows" % int(host[3]))
            values, rest = host[4:4 + dvalues.numel()].copy(), host[4 + dvalues.numel():]
    if info is not None:
        info.update(path="device" if values is not None else "host", flags=flags)
    if values is None:
        values = host_call().reshape(-1)
    return int(np.argmax(values)), values, rest                                  # the first point that attains the maximum


# ---- per-query normalisation of the member scores in front of a merge (mms_normalize_members, csrc/normalize.hip) ----
NORMALIZE = ("none", "minmax", "zscore", "rank")          # MMS_NORMALIZE_NONE .. MMS_NORMALIZE_RANK: the index is the library's mode
NORMALIZE_FLAG_NON_FINITE, NORMALIZE_FLAG_RESERVED_ID = 2, 8                             # status[2] of mms_normalize_members (include/mmscore.h)


def _check_normalize(mode):
    if mode not in NORMALIZE:
        raise ValueError("normalize must be one of %s, not %r" % (", ".join(repr(m) for m in NORMALIZE), mode))


def normalize_members(query_id, members, mode):
    """The member scores on a common per-query scale, the definition ``mms_normalize_members`` restates: float32 [M, n] from ``members`` float32
    [M, n] (member-major).  A group is all rows of one query id, in any order, not necessarily adjacent; every member is treated on its own, group
    by group.  With c rows in the group and x_r = float64(members[m][r]) (-0.0 counts as +0.0), in IEEE double, every operation rounded on its
    own, the result rounded once to float32:
      ``"minmax"``  (x - lo) / (hi - lo) with the group's minimum and maximum; +0.0 for every row when hi == lo
      ``"zscore"``  (x - mean) / sd; mean = S1 / c with S1 the sum of x_r taken sequentially in ascending row index from +0.0, sd = sqrt(S2 / c)
                    with S2 the sum of (x_r - mean) * (x_r - mean) taken the same way (population variance); +0.0 for every row unless sd > 0
      ``"rank"``    (c - 1 - g) / (c - 1), g = the rows of the group whose x is strictly greater: the best row 1, the worst 0, ties share a value;
                    +0.0 when c == 1.  Depends only on the order of the scores inside the group.
      ``"none"``    ``members`` itself, unchanged.
    No transcendental function on purpose: the host and the device agree bit for bit."""
    import numpy as np
    _check_normalize(mode)
    if mode == "none":
        return members
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    mem = np.asarray(members, np.float32)
    n = len(q)
    if mem.ndim != 2 or mem.shape[1] != n:
        raise ValueError("normalize_members: members must be [M, %d], not %s" % (n, tuple(mem.shape)))
    M = mem.shape[0]
    out = np.zeros((M, n), np.float32)
    if n == 0 or M == 0:
        return out
    _, inv = np.unique(q, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind="stable")                       # grouped by query, ascending row index inside a group
    gs = inv.reshape(-1)[order]
    head = np.r_[True, gs[1:] != gs[:-1]]
    start = np.flatnonzero(head)
    size = np.diff(np.r_[start, n])
    grp = np.cumsum(head) - 1                                                # sorted position -> its group
    c = size.astype(np.float64)
    x = mem[:, order].astype(np.float64) + 0.0                               # [M, n], grouped; + 0.0 folds -0.0 onto +0.0
    with np.errstate(all="ignore"):                                          # (a non-finite score: the device flags it and the caller lands here)
        if mode == "minmax":
            lo, hi = np.minimum.reduceat(x, start, axis=1)[:, grp], np.maximum.reduceat(x, start, axis=1)[:, grp]
            res = np.where(hi == lo, 0.0, (x - lo) / (hi - lo))
        elif mode == "zscore":
            def seq_sum(term):                                               # per group the sequential sum of term(j-th row of the group), j ascending
                s = np.zeros((M, len(start)), np.float64)
                for j in range(int(size.max())):
                    sel = np.flatnonzero(size > j)
                    s[:, sel] = s[:, sel] + term(start[sel] + j, sel)
                return s
            mean = seq_sum(lambda at, sel: x[:, at]) / c

            def square(at, sel):
                d = x[:, at] - mean[:, sel]
                return d * d
            sd = np.sqrt(seq_sum(square) / c)[:, grp]
            res = np.where(sd > 0, (x - mean[:, grp]) / sd, 0.0)
        else:
            res = np.empty((M, n), np.float64)
            group_end, cc = (start + size)[grp], c[grp]
            for m in range(M):
                o = np.lexsort((x[m], gs))                                   # by group, then score ascending (the groups stay where they are)
                xs = x[m][o]
                new = np.r_[True, (xs[1:] != xs[:-1]) | head[1:]]            # first entry of a run of equal scores inside a group
                run_end = np.r_[np.flatnonzero(new)[1:], n][np.cumsum(new) - 1]
                greater = (group_end - run_end).astype(np.float64)
                res[m, o] = np.where(cc > 1, (cc - 1.0 - greater) / np.maximum(cc - 1.0, 1.0), 0.0)
    out[:, order] = res.astype(np.float32)
    return out


def normalize_members_device(query_id, members, mode, info: dict = None):
    """``normalize_members`` on the GPU (``mms_normalize_members``): -> device float32 [M, n], bit-equal to the host form.  ``members``: fp32 [M, n]
    (a device tensor is used in place, and returned as it is for ``"none"``), ``query_id``: int64 [n]; host arrays are copied up once.  Nothing is
    read back but the status word (one synchronising read).  What the device does not do -- a non-finite score in any member, a query id equal to
    the reserved -1 -- it detects: the result is then the host form's, uploaded.  ``info`` receives ``{"path": "device" | "host", "flags": int,
    "queries", "largest_query"}``."""
    import torch

    from .ndcg import _DeviceCall, _members_on, _on_device, _ptr
    _check_normalize(mode)
    dev = next((t.device for t in (members, query_id) if torch.is_tensor(t) and t.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    mem = _members_on(members, dev)
    q = _on_device(query_id, dev, torch.int64).reshape(-1)
    n = q.shape[0]
    if mem.ndim != 2 or mem.shape[1] != n:
        raise ValueError("normalize_members_device: members must be [M, %d], not %s" % (n, tuple(mem.shape)))
    if mode == "none":
        if info is not None:
            info.update(path="device", flags=0)
        return mem
    call = _DeviceCall(dev)
    ws_bytes = call.l.mms_normalize_workspace_bytes(n, mem.shape[0])
    if ws_bytes < 0:
        raise ValueError("normalize_members_device: %d rows of %d members, the device path takes at most 2^22 rows of 1..8 members" % (n, mem.shape[0]))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)             # (the caching allocator returns 512-byte aligned blocks)
    out = torch.empty_like(mem)
    call("mms_normalize_members", _ptr(q), _ptr(mem), mem.shape[0], n, NORMALIZE.index(mode), _ptr(out), call.status.data_ptr(), ws.data_ptr(), ws_bytes)
    queries, largest, flags, _ = (int(v) for v in call.status.cpu().numpy())  # the one synchronising read
    if info is not None:
        info.update(path="host" if flags else "device", flags=flags, queries=queries, largest_query=largest)
    if flags:
        return torch.from_numpy(normalize_members(q.cpu().numpy(), mem.cpu().numpy(), mode)).to(dev)
    return out


def _normalized(query_id, members, normalize, where, info):
    """The members a ``fit_*`` function sweeps: ``members`` itself for ``"none"``, else normalised ONCE in front of the unchanged sweep -- by the
    device form for ``where="device"``, by the host form for ``where="host"``; ``info`` then receives ``normalize`` (with ``"none"`` it is today's dict)."""
    from . import ndcg
    _check_normalize(normalize)
    if normalize == "none":
        return members
    if info is not None:
        info["normalize"] = normalize
    if where == "device":
        return normalize_members_device(query_id, members, normalize)
    return normalize_members(ndcg._to_np(query_id), ndcg._member_array(members), normalize)


def fit_weights(query_id, product_id, members, rank_label, grid=None, k: int = 5, allow_missing: bool = False, where: str = "device", info: dict = None,
                normalize: str = "none"):
    """The ensemble weights as a result of the valid set: nDCG@k of the merge ``(...(w0 * s0 + w1 * s1) + ...)`` (``ndcg.merge_members``: IEEE double,
    every operation rounded on its own, main.py:59's evaluation) for every row ``w`` of ``grid`` (default ``weight_grid(M, 20)``), and the winner --
    the FIRST grid row that attains the maximum.  ``members``: fp32 [M, n], member-major (a device tensor stays where it is).
    -> (weights tuple, value, index, values float64 numpy [W]).
    ``where="device"``: ``ndcg.ndcg_sweep_device`` (``mms_ndcg_weight_sweep``: one call for the whole grid); ONE synchronising read carries the
    status and the values.  What the device does not do -- a non-finite merged score of a key query's row, a repeated key query, a reserved id --
    it detects: the values then come from ``ndcg.ndcg_sweep_host``, which ``where="host"`` runs directly; both give the same floats, bit for bit.
    A key query without rows raises ``KeyError`` unless ``allow_missing``.  ``info`` (a dict) receives ``{"path": "device" | "host", "flags": int}``.
    ``normalize``: one of ``NORMALIZE``; other than ``"none"`` the members are put on a per-query scale ONCE (``normalize_members_device`` for
    ``where="device"``, ``normalize_members`` for ``"host"``: the same floats) and the sweep runs on the result unchanged; ``info`` then also
    receives ``normalize``."""
    from . import ndcg
    _check_where(where)
    members = _normalized(query_id, members, normalize, where, info)
    label_dict = ndcg._label_dict(rank_label)
    grid = _weight_rows(grid, len(members), "fit_weights")
    index, values, _ = _fit(
        lambda: ndcg.ndcg_sweep_device(query_id, product_id, members, grid, rank_label, k, allow_missing)[::2],
        lambda: ndcg.ndcg_sweep_host(ndcg._to_np(query_id), ndcg._to_np(product_id), ndcg._member_array(members), grid, label_dict, k, allow_missing)[0],
        where == "device" and len(label_dict), info)
    return tuple(float(x) for x in grid[index]), float(values[index]), index, values


def filter_grid(steps: int = 100, tie: float = TIE):
    """The grid ``fit_filter`` searches by default: float64 [steps + 2, 2] rows ``(gap, tie)``.  Row 0 is ``(-inf, +inf)``, "no filter": every product
    kept, every row a survivor, so the output row is the unfiltered top-5; rows ``1 + i`` are ``(i / steps, tie)`` for i = 0..steps."""
    import numpy as np
    if steps < 1:
        raise ValueError("filter_grid: steps must be >= 1")
    g = np.empty((steps + 2, 2), np.float64)
    g[0] = (-np.inf, np.inf)
    g[1:, 0] = np.arange(steps + 1, dtype=np.float64) / steps
    g[1:, 1] = tie
    return g


def fit_filter(query_id, product_id, score, rank_label, filters=None, k: int = 5, allow_missing: bool = False, where: str = "device", info: dict = None):
    """The uniqueness filter's constants as a result of the valid set: nDCG@k of the SUBMISSION rows (``ndcg.submission_codes``: filter, 1..4-survivor
    fallback, dropped queries, divided by the whole key's length) for every row ``(gap, tie)`` of ``filters`` (default ``filter_grid()``), and the
    winner -- the FIRST grid row that attains the maximum, the rule of ``fit_weights``.  -> ((gap, tie), value, index, values float64 numpy [G]).
    ``where="device"``: ``ndcg.filter_sweep_device`` (``mms_filter_sweep``: one call for the whole grid); ONE synchronising read carries the status
    and the values.  What the device does not do -- a (query, product) pair that occurs twice, a non-finite score in any row, a repeated key query,
    a reserved id -- it detects: the values then come from ``ndcg.filter_sweep_host``, which ``where="host"`` runs directly; both give the same
    floats, bit for bit.  A key query without rows raises ``KeyError`` unless ``allow_missing``.  ``info`` receives ``{"path", "flags"}``."""
    from . import ndcg
    _check_where(where)
    label_dict = ndcg._label_dict(rank_label)
    filters = _filter_rows(filters, "fit_filter")
    index, values, _ = _fit(
        lambda: ndcg.filter_sweep_device(query_id, product_id, score, filters, rank_label, k, allow_missing)[::2],
        lambda: ndcg.filter_sweep_host(ndcg._to_np(query_id), ndcg._to_np(product_id), ndcg._to_np(score), filters, label_dict, k, allow_missing)[0],
        where == "device" and len(label_dict), info)
    return (float(filters[index, 0]), float(filters[index, 1])), float(values[index]), index, values


def fit_joint(query_id, product_id, members, rank_label, grid=None, filters=None, k: int = 5, allow_missing: bool = False, where: str = "device",
              info: dict = None, normalize: str = "none"):
    """The merge weights AND the uniqueness filter as ONE result of the valid set: nDCG@k of the SUBMISSION rows (``ndcg.submission_codes`` on the
    merge ``ndcg.merge_members(members, w)``) for every pair of a row ``w`` of ``grid`` (default ``weight_grid(M, 20)``) and a row ``(gap, tie)`` of
    ``filters`` (default ``filter_grid()``), and the winner -- the FIRST pair that attains the maximum in row-major (weight-major) order.  The filter's
    decisions move with the weights, so this optimum can lie strictly above ``fit_weights`` followed by ``fit_filter``, which fits the weights on the
    unfiltered ranking.  -> (weights tuple, (gap, tie), value, (iw, ig), values float64 numpy [W, G]).
    ``where="device"``: ``ndcg.joint_sweep_device`` (``mms_joint_sweep``: one call for both grids); ONE synchronising read carries the status and the
    values.  What the device does not do -- a (query, product) pair that occurs twice, a non-finite merged score in any row, a repeated key query, a
    reserved id -- it detects: the values then come from ``ndcg.joint_sweep_host``, which ``where="host"`` runs directly; both give the same floats,
    bit for bit.  A key query without rows raises ``KeyError`` unless ``allow_missing``.  ``info`` receives ``{"path", "flags"}``.
    ``normalize``: one of ``NORMALIZE``; other than ``"none"`` the members are put on a per-query scale ONCE (``normalize_members_device`` for
    ``where="device"``, ``normalize_members`` for ``"host"``: the same floats) and the sweep runs on the result unchanged; ``info`` then also
    receives ``normalize``."""
    from . import ndcg
    _check_where(where)
    members = _normalized(query_id, members, normalize, where, info)
    label_dict = ndcg._label_dict(rank_label)
    grid, filters = _weight_rows(grid, len(members), "fit_joint"), _filter_rows(filters, "fit_joint")
    index, values, _ = _fit(
        lambda: ndcg.joint_sweep_device(query_id, product_id, members, grid, filters, rank_label, k, allow_missing)[::2],
        lambda: ndcg.joint_sweep_host(ndcg._to_np(query_id), ndcg._to_np(product_id), ndcg._member_array(members), grid, filters, label_dict, k, allow_missing)[0],
        where == "device" and len(label_dict), info)
    return _joint_result(grid, filters, values, index)


# ---- resampling the joint fit: held-out nDCG@k of the (weights, gap, tie) that fit_joint selects ----
RESAMPLE_CODE_BUDGET = 4 << 30            # fit_joint_resampled's cap on the code matrix (G * Qa * Wp bytes): a cap, not a tuned number


def kfold_counts(n_key_queries: int, folds: int = 5, repeats: int = 1, seed: int = 0):
    """The replicates of a (repeated) k-fold split of the key queries: (count_fit, count_eval), uint8 [folds * repeats, n_key_queries].  Repeat ``t``
    assigns key query i to fold ``default_rng(seed + t).permutation(n_key_queries)[i] % folds``; replicate ``t * folds + f`` fits on the queries
    outside fold f (count 1) and evaluates on those inside, so every key query is held out exactly once per repeat."""
    import numpy as np
    if folds < 2 or repeats < 1:
        raise ValueError("kfold_counts: folds must be >= 2 and repeats >= 1")
    if folds > n_key_queries:
        raise ValueError("kfold_counts: %d folds of %d key queries" % (folds, n_key_queries))
    ev = np.zeros((repeats, folds, n_key_queries), np.uint8)
    for t in range(repeats):
        fold = np.random.default_rng(seed + t).permutation(n_key_queries) % folds
        ev[t, fold, np.arange(n_key_queries)] = 1
    ev = ev.reshape(repeats * folds, n_key_queries)
    return (1 - ev).astype(np.uint8), ev


def bootstrap_counts(n_key_queries: int, replicates: int = 200, seed: int = 0):
    """Bootstrap replicates of the key queries: (count_fit, count_eval), uint8 [replicates, n_key_queries].  A fit row holds the multinomial counts of
    n_key_queries draws with replacement (``default_rng(seed).multinomial``); the eval row is its out-of-bag indicator (1 where the count is 0)."""
    import numpy as np
    if n_key_queries < 1 or replicates < 1:
        raise ValueError("bootstrap_counts: n_key_queries and replicates must be >= 1")
    fit = np.random.default_rng(seed).multinomial(n_key_queries, np.full(n_key_queries, 1.0 / n_key_queries), size=replicates)
    if fit.max() > 255:
        raise ValueError("bootstrap_counts: a key query was drawn %d times, the counts are bytes" % int(fit.max()))
    return fit.astype(np.uint8), (fit == 0).astype(np.uint8)


def fit_joint_resampled(query_id, product_id, members, rank_label, grid=None, filters=None, k: int = 5, allow_missing: bool = False,
                        scheme: str = "kfold", folds: int = 5, repeats: int = 4, replicates: int = 200, seed: int = 0, counts=None, probes=(),
                        where: str = "device", info: dict = None, code_budget: int = RESAMPLE_CODE_BUDGET, normalize: str = "none"):
    """``fit_joint`` AND how far its winner can be trusted: the maximum of W x G noisy estimates is biased upward, so the fit is repeated on
    resampled answer keys and graded on the key queries each replicate left out -- from the per-query codes of ONE sweep
    (``ndcg.joint_codes_device`` / ``mms_joint_sweep_codes``), because the filter's product statistics are taken over all rows whatever the key.
    Replicates: ``scheme="kfold"`` -> ``kfold_counts(Qa, folds, repeats, seed)``, ``"bootstrap"`` -> ``bootstrap_counts(Qa, replicates, seed)``, or
    ``counts=(count_fit, count_eval)`` uint8 [R, Qa] of the caller.  Per replicate the FIRST item at the maximum of the count-weighted mean of the
    per-query values (``ndcg.resample_select_host``'s arithmetic) and that item's mean over the eval counts.  ``probes``: further ``(iw, ig)`` pairs
    whose fit / eval values are reported per replicate -- the reference's constants, say; probe 0 is always the whole-key winner.
    -> dict: ``whole`` (the tuple of ``fit_joint``, from the same sweep's values and bit-equal to it), ``winners`` int64 [R, 2] ((iw, ig); -1 for an
    empty fit row), ``fit_values`` / ``eval_values`` [R], ``probe_fit`` / ``probe_eval`` [R, 1 + len(probes)], ``probes`` (the (iw, ig) list),
    ``count_fit`` / ``count_eval``, and the summaries ``heldout`` (nan-mean of eval_values), ``optimism`` (nan-mean of fit - eval) and ``agreement``
    (share of replicates that select the whole-key winner).
    ``where="device"``: the sweep and ``mms_resample_select`` are enqueued back to back and ONE synchronising read carries status, values and the
    resampled results.  Any flag ``fit_joint`` falls back on sends this call to the host forms too (``ndcg.joint_sweep_host``,
    ``ndcg.joint_codes_host``, ``ndcg.resample_select_host``), which ``where="host"`` runs directly; ``info`` receives ``{"path", "flags"}``.
    The code matrix takes G * Qa * 64 * ceil(W / 64) bytes (90 MB at the default grids on the valid set); over ``code_budget`` bytes (default
    4 GiB) the call raises ``ValueError``: fit a coarser grid.
    ``normalize``: one of ``NORMALIZE``; other than ``"none"`` the members are put on a per-query scale ONCE (``normalize_members_device`` for
    ``where="device"``, ``normalize_members`` for ``"host"``: the same floats) and the sweep runs on the result unchanged; ``info`` then also
    receives ``normalize``."""
    import numpy as np

    from . import ndcg
    _check_where(where)
    members = _normalized(query_id, members, normalize, where, info)
    label_dict = ndcg._label_dict(rank_label)
    Qa = len(label_dict)
    grid, filters = _weight_rows(grid, len(members), "fit_joint_resampled"), _filter_rows(filters, "fit_joint_resampled")
    W, G = grid.shape[0], filters.shape[0]
    code_bytes = G * Qa * ((W + 63) // 64 * 64)
    if code_bytes > code_budget:
        raise ValueError("fit_joint_resampled: the code matrix of %d x %d grid points and %d key queries takes %d bytes, over the budget of %d: "
                         "fit a coarser grid (fewer weight steps or filters) or raise code_budget" % (W, G, Qa, code_bytes, code_budget))
    if counts is not None:
        count_fit, count_eval = (np.ascontiguousarray(c) for c in counts)
    elif scheme == "kfold":
        count_fit, count_eval = kfold_counts(Qa, folds, repeats, seed)
    elif scheme == "bootstrap":
        count_fit, count_eval = bootstrap_counts(Qa, replicates, seed)
    else:
        raise ValueError("scheme must be 'kfold' or 'bootstrap', not %r" % (scheme,))
    count_fit, count_eval = ndcg._count_arrays(count_fit, count_eval, Qa)
    R = count_fit.shape[0]
    probes = [(int(a), int(b)) for a, b in probes]
    if any(not (0 <= a < W and 0 <= b < G) for a, b in probes) or 1 + len(probes) > ndcg.MAX_PROBES:
        raise ValueError("fit_joint_resampled: probes are at most %d (iw, ig) pairs inside the %d x %d grids" % (ndcg.MAX_PROBES - 1, W, G))
    user_items = np.array([a * G + b for a, b in probes], np.int64)
    P = 1 + len(probes)

    def device_call():
        import torch
        values, _, status, codes = ndcg.joint_codes_device(query_id, product_id, members, grid, filters, rank_label, k, allow_missing)
        flat = values.reshape(-1)
        # the whole-key winner, the first item at the maximum, stays on the device as probe 0 (index plumbing on [W * G]; checked after the read)
        first = torch.where(flat == flat.max(), torch.arange(W * G, device=flat.device), W * G).min().reshape(1)
        items = torch.cat([first, torch.from_numpy(user_items).to(flat.device)])
        return (flat, status, first) + ndcg.resample_select_device(codes, W, count_fit, count_eval, k, items, status)[:5]

    def host_call():
        qh, ph, mem = ndcg._to_np(query_id), ndcg._to_np(product_id), ndcg._member_array(members)
        values = ndcg.joint_sweep_host(qh, ph, mem, grid, filters, label_dict, k, allow_missing)[0]
        codes = ndcg.joint_codes_host(qh, ph, mem, grid, filters, label_dict, k, allow_missing)
        res.extend(ndcg.resample_select_host(codes, count_fit, count_eval, k, np.r_[np.int64(np.argmax(values)), user_items]))
        return values

    res = []
    index, values, rest = _fit(device_call, host_call, where == "device" and Qa, info, soft_flags=ndcg.FLAG_EMPTY_FIT)
    if rest is not None:                                                         # first [1], best, fit, eval [R], probe_fit, probe_eval [R, P]
        if int(rest[0]) != index:
            raise RuntimeError("fit_joint_resampled: probe 0 is item %d, the whole-key winner item %d" % (int(rest[0]), index))
        best, fv, ev, pf, pe = np.split(rest[1:], np.cumsum([R, R, R, R * P]))
        res = [best.astype(np.int64), fv.copy(), ev.copy(), pf.reshape(R, P).copy(), pe.reshape(R, P).copy()]
    iw, ig = divmod(index, G)
    whole = _joint_result(grid, filters, values, index)
    best, fit_values, eval_values, probe_fit, probe_eval = res
    winners = np.where(best[:, None] >= 0, np.stack([best // G, best % G], 1), -1)
    gap = fit_values - eval_values
    heldout = float(np.mean(eval_values[~np.isnan(eval_values)])) if not np.isnan(eval_values).all() else float("nan")      # the nan-means
    optimism = float(np.mean(gap[~np.isnan(gap)])) if not np.isnan(gap).all() else float("nan")
    return dict(whole=whole, winners=winners, fit_values=fit_values, eval_values=eval_values, probe_fit=probe_fit, probe_eval=probe_eval,
                probes=[(iw, ig)] + probes, count_fit=count_fit, count_eval=count_eval, heldout=heldout, optimism=optimism,
                agreement=float(np.mean(best == index)) if R else float("nan"))


# ---- cascade: lxmert prunes each query to its best `keep` pairs, the other three members score what is left (mms_score_ensemble_cascade) ----
CASCADE_FLAG_NON_FINITE, CASCADE_FLAG_RESERVED_ID, CASCADE_FLAG_TOO_MANY = 1, 2, 4      # status[0] of mms_cascade_select (include/mmscore.h)


def cascade_keep(query_id, stage1, keep: int, parts=None):
    """The selection of the cascade on the host, the reference of ``mms_cascade_select``: within each query the rows are ordered by (``stage1``
    descending, row ascending; -0.0 == +0.0, the fp32 values compared exactly) and the first ``min(keep, rows)`` are kept.
    -> (kept bool [n], kept_list int32: the kept rows in ascending row order).  ``parts``: batch offsets (ascending row indices; 0 and n may be
    left out) -- the device sees one batch per call, so a query cut by an offset is selected per part: never fewer rows kept, only more."""
    import numpy as np
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    s = np.asarray(stage1, np.float32).astype(np.float64).reshape(-1) + 0.0          # + 0.0 folds -0.0 onto +0.0
    n = len(q)
    if len(s) != n:
        raise ValueError("cascade_keep: %d query ids, %d scores" % (n, len(s)))
    if keep < 1:
        raise ValueError("cascade_keep: keep must be >= 1")
    kept = np.zeros(n, bool)
    cuts = sorted({0, n} | {int(c) for c in (parts if parts is not None else ()) if 0 < int(c) < n})
    for a, b in zip(cuts[:-1], cuts[1:]):
        order = a + np.lexsort((np.arange(b - a), -s[a:b], q[a:b]))                  # by query, score descending, row ascending
        qs = q[order]
        start = np.flatnonzero(np.r_[True, qs[1:] != qs[:-1]])
        rank = np.arange(b - a) - np.repeat(start, np.diff(np.r_[start, b - a]))
        kept[order[rank < keep]] = True
    return kept, np.flatnonzero(kept).astype(np.int32)


def cascade_keep_device(query_id, stage1, keep: int, info: dict = None):
    """``cascade_keep`` of ONE batch on the GPU (``mms_cascade_select``): -> (kept bool [n], kept_list int32 [n_kept]) as device tensors; one
    synchronising read of the status word.  On a flag (a non-finite score, a query id equal to the reserved -1, more than 2^22 rows) the device
    keeps every row; the result then comes from the host form.  ``info`` receives ``{"path", "flags", "n_kept", "queries", "largest_query"}``."""
    import torch

    from .ndcg import _DeviceCall, _ptr, _rows_on_device
    (s, q), dev = _rows_on_device((stage1, query_id), ((torch.float32,), (torch.int64,)), "cascade_keep_device")
    n = s.shape[0]
    call = _DeviceCall(dev)
    ws_bytes = call.l.mms_cascade_workspace_bytes(n)
    if ws_bytes < 0:
        raise ValueError("cascade_keep_device: %d rows" % n)
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=dev)
    kept = torch.empty((n,), dtype=torch.uint8, device=dev)
    kept_list = torch.empty((n,), dtype=torch.int32, device=dev)
    call("mms_cascade_select", _ptr(q), _ptr(s), n, int(keep), _ptr(kept), _ptr(kept_list), call.status.data_ptr(), ws.data_ptr(), ws_bytes)
    flags, n_kept, queries, largest = (int(v) for v in call.status.cpu().numpy())    # the one synchronising read
    if info is not None:
        info.update(path="host" if flags else "device", flags=flags, n_kept=n_kept, queries=queries, largest_query=largest)
    if flags:
        hk, hl = cascade_keep(q.cpu().numpy(), s.cpu().numpy(), keep)
        return torch.from_numpy(hk).to(dev), torch.from_numpy(hl).to(dev)
    return kept.bool(), kept_list[:n_kept]


def cascade_members(members, kept):
    """The member scores the cascade returns for the selection ``kept``: rows 0-2 of a pruned pair are 0.0, row 3 (lxmert, the first stage) stays.
    ``members``: fp32 [4, n], numpy or a tensor (the result lives where ``members`` does)."""
    import numpy as np
    if hasattr(members, "detach"):
        import torch
        k = torch.as_tensor(kept, device=members.device).bool()
        out = members.clone()
        out[:3, ~k] = 0.0
        return out
    out = np.array(members, np.float32, copy=True)
    out[:3, ~np.asarray(kept, bool)] = 0.0
    return out


def cascade_curve(query_id, product_id, members, rank_label, keeps, weights=WEIGHTS, gap=GAP, tie=TIE, k: int = 5, parts=None, where: str = "device"):
    """What a given ``keep`` costs in nDCG, read off ONE full pass over the valid set (``members``: fp32 [4, n] of ``mms_score_ensemble``; member 3 is
    the first stage).  -> a list with one dict per ``keep``:
      ``keep``; ``kept``: the pairs the cascade would send through stage 2; ``fraction``: kept / n;
      ``ndcg``: nDCG@k of the SUBMISSION rows of the cascade's scores -- ``fit_joint`` on ``cascade_members(members, kept)`` with the one-row weight
      grid ``weights`` and the one-row filter grid ``(gap, tie)``, so that ``where="device"`` and ``where="host"`` give the same float;
      ``changed``: the queries whose submission row differs from the full ensemble's (a row only one of the two writes counts), from
      ``submission_rows`` on ``ndcg.merge_members`` of the host copies.
    ``parts``: the batch offsets of the pass (``cascade_keep``).  The members of a pruned pair are exact zeros, as on the device; what the curve cannot
    show is the round-off between a stage 2 of n_kept pairs and the full pass's launch regimes (<= 2e-5 on a score, include/mmscore.h)."""
    import numpy as np

    from . import ndcg
    _check_where(where)
    q, p, mem = ndcg._to_np(query_id).astype(np.int64), ndcg._to_np(product_id).astype(np.int64), np.asarray(ndcg._to_np(members), np.float32)
    n = len(q)
    grid = np.array([weights], np.float64)
    filters = np.array([[gap, tie]], np.float64)
    full_rows = submission_rows(q, p, ndcg.merge_members(mem, grid[0]), gap, tie)
    out = []
    for keep in keeps:
        kept, _ = cascade_keep(q, mem[3], int(keep), parts)
        cm = cascade_members(mem, kept)
        if where == "device":
            import torch
            dev = members.device if hasattr(members, "detach") and members.is_cuda else torch.device("cuda", torch.cuda.current_device())
            value = fit_joint(query_id, product_id, torch.from_numpy(cm).to(dev), rank_label, grid, filters, k, where="device")[2]
        else:
            value = fit_joint(q, p, cm, rank_label, grid, filters, k, where="host")[2]
        rows = submission_rows(q, p, ndcg.merge_members(cm, grid[0]), gap, tie)
        changed = sum(1 for qq in set(full_rows) | set(rows) if full_rows.get(qq) != rows.get(qq))
        out.append(dict(keep=int(keep), kept=int(kept.sum()), fraction=float(kept.sum()) / n if n else 1.0, ndcg=float(value), changed=int(changed)))
    return out


# ---- plans: ordered stages of members with a rule that decides which rows go on (mms_score_ensemble_plan, include/mmscore.h) ----
PLAN_MEMBERS = {"zk": 1, "lds": 2, "lxmert": 4}          # MMS_MEMBER_ZK (members 0 and 1 together) / MMS_MEMBER_LDS / MMS_MEMBER_LX
PLAN_MAX_STAGES = 3
_PLAN_ROWS = {1: (0, 1), 2: (2,), 4: (3,)}               # member mask bit -> rows of the [4, n] table


def _plan_rows(mask):
    return [r for bit, rows in _PLAN_ROWS.items() if mask & bit for r in rows]


def plan(stages):
    """Normalises a plan to a tuple of ``(members mask, keep, safe_k)`` rows -- the ``mms_plan_stage`` records -- and raises ``ValueError`` on every
    violation of the stage rules of include/mmscore.h.  A stage is ``(members, rule)``: ``members`` names joined by ``+`` (``"zk"`` = both zk members,
    ``"lds"``, ``"lxmert"``) or a mask; ``rule`` is ``None`` (the last stage), an int ``keep`` or ``("safe", k)``.  Example:
    ``[("lxmert", 10), ("zk", ("safe", 5)), ("lds", None)]``.  A normalised plan (rows of three ints) passes through unchanged."""
    stages = list(stages)
    if not 1 <= len(stages) <= PLAN_MAX_STAGES:
        raise ValueError("plan: 1 to %d stages, not %d" % (PLAN_MAX_STAGES, len(stages)))
    out, seen = [], 0
    for s, st in enumerate(stages):
        st = tuple(st) if isinstance(st, (tuple, list)) else (st, None)
        if len(st) == 3:
            names, keep, safe_k = st
            import numbers
            if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 for v in (keep, safe_k)):
                raise ValueError("plan: stage %d: keep and safe_k must be ints >= 0, not %r / %r" % (s, keep, safe_k))
            keep, safe_k = int(keep), int(safe_k)
        elif len(st) == 2:
            names, rule = st
            keep = safe_k = 0
            if rule is None:
                pass
            elif isinstance(rule, (tuple, list)):
                if len(rule) != 2 or rule[0] != "safe" or isinstance(rule[1], bool) or not isinstance(rule[1], (int,)) or rule[1] < 1:
                    raise ValueError("plan: stage %d: the safe rule is (\"safe\", k) with an int k >= 1, not %r" % (s, rule))
                safe_k = int(rule[1])
            elif isinstance(rule, bool) or not isinstance(rule, int) or rule < 1:
                raise ValueError("plan: stage %d: keep must be an int >= 1, not %r" % (s, rule))
            else:
                keep = int(rule)
        else:
            raise ValueError("plan: stage %d: (members, rule) expected, not %r" % (s, st))
        if isinstance(names, str):
            mask = 0
            for nm in names.split("+"):
                nm = nm.strip()
                if nm not in PLAN_MEMBERS:
                    raise ValueError("plan: stage %d: unknown member %r (one of %s)" % (s, nm, ", ".join(PLAN_MEMBERS)))
                if mask & PLAN_MEMBERS[nm]:
                    raise ValueError("plan: stage %d names %r twice" % (s, nm))
                mask |= PLAN_MEMBERS[nm]
        elif isinstance(names, bool) or not isinstance(names, int):
            raise ValueError("plan: stage %d: members are names joined by + or a mask, not %r" % (s, names))
        else:
            mask = names
        if not 1 <= mask <= 7:
            raise ValueError("plan: stage %d: the members must be a non-empty subset of zk+lds+lxmert" % s)
        if mask & seen:
            raise ValueError("plan: stage %d repeats a member of an earlier stage" % s)
        seen |= mask
        if s == len(stages) - 1:
            if keep or safe_k:
                raise ValueError("plan: the last stage selects nothing (rule None)")
        elif (keep >= 1) == (safe_k >= 1):
            raise ValueError("plan: stage %d needs exactly one of keep >= 1 / (\"safe\", k >= 1)" % s)
        out.append((mask, keep, safe_k))
    return tuple(out)


def _plan_weights(pl, weights):
    import numpy as np
    w = np.asarray(weights, np.float32).reshape(-1)
    if len(w) != 4:
        raise ValueError("a plan merges four members, not %d weights" % len(w))
    if any(sk for _, _, sk in pl) and not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("a plan with a safe stage needs finite weights >= 0")
    return w


def plan_from_weights(w):
    """The one-stage plan without the members whose weight is zero (zk: both of its weights): what ``fit_weights`` / ``fit_joint`` may return."""
    w = [float(x) for x in w]
    if len(w) != 4:
        raise ValueError("the ensemble merges four members, not %d" % len(w))
    mask = (1 if (w[0] != 0.0 or w[1] != 0.0) else 0) | (2 if w[2] != 0.0 else 0) | (4 if w[3] != 0.0 else 0)
    if not mask:
        raise ValueError("plan_from_weights: every weight is zero")
    return plan([(mask, None)])


def plan_merge(members, weights):
    """``((w0 * T0 + w1 * T1) + w2 * T2) + w3 * T3`` in fp32, every product and every sum a numpy operation of its own: ``k_merge4``'s expression."""
    import numpy as np
    t = np.asarray(members, np.float32)
    w = np.asarray(weights, np.float32)
    p0 = w[0] * t[0]
    p1 = w[1] * t[1]
    acc = p0 + p1
    p2 = w[2] * t[2]
    acc = acc + p2
    p3 = w[3] * t[3]
    acc = acc + p3
    return acc


def cascade_safe_keep(query_id, lower, upper, k: int, parts=None):
    """The safe selection on the host, the reference of ``mms_cascade_select_safe``: row i is pruned iff at least ``k`` OTHER rows j of its query have
    ``lower[j] > upper[i]`` (strict; the fp32 values, -0.0 == +0.0).  -> (kept bool [n], kept_list int32).  ``parts`` as ``cascade_keep``."""
    import numpy as np
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    lo = np.asarray(lower, np.float32).astype(np.float64).reshape(-1) + 0.0
    up = np.asarray(upper, np.float32).astype(np.float64).reshape(-1) + 0.0
    n = len(q)
    if len(lo) != n or len(up) != n:
        raise ValueError("cascade_safe_keep: %d query ids, %d / %d bounds" % (n, len(lo), len(up)))
    if k < 1:
        raise ValueError("cascade_safe_keep: k must be >= 1")
    kept = np.ones(n, bool)
    cuts = sorted({0, n} | {int(c) for c in (parts if parts is not None else ()) if 0 < int(c) < n})
    for a, b in zip(cuts[:-1], cuts[1:]):
        order = a + np.lexsort((lo[a:b], q[a:b]))                                    # by query, lower ascending
        qs = q[order]
        start = np.flatnonzero(np.r_[True, qs[1:] != qs[:-1]])
        for g0, g1 in zip(start, np.r_[start[1:], b - a]):
            rows = order[g0:g1]
            if len(rows) <= k:
                continue
            above = len(rows) - np.searchsorted(lo[rows], up[rows], side="right")    # rows of the query with lower > upper[i] ...
            above = above - (lo[rows] > up[rows])                                   # ... other than i itself
            kept[rows[above >= k]] = False
    return kept, np.flatnonzero(kept).astype(np.int32)


def cascade_safe_keep_device(query_id, lower, upper, k: int, info: dict = None):
    """``cascade_safe_keep`` of ONE batch on the GPU (``mms_cascade_select_safe``): -> (kept bool [n], kept_list int32 [n_kept]) as device tensors; one
    synchronising read of the status word.  On a flag the device keeps every row; the result then comes from the host form.  ``info`` as
    ``cascade_keep_device``."""
    import torch

    from .ndcg import _DeviceCall, _ptr, _rows_on_device
    (lo, up, q), dev = _rows_on_device((lower, upper, query_id), ((torch.float32,), (torch.float32,), (torch.int64,)), "cascade_safe_keep_device")
    n = lo.shape[0]
    call = _DeviceCall(dev)
    ws_bytes = call.l.mms_cascade_safe_workspace_bytes(n)
    if ws_bytes < 0:
        raise ValueError("cascade_safe_keep_device: %d rows" % n)
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=dev)
    kept = torch.empty((n,), dtype=torch.uint8, device=dev)
    kept_list = torch.empty((n,), dtype=torch.int32, device=dev)
    call("mms_cascade_select_safe", _ptr(q), _ptr(lo), _ptr(up), n, int(k), _ptr(kept), _ptr(kept_list), call.status.data_ptr(), ws.data_ptr(), ws_bytes)
    flags, n_kept, queries, largest = (int(v) for v in call.status.cpu().numpy())    # the one synchronising read
    if info is not None:
        info.update(path="host" if flags else "device", flags=flags, n_kept=n_kept, queries=queries, largest_query=largest)
    if flags:
        hk, hl = cascade_safe_keep(q.cpu().numpy(), lo.cpu().numpy(), up.cpu().numpy(), k)
        return torch.from_numpy(hk).to(dev), torch.from_numpy(hl).to(dev)
    return kept.bool(), kept_list[:n_kept]


def _plan_reached_batch(q, mem, pl, w):
    """plan_reached of ONE batch (one device call): the table, the bounds and the selections exactly as include/mmscore.h defines them."""
    import numpy as np
    n = len(q)
    table = np.zeros((4, n), np.float32)
    reached = np.zeros(n, np.uint8)
    act = np.arange(n)
    later = 0
    for mask, _, _ in pl:
        later |= mask
    for s, (mask, keep, safe_k) in enumerate(pl):
        later &= ~mask
        rows = _plan_rows(mask)
        table[np.ix_(rows, act)] = mem[np.ix_(rows, act)]
        reached[act] += 1
        if s == len(pl) - 1 or len(act) == 0:
            break
        lower = plan_merge(table[:, act], w)
        filled = table[:, act].copy()
        filled[_plan_rows(later)] = np.float32(1.0)
        upper = plan_merge(filled, w)
        flagged = (q[act] == -1).any() or len(act) > (1 << 22) or not np.isfinite(lower).all() or (safe_k >= 1 and not np.isfinite(upper).all())
        if flagged:
            continue                                                                 # a flag sends every row of the stage on
        kept = cascade_keep(q[act], lower, keep)[0] if keep >= 1 else cascade_safe_keep(q[act], lower, upper, safe_k)[0]
        act = act[kept]
    return reached


def plan_reached(query_id, members, plan_, weights=WEIGHTS, parts=None):
    """How many stages of ``plan_`` each row goes through (uint8 [n], 1 .. stages), read off a FULL member table (fp32 [4, n], e.g. of
    ``mms_score_ensemble``): the host definition of ``mms_score_ensemble_plan``'s ``reached``.  All arithmetic in fp32, one operation per statement.
    ``parts``: batch offsets -- every batch is a call of its own, so a query cut by an offset is selected per part."""
    import numpy as np
    pl = plan(plan_)
    w = _plan_weights(pl, weights)
    q = np.asarray(query_id).astype(np.int64).reshape(-1)
    mem = np.asarray(members, np.float32)
    n = len(q)
    if mem.shape != (4, n):
        raise ValueError("plan_reached: members must be [4, %d], not %s" % (n, mem.shape))
    reached = np.zeros(n, np.uint8)
    cuts = sorted({0, n} | {int(c) for c in (parts if parts is not None else ()) if 0 < int(c) < n})
    for a, b in zip(cuts[:-1], cuts[1:]):
        reached[a:b] = _plan_reached_batch(q[a:b], mem[:, a:b], pl, w)
    return reached


def plan_scored(reached, n_stages: int):
    """The pairs each stage scores, ``mms_score_ensemble_plan``'s ``n_scored_out``, from ``reached``."""
    import numpy as np
    r = np.asarray(reached)
    return [int((r >= s + 1).sum()) for s in range(n_stages)]


def plan_members(members, plan_, reached):
    """The member table a plan returns for ``reached``: a member's row holds the full table's score where the row reached the member's stage and
    +0.0 elsewhere (a member of no stage: zeros).  ``members``: fp32 [4, n], numpy or a tensor (the result lives where ``members`` does)."""
    import numpy as np
    pl = plan(plan_)
    if hasattr(members, "detach"):
        import torch
        r = torch.as_tensor(np.asarray(reached.cpu() if hasattr(reached, "detach") else reached), device=members.device)
        out = torch.zeros_like(members)
        for s, (mask, _, _) in enumerate(pl):
            for row in _plan_rows(mask):
                out[row] = torch.where(r >= s + 1, members[row], out[row])
        return out
    mem = np.asarray(members, np.float32)
    r = np.asarray(reached)
    out = np.zeros_like(mem)
    for s, (mask, _, _) in enumerate(pl):
        for row in _plan_rows(mask):
            out[row] = np.where(r >= s + 1, mem[row], np.float32(0.0))
    return out


def _topk_lists(q, score, k):
    """{query: the rows of its k best by (score descending, row ascending)}"""
    import numpy as np
    order = np.lexsort((np.arange(len(q)), -(score.astype(np.float64) + 0.0), q))
    qs = q[order]
    start = np.flatnonzero(np.r_[True, qs[1:] != qs[:-1]]) if len(q) else np.zeros(0, np.int64)
    return {int(qs[a]): tuple(order[a:min(a + k, b)].tolist()) for a, b in zip(start, np.r_[start[1:], len(q)])}


def plan_curve(query_id, product_id, members, rank_label, plans, weights=WEIGHTS, gap=GAP, tie=TIE, k: int = 5, parts=None, where: str = "device"):
    """What each of ``plans`` costs, read off ONE full pass over the valid set (``members``: fp32 [4, n] of ``mms_score_ensemble``).  -> one dict per plan:
      ``plan`` (normalised); ``scored``: the pairs each stage scores; ``fraction``: per stage, scored / n;
      ``ndcg``: nDCG@k of the SUBMISSION rows of the plan's scores -- ``fit_joint`` on ``plan_members`` with the one-row grids ``weights`` and
      ``(gap, tie)``, so that ``where="device"`` and ``where="host"`` give the same float;
      ``changed``: the queries whose submission row differs from the full table's (``submission_rows`` on ``ndcg.merge_members``, as ``cascade_curve``);
      ``topk_changed``: the queries whose top ``k`` of the merged score (fp32, ``plan_merge``; score descending, row ascending) differs from the full
      table's -- 0 for a plan over all members whose only pruning stages are ``("safe", >= k)``; the uniqueness filter is what ``changed`` shows.
    What the curve cannot show is the round-off between a later stage's launch regimes and the full pass's (<= 2e-5 on a score, include/mmscore.h)."""
    import numpy as np

    from . import ndcg
    _check_where(where)
    q, p, mem = ndcg._to_np(query_id).astype(np.int64), ndcg._to_np(product_id).astype(np.int64), np.asarray(ndcg._to_np(members), np.float32)
    n = len(q)
    grid = np.array([weights], np.float64)
    filters = np.array([[gap, tie]], np.float64)
    full_rows = submission_rows(q, p, ndcg.merge_members(mem, grid[0]), gap, tie)
    full_top = _topk_lists(q, plan_merge(mem, weights), k)
    out = []
    for pl in plans:
        pl = plan(pl)
        reached = plan_reached(q, mem, pl, weights, parts)
        pm = plan_members(mem, pl, reached)
        if where == "device":
            import torch
            dev = members.device if hasattr(members, "detach") and members.is_cuda else torch.device("cuda", torch.cuda.current_device())
            value = fit_joint(query_id, product_id, torch.from_numpy(pm).to(dev), rank_label, grid, filters, k, where="device")[2]
        else:
            value = fit_joint(q, p, pm, rank_label, grid, filters, k, where="host")[2]
        rows = submission_rows(q, p, ndcg.merge_members(pm, grid[0]), gap, tie)
        changed = sum(1 for qq in set(full_rows) | set(rows) if full_rows.get(qq) != rows.get(qq))
        top = _topk_lists(q, plan_merge(pm, weights), k)
        scored = plan_scored(reached, len(pl))
        out.append(dict(plan=pl, scored=scored, fraction=[float(c) / n if n else 1.0 for c in scored], ndcg=float(value), changed=int(changed),
                        topk_changed=int(sum(1 for qq in full_top if full_top[qq] != top[qq]))))
    return out
