// Cascade selection on the device (mms_cascade_select, include/mmscore.h): the per-query top-`keep` of a first-stage score over two parallel
// arrays (group_id, score), decision for decision what ensemble.cascade_keep computes on the host -- and the two small kernels around the second
// stage of mms_score_ensemble_cascade (first-stage column out of the probabilities; scatter of the second stage's scores + merge).
//
//   within a query the rows are ordered by (score descending, row ascending); the first min(keep, rows) of that order are kept
//   kept_list = the kept rows in ascending row order, n_kept their number
//
// No sort: a row is kept iff fewer than `keep` rows of its query rank before it, every comparison on the order-preserving integer image of the
// score widened to double (enc_score: -0.0 folded onto +0.0).  Two fills (the key table to 0xFF, the value tables to 0) and nine launches:
//   k_cas_insert      row -> slot of its query in an open-addressing table (capacity >= 2 n); rows per query (atomic add, one per RUN of equal
//                     ids inside a wavefront: wave_run), first row per query (atomic max of the inverted row); flags
//   k_cas_scan_*      one exclusive scan over the rows of two per-row values that are non-zero on a query's FIRST row only: "rows of the query",
//                     "is a first row" -> list offset, query number (block sums / top / apply; block_scan and scan_top of rank_tables.h)
//   k_cas_scatter     rows grouped by query (scatter_rows; the order inside a list does not matter)
//   k_cas_mark        one wavefront per query: a lane owns a row of the list and counts the rows that rank before it (ranks_before), stopping at
//                     `keep`; a query of at most `keep` rows is kept without a comparison.  No limit on the rows of a query or on `keep`
//   k_cas_kept_*      kept byte per row (all ones under a flag), exclusive scan over the rows in row order, compact list
// The SAFE selection (mms_cascade_select_safe) is the same front and back around another mark kernel, with two images per row (enc: the row's lower bound,
// enc_up: its upper bound; k_cas_insert<true>):
//   k_cas_mark_safe   one wavefront per query: a lane owns a row and counts the OTHER rows of the list whose lower image exceeds its upper image, stopping at k;
//                     the row is pruned iff it finds k.  A query of at most k rows is kept without a comparison
// and the three small kernels around the stages of mms_score_ensemble_plan (k_plan_scatter, k_plan_bounds, k_plan_merge) are at the end.
// The only atomics are integer add / max / or / compare-and-swap whose final memory value is independent of the arrival order, and the values
// they return (a list position in k_cas_scatter) never reach the output: equal inputs give equal bytes.
#include "rank_tables.h"

namespace {

constexpr int SCAN_ROWS = 1024;                             // rows per workgroup of the scan kernels: 256 threads x 4

struct CasWs {               // device workspace carved by cas_layout(); [cap] tables first (the 0xFF part, then the zero part), [n] arrays after
    long long* qkey;                                                             // 0xFF
    int* qcnt; int* qfill; unsigned* qfirst_inv;                                 // 0
    int* qoff;                                                                   // written before read
    u64* enc; int* qslot; int* qlist; int* qsel; int* mark; int4* bsum; int* ksum;
    u64* enc_up;                                                                 // the safe selection only: the image of a row's upper bound (enc: its lower bound)
    unsigned mask; int cap;
    size_t ff_bytes, zero_bytes, total_bytes;
};

CasWs cas_layout(void* base, long long n, bool safe = false) {
    CasWs w{};
    const int cap = rank_table_slots(n);
    w.cap = cap; w.mask = (unsigned)(cap - 1);
    Carver cv{(char*)base, 0};
    const size_t c = (size_t)cap, r = (size_t)(n > 0 ? n : 1), nb = (r + SCAN_ROWS - 1) / SCAN_ROWS;
    cv.take(w.qkey, c);
    w.ff_bytes = cv.o;
    cv.take(w.qcnt, c); cv.take(w.qfill, c); cv.take(w.qfirst_inv, c);
    w.zero_bytes = cv.o - w.ff_bytes;
    cv.take(w.qoff, c);
    cv.take(w.enc, r); cv.take(w.qslot, r); cv.take(w.qlist, r); cv.take(w.qsel, r); cv.take(w.mark, r);
    cv.take(w.bsum, nb); cv.take(w.ksum, nb);
    if (safe) cv.take(w.enc_up, r);
    w.total_bytes = cv.o;
    return w;
}

// SAFE: `score` is the lower bound and `upper` the upper bound of a row (two images per row; either one non-finite raises the flag)
template <bool SAFE>
__global__ __launch_bounds__(256) void k_cas_insert(const long long* gid, const float* score, const float* upper, int n, CasWs w, int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool live = r < n;
    long long q = 0;
    double s = 0.0, u = 0.0;
    if (live) {
        q = gid[r]; s = (double)score[r];                                // fp32 -> fp64 is exact
        if (SAFE) u = (double)upper[r];
        int flags = 0;
        if (!finite_score(s) || !finite_score(u)) flags |= MMS_CASCADE_FLAG_NONFINITE;
        if (q == RANK_EMPTY) flags |= MMS_CASCADE_FLAG_RESERVED_ID;
        if (flags) { atomicOr(&status[0], flags); live = false; w.qslot[r] = -1; }
    }
    const Run run = wave_run(q, live);
    const int lane = threadIdx.x & 63;
    int qs = -1;
    if (live) {
        w.enc[r] = enc_score(s);
        if (SAFE) w.enc_up[r] = enc_score(u);
        if (lane == run.head) {                                          // the run's smallest row
            bool fresh;
            qs = table_slot(w.qkey, w.mask, q, &fresh);
            atomicMax(&w.qfirst_inv[qs], 0xFFFFFFFFu - (unsigned)r);     // min row, kept inverted so that the zero fill means "none"
            atomicAdd(&w.qcnt[qs], run.len);
        }
    }
    qs = __shfl(qs, run.head);
    if (live) w.qslot[r] = qs;
}

// the scanned values of row r (non-zero only on the first row of a query): x = rows of the query, y = 1
__device__ __forceinline__ int4 cas_vals(const CasWs& w, int r, int n) {
    int4 v = make_int4(0, 0, 0, 0);
    if (r < n) {
        const int qs = w.qslot[r];
        if (qs >= 0 && 0xFFFFFFFFu - w.qfirst_inv[qs] == (unsigned)r) v = make_int4(w.qcnt[qs], 1, 0, 0);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_cas_scan_sums(int n, CasWs w) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) t = t + cas_vals(w, r0 + i, n);
    int4 total;
    block_scan(t, &total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive prefixes (in place); the number of queries -> status[2]
__global__ __launch_bounds__(256) void k_cas_scan_top(int nb, CasWs w, int* status) {
    const int4 total = scan_top(w.bsum, nb);
    if (threadIdx.x == 0) status[2] = total.y;
}

__global__ __launch_bounds__(256) void k_cas_scan_apply(int n, CasWs w, int* status) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 v[4];
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = cas_vals(w, r0 + i, n); t = t + v[i]; }
    int4 total;
    int4 pre = block_scan(t, &total) + w.bsum[blockIdx.x];
    int largest = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v[i].y) {                                     // first row of a query
            const int qs = w.qslot[r0 + i];
            w.qoff[qs] = pre.x;
            w.qsel[pre.y] = qs;                           // pre.y < distinct queries <= n
            largest = max(largest, v[i].x);
        }
        pre = pre + v[i];
    }
    if (largest) atomicMax(&status[3], largest);
}

__global__ __launch_bounds__(256) void k_cas_scatter(int n, CasWs w) {
    scatter_rows(n, w.qslot, w.qoff, w.qfill, w.qlist);
}

// one wavefront per query, wavefronts stride over the queries (their number is known on the device only); a lane owns rows x, x + 64, .. of the list
__global__ __launch_bounds__(256) void k_cas_mark(CasWs w, int keep, const int* status) {
    const int lane = threadIdx.x & 63;
    const int n_q = status[2];
    const int waves = gridDim.x * 4;
    for (int o = blockIdx.x * 4 + (threadIdx.x >> 6); o < n_q; o += waves) {
        const int qs = w.qsel[o];
        const int cnt = w.qcnt[qs], off = w.qoff[qs];
        for (int x = lane; x < cnt; x += 64) {
            const int r = w.qlist[off + x];
            int before = 0;
            if (cnt > keep) {
                const u64 e = w.enc[r];
                for (int y = 0; y < cnt && before < keep; ++y) {
                    const int r2 = w.qlist[off + y];
                    before += ranks_before(w.enc[r2], (unsigned)r2, e, (unsigned)r) ? 1 : 0;
                }
            }
            w.mark[r] = before < keep ? 1 : 0;
        }
    }
}

// The safe rule, same walk: a lane's row i is pruned iff at least k OTHER rows j of its list have lower(j) > upper(i), strictly, on the images; the count
// stops at k.  A query of at most k rows is kept without a comparison (there are fewer than k other rows).
__global__ __launch_bounds__(256) void k_cas_mark_safe(CasWs w, int k, const int* status) {
    const int lane = threadIdx.x & 63;
    const int n_q = status[2];
    const int waves = gridDim.x * 4;
    for (int o = blockIdx.x * 4 + (threadIdx.x >> 6); o < n_q; o += waves) {
        const int qs = w.qsel[o];
        const int cnt = w.qcnt[qs], off = w.qoff[qs];
        for (int x = lane; x < cnt; x += 64) {
            const int r = w.qlist[off + x];
            int above = 0;
            if (cnt > k) {
                const u64 up = w.enc_up[r];
                for (int y = 0; y < cnt && above < k; ++y) {
                    const int r2 = w.qlist[off + y];
                    above += (y != x && w.enc[r2] > up) ? 1 : 0;
                }
            }
            w.mark[r] = above < k ? 1 : 0;
        }
    }
}

// kept byte of row r: the mark, or 1 for every row under a flag (k_cas_insert has finished: the flag word is final)
__device__ __forceinline__ int cas_kept(const CasWs& w, int r, int n, int flags) { return r < n ? (flags ? 1 : w.mark[r]) : 0; }

__global__ __launch_bounds__(256) void k_cas_kept_sums(int n, CasWs w, const int* status, unsigned char* kept) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    const int flags = status[0];
    int t = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = cas_kept(w, r0 + i, n, flags);
        if (r0 + i < n) kept[r0 + i] = (unsigned char)k;
        t += k;
    }
    int total;
    block_scan(t, &total);
    if (threadIdx.x == 0) w.ksum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_cas_kept_top(int nb, CasWs w, int* status) {
    const int total = scan_top(w.ksum, nb);
    if (threadIdx.x == 0) status[1] = total;
}

__global__ __launch_bounds__(256) void k_cas_kept_apply(int n, CasWs w, const unsigned char* kept, int* list) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int k[4], t = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { k[i] = r0 + i < n ? kept[r0 + i] : 0; t += k[i]; }
    int total;
    int pre = block_scan(t, &total) + w.ksum[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (k[i]) list[pre] = r0 + i;                     // pre < kept rows <= n
        pre += k[i];
    }
}

// n > MMS_CASCADE_MAX_ROWS: every row kept, nothing ranked
__global__ __launch_bounds__(256) void k_cas_keep_all(long long n, unsigned char* kept, int* list, int* status) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) { kept[i] = 1; list[i] = (int)i; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { status[0] = MMS_CASCADE_FLAG_TOO_MANY; status[1] = (int)n; status[2] = 0; status[3] = 0; }
}

__global__ __launch_bounds__(256) void k_cascade_stage1(const float* probs, long long n, float* x) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) x[i] = probs[2 * i + 1];   // probs[:, 1]
}

// the expression of k_merge4 (batchops.hip), every product and sum rounded on its own
#pragma clang fp contract(off)
// thread t in two roles: t < n_kept scatters the second stage's scores of kept pair list[t] and merges it; t < n with kept[t] == 0 writes the pruned pair
__global__ __launch_bounds__(256) void k_cascade_merge(const float* p0, const float* p1, const float* p2, const int* list, const int* n_kept_dev,
                                                       const unsigned char* kept, const float* x, float w0, float w1, float w2, float w3,
                                                       float* merged, float* members, long long n) {
    const long long nk = *n_kept_dev;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
        if (t < nk) {
            const long long i = list[t];
            const float s0 = p0[2 * t + 1], s1 = p1[2 * t + 1], s2 = p2[2 * t + 1], s3 = x[i];
            merged[i] = ((w0 * s0 + w1 * s1) + w2 * s2) + w3 * s3;
            if (members) { members[i] = s0; members[n + i] = s1; members[2 * n + i] = s2; members[3 * n + i] = s3; }
        }
        if (!kept[t]) {
            const float z = 0.0f, s3 = x[t];
            merged[t] = ((w0 * z + w1 * z) + w2 * z) + w3 * s3;
            if (members) { members[t] = z; members[n + t] = z; members[2 * n + t] = z; members[3 * n + t] = s3; }
        }
    }
}

// ---- plans (mms_score_ensemble_plan): T is the [4][n] member table of the call, `list` the ascending original rows of the stage (nullptr: every row) ----

// pair t of the stage's batch -> row list[t] of T, for the members the stage computed (mask: 1 = both zk members, 2 = lds, 4 = lxmert); one more stage reached
__global__ __launch_bounds__(256) void k_plan_scatter(const float* p0, const float* p1, const float* p2, const float* p3, int members, const int* list,
                                                      long long n_stage, float* T, long long n, unsigned char* reached) {
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n_stage; t += (long long)gridDim.x * 256) {
        const long long i = list ? list[t] : t;
        if (members & 1) { T[i] = p0[2 * t + 1]; T[n + i] = p1[2 * t + 1]; }
        if (members & 2) T[2 * n + i] = p2[2 * t + 1];
        if (members & 4) T[3 * n + i] = p3[2 * t + 1];
        reached[i] = (unsigned char)(reached[i] + 1);                      // a row is in a stage's list once: no other thread touches reached[i]
    }
}

// the bounds of the stage's rows, dense by list position: lower = the merge of T as it stands, upper = the same with the members of `later` (a mask) at 1.0f
__global__ __launch_bounds__(256) void k_plan_bounds(const float* T, long long n, const int* list, long long n_stage, int later, float w0, float w1, float w2,
                                                     float w3, float* lower, float* upper) {
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n_stage; t += (long long)gridDim.x * 256) {
        const long long i = list ? list[t] : t;
        const float s0 = T[i], s1 = T[n + i], s2 = T[2 * n + i], s3 = T[3 * n + i];
        lower[t] = ((w0 * s0 + w1 * s1) + w2 * s2) + w3 * s3;
        if (!upper) continue;                                             // a keep stage reads the lower bound only
        const float u0 = (later & 1) ? 1.0f : s0, u1 = (later & 1) ? 1.0f : s1, u2 = (later & 2) ? 1.0f : s2, u3 = (later & 4) ? 1.0f : s3;
        upper[t] = ((w0 * u0 + w1 * u1) + w2 * u2) + w3 * u3;
    }
}

// merged = the merge of the final T; member_scores (optional) = T
__global__ __launch_bounds__(256) void k_plan_merge(const float* T, long long n, float w0, float w1, float w2, float w3, float* merged, float* members) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float s0 = T[i], s1 = T[n + i], s2 = T[2 * n + i], s3 = T[3 * n + i];
        merged[i] = ((w0 * s0 + w1 * s1) + w2 * s2) + w3 * s3;
        if (members) { members[i] = s0; members[n + i] = s1; members[2 * n + i] = s2; members[3 * n + i] = s3; }
    }
}

inline dim3 flat_grid(long long n) { long long g = (n + 255) / 256; return dim3((unsigned)(g < 1 ? 1 : (g > 65535 ? 65535 : g))); }

}  // namespace

long long cascade_workspace_bytes(long long n) { return n > MMS_CASCADE_MAX_ROWS ? 256 : (long long)cas_layout(nullptr, n).total_bytes; }

// the launches both selections share; `upper` == nullptr: the top-`keep` rule on `score`, else the safe rule on (score = lower, upper) with k = keep
static void cascade_select(const int64_t* group_ids, const float* score, const float* upper, long long n, int keep, uint8_t* kept, int32_t* kept_list,
                           int32_t* status, void* workspace, hipStream_t st) {
    if (n <= 0) { (void)hipMemsetAsync(status, 0, 16, st); return; }
    if (n > MMS_CASCADE_MAX_ROWS) {
        hipLaunchKernelGGL(k_cas_keep_all, flat_grid(n), dim3(256), 0, st, n, kept, kept_list, status);
        return;
    }
    (void)hipMemsetAsync(status, 0, 16, st);
    const int m = (int)n;
    const CasWs w = cas_layout(workspace, m, upper != nullptr);
    (void)hipMemsetAsync(w.qkey, 0xFF, w.ff_bytes, st);
    (void)hipMemsetAsync(w.qcnt, 0, w.zero_bytes, st);
    const dim3 block(256), rows((m + 255) / 256), scan((m + SCAN_ROWS - 1) / SCAN_ROWS);
    if (upper) hipLaunchKernelGGL(k_cas_insert<true>, rows, block, 0, st, (const long long*)group_ids, score, upper, m, w, status);
    else hipLaunchKernelGGL(k_cas_insert<false>, rows, block, 0, st, (const long long*)group_ids, score, upper, m, w, status);
    hipLaunchKernelGGL(k_cas_scan_sums, scan, block, 0, st, m, w);
    hipLaunchKernelGGL(k_cas_scan_top, dim3(1), block, 0, st, (int)scan.x, w, status);
    hipLaunchKernelGGL(k_cas_scan_apply, scan, block, 0, st, m, w, status);
    hipLaunchKernelGGL(k_cas_scatter, rows, block, 0, st, m, w);
    const int sel_blocks = (int)std::min<long long>(2048, ((long long)m + 3) / 4);
    if (upper) hipLaunchKernelGGL(k_cas_mark_safe, dim3(sel_blocks), block, 0, st, w, keep, status);
    else hipLaunchKernelGGL(k_cas_mark, dim3(sel_blocks), block, 0, st, w, keep, status);
    hipLaunchKernelGGL(k_cas_kept_sums, scan, block, 0, st, m, w, status, kept);
    hipLaunchKernelGGL(k_cas_kept_top, dim3(1), block, 0, st, (int)scan.x, w, status);
    hipLaunchKernelGGL(k_cas_kept_apply, scan, block, 0, st, m, w, kept, kept_list);
}

void launch_cascade_select(const int64_t* group_ids, const float* score, long long n, int keep, uint8_t* kept, int32_t* kept_list, int32_t* status,
                           void* workspace, hipStream_t st) {
    cascade_select(group_ids, score, nullptr, n, keep, kept, kept_list, status, workspace, st);
}

long long cascade_safe_workspace_bytes(long long n) { return n > MMS_CASCADE_MAX_ROWS ? 256 : (long long)cas_layout(nullptr, n, true).total_bytes; }

void launch_cascade_select_safe(const int64_t* group_ids, const float* lower, const float* upper, long long n, int k, uint8_t* kept, int32_t* kept_list,
                                int32_t* status, void* workspace, hipStream_t st) {
    cascade_select(group_ids, lower, upper, n, k, kept, kept_list, status, workspace, st);
}

void launch_cascade_stage1(const float* probs, long long n, float* x, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_cascade_stage1, flat_grid(n), dim3(256), 0, st, probs, n, x);
}

void launch_cascade_merge(const float* const probs3[3], const int* kept_list, const int* n_kept_dev, const uint8_t* kept, const float* x, const float w[4],
                          float* merged, float* members, long long n, hipStream_t st) {
    if (n > 0)
        hipLaunchKernelGGL(k_cascade_merge, flat_grid(n), dim3(256), 0, st, probs3[0], probs3[1], probs3[2], kept_list, n_kept_dev, kept, x, w[0], w[1], w[2],
                           w[3], merged, members, n);
}

void launch_plan_scatter(const float* const probs[4], int members, const int* list, long long n_stage, float* T, long long n, uint8_t* reached, hipStream_t st) {
    if (n_stage > 0)
        hipLaunchKernelGGL(k_plan_scatter, flat_grid(n_stage), dim3(256), 0, st, probs[0], probs[1], probs[2], probs[3], members, list, n_stage, T, n, reached);
}

void launch_plan_bounds(const float* T, long long n, const int* list, long long n_stage, int later, const float w[4], float* lower, float* upper, hipStream_t st) {
    if (n_stage > 0)
        hipLaunchKernelGGL(k_plan_bounds, flat_grid(n_stage), dim3(256), 0, st, T, n, list, n_stage, later, w[0], w[1], w[2], w[3], lower, upper);
}

void launch_plan_merge(const float* T, long long n, const float w[4], float* merged, float* members, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_plan_merge, flat_grid(n), dim3(256), 0, st, T, n, w[0], w[1], w[2], w[3], merged, members);
}
