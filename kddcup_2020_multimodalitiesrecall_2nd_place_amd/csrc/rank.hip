// Submission ranking on the device (mms_rank_submission, include/mmscore.h): the global product-uniqueness filter and the per-query
// top-5 of code/main.py:64-104 over three parallel arrays (query_id, product_id, score), decision for decision what
// ensemble.submission_rows computes on the host with numpy sorts.
//
//   per product, over all rows:  best, second = 2nd entry of the descending score list (two rows at the maximum: second == best)
//   keep_product = rows of the product < 2  or  not (best - second < gap)
//   survive(row) = keep_product and |s - best| < tie
//   query with >= 5 survivors: its 5 best survivors; with 1..4: the 5 best of ALL its rows; with none: no output row
//   order inside a row: score descending, equal scores in row order; output rows: the >= 5 class first, then the 1..4 class, each in
//   the order of the queries' first appearance.
//
// No sort: every comparison is done on an order-preserving 64-bit integer image of the score as a double (-0.0 folded onto +0.0, as
// IEEE == does), so "best" is an integer atomic max and the selection key (image descending, row ascending) is total.  Three fills (status, the key tables to 0xFF, the value tables to 0) and eight launches:
//   k_rank_insert    row -> slot of its product / its query in two open-addressing tables (capacity >= 2 n); best image per product
//                    (64-bit atomic max), rows per product / per query (atomic add), first row per query (atomic min)
//   k_rank_second    per product: rows equal to best (count), max image of the others; the (query slot, product slot) pair goes into a
//                    third table -- a pair that is already there raises flag bit 0
//   k_rank_survive   second, keep_product, survive per row; survivors per query
//   k_rank_scan_*    one exclusive scan over the rows of four per-row values that are non-zero on a query's FIRST row only: "class >= 5",
//                    "class 1..4", "rows of the query", "is a first row" -> output position, list offset, counts (block sums / top / apply; block_scan and scan_top of rank_tables.h)
//   k_rank_scatter   rows grouped by query (counting sort by the offsets above, scatter_rows; the order inside a list does not matter)
//   k_rank_select    one wavefront per output row: five rounds of a wave-wide arg-max over (image, row) below the previous pick (wave_next)
// The only atomics are integer max / min / add / or / compare-and-swap whose final memory value is independent of the arrival order, and
// the values they return (a list position in k_rank_scatter) never reach the output: equal inputs give bit-equal outputs.
// Rows of one query are mostly adjacent, so the query-side atomics are issued once per RUN of equal query ids inside a wavefront
// (wave_run): ~30x fewer operations on the few hot slots than one per row.
#include "rank_tables.h"

namespace {

constexpr int SCAN_ROWS = 1024;                             // rows per workgroup of the scan kernels: 256 threads x 4

struct RankWs {              // device workspace carved by rank_layout(); [cap] tables first (the 0xFF part, then the zero part), [n] arrays after
    long long* pkey; long long* qkey; long long* pairkey;                       // 0xFF
    u64* pbest; u64* prest; int* pcnt; int* pbcnt; int* qcnt; int* qsurv; int* qfill; unsigned* qfirst_inv;   // 0
    int* qoff;                                                                   // written before read
    u64* enc; int* pslot; int* qslot; int* qlist; int* qsel; int4* bsum; unsigned char* surv;
    int* hdr;                                                                    // [4]: total of the four scanned values
    unsigned mask; int cap;
    size_t ff_bytes, zero_bytes, total_bytes;
};

}  // namespace

int rank_table_slots(long long n) {
    int cap = 1024;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}

namespace {

RankWs rank_layout(void* base, long long n) {
    RankWs w{};
    const int cap = rank_table_slots(n);
    w.cap = cap; w.mask = (unsigned)(cap - 1);
    Carver cv{(char*)base, 0};
    const size_t c = (size_t)cap, r = (size_t)(n > 0 ? n : 1), nb = (r + SCAN_ROWS - 1) / SCAN_ROWS;
    cv.take(w.pkey, c); cv.take(w.qkey, c); cv.take(w.pairkey, c);
    w.ff_bytes = cv.o;
    cv.take(w.pbest, c); cv.take(w.prest, c);
    cv.take(w.pcnt, c); cv.take(w.pbcnt, c); cv.take(w.qcnt, c); cv.take(w.qsurv, c); cv.take(w.qfill, c);
    cv.take(w.qfirst_inv, c);
    w.zero_bytes = cv.o - w.ff_bytes;
    cv.take(w.qoff, c);
    cv.take(w.enc, r); cv.take(w.pslot, r); cv.take(w.qslot, r); cv.take(w.qlist, r); cv.take(w.qsel, r);
    cv.take(w.bsum, nb); cv.take(w.surv, r);
    cv.take(w.hdr, 4);
    w.total_bytes = cv.o;
    return w;
}

template <typename S>
__global__ __launch_bounds__(256) void k_rank_insert(const long long* qid, const long long* pid, const S* score, int n, RankWs w, int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool live = r < n;
    long long q = 0, p = 0;
    double s = 0.0;
    if (live) {
        q = qid[r]; p = pid[r]; s = (double)score[r];
        int flags = 0;
        if (!finite_score(s)) flags |= 2;
        if (q == RANK_EMPTY || p == RANK_EMPTY) flags |= 8;
        if (flags) { atomicOr(&status[2], flags); live = false; w.pslot[r] = -1; w.qslot[r] = -1; }
    }
    const Run run = wave_run(q, live);
    const int lane = threadIdx.x & 63;
    int qs = -1;
    if (live) {
        const u64 e = enc_score(s);
        bool fresh;
        const int ps = table_slot(w.pkey, w.mask, p, &fresh);
        atomicMax(&w.pbest[ps], e);
        atomicAdd(&w.pcnt[ps], 1);
        w.enc[r] = e; w.pslot[r] = ps;
        if (lane == run.head) {                                          // the run's smallest row
            qs = table_slot(w.qkey, w.mask, q, &fresh);
            atomicMax(&w.qfirst_inv[qs], 0xFFFFFFFFu - (unsigned)r);     // min row, kept inverted so that the zero fill means "none"
            atomicAdd(&w.qcnt[qs], run.len);
        }
    }
    qs = __shfl(qs, run.head);
    if (live) w.qslot[r] = qs;
}

__global__ __launch_bounds__(256) void k_rank_second(int n, RankWs w, int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int ps = w.pslot[r];
    if (ps < 0) return;
    const u64 e = w.enc[r];
    if (e == w.pbest[ps]) atomicAdd(&w.pbcnt[ps], 1);
    else atomicMax(&w.prest[ps], e);
    bool fresh;
    table_slot(w.pairkey, w.mask, ((long long)w.qslot[r] << 32) | (long long)ps, &fresh);
    if (!fresh) atomicOr(&status[2], 1);                                 // this (query, product) pair was already in the table
}

__global__ __launch_bounds__(256) void k_rank_survive(int n, RankWs w, double gap, double tie) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int ps = r < n ? w.pslot[r] : -1;
    const bool live = ps >= 0;
    const int qs = live ? w.qslot[r] : -1;
    bool sv = false;
    if (live) {
        const double best = dec_score(w.pbest[ps]);
        bool keep = true;
        if (w.pcnt[ps] >= 2) {
            const double second = w.pbcnt[ps] >= 2 ? best : dec_score(w.prest[ps]);
            keep = !(best - second < gap);
        }
        sv = keep && fabs(dec_score(w.enc[r]) - best) < tie;
        w.surv[r] = sv ? 1 : 0;
    }
    const Run run = wave_run((long long)qs, live);
    const int lane = threadIdx.x & 63;
    const u64 svm = __ballot(sv);
    if (live && lane == run.head) {
        const u64 m = run.len >= 64 ? ~0ull : (((1ull << run.len) - 1) << run.head);
        const int c = __popcll(svm & m);
        if (c) atomicAdd(&w.qsurv[qs], c);
    }
}

// the four scanned values of row r (non-zero only on the first row of a query)
__device__ __forceinline__ int4 scan_vals(const RankWs& w, int r, int n) {
    int4 v = make_int4(0, 0, 0, 0);
    if (r < n) {
        const int qs = w.qslot[r];
        if (qs >= 0 && 0xFFFFFFFFu - w.qfirst_inv[qs] == (unsigned)r) {
            const int sv = w.qsurv[qs];
            v = make_int4(sv >= 5, sv >= 1 && sv < 5, w.qcnt[qs], 1);
        }
    }
    return v;
}

__global__ __launch_bounds__(256) void k_rank_scan_sums(int n, RankWs w) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) t = t + scan_vals(w, r0 + i, n);
    int4 total;
    block_scan(t, &total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive prefixes (in place), totals -> hdr and status
__global__ __launch_bounds__(256) void k_rank_scan_top(int nb, RankWs w, int max_queries, int* status) {
    const int4 total = scan_top(w.bsum, nb);
    if (threadIdx.x == 0) {
        w.hdr[0] = total.x; w.hdr[1] = total.y; w.hdr[2] = total.z; w.hdr[3] = total.w;
        status[0] = total.x + total.y; status[1] = total.x; status[3] = total.w;
        if (total.x + total.y > max_queries) atomicOr(&status[2], 4);
    }
}

__global__ __launch_bounds__(256) void k_rank_scan_apply(const long long* qid, int n, RankWs w, int max_queries, long long* out_query) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 v[4];
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = scan_vals(w, r0 + i, n); t = t + v[i]; }
    int4 total;
    int4 pre = block_scan(t, &total) + w.bsum[blockIdx.x];
    const int n_ge5 = w.hdr[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v[i].w) {                                     // first row of a query
            const int qs = w.qslot[r0 + i];
            const int pos = v[i].x ? pre.x : (v[i].y ? n_ge5 + pre.y : -1);
            w.qoff[qs] = pre.z;
            if (pos >= 0) {
                w.qsel[pos] = qs;                         // pos < distinct queries <= n
                if (pos < max_queries) out_query[pos] = qid[r0 + i];
            }
        }
        pre = pre + v[i];
    }
}

__global__ __launch_bounds__(256) void k_rank_scatter(int n, RankWs w) {
    scatter_rows(n, w.qslot, w.qoff, w.qfill, w.qlist);
}

// one wavefront per output row, wavefronts stride over the rows (the row count is known on the device only)
__global__ __launch_bounds__(256) void k_rank_select(const long long* pid, RankWs w, int max_queries, const int* status, long long* out_products,
                                                    int* out_count) {
    const int lane = threadIdx.x & 63;
    const int n_out = min(status[0], max_queries);
    const int waves = gridDim.x * 4;
    for (int o = blockIdx.x * 4 + (threadIdx.x >> 6); o < n_out; o += waves) {
        const int qs = w.qsel[o];
        const int cnt = w.qcnt[qs], off = w.qoff[qs];
        const bool filtered = w.qsurv[qs] >= 5;
        Pick prev{~0ull, 0};                              // previous pick: every image is below ~0
        int picked = 0;
        for (int k = 0; k < 5; ++k) {
            const Pick b = wave_next(cnt, prev, [&](int i) {             // (image descending, row ascending) over the survivors / all rows
                const int r = w.qlist[off + i];
                return Pick{filtered && !w.surv[r] ? 0 : w.enc[r], (unsigned)r};
            });
            long long prod = -1;                          // exhausted: prev stays, so the remaining rounds find nothing either and write -1
            if (b.img != 0) { prod = pid[b.tie]; prev = b; ++picked; }
            if (lane == 0) out_products[(long long)o * 5 + k] = prod;
        }
        if (lane == 0) out_count[o] = picked;
    }
}

}  // namespace

long long rank_workspace_bytes(long long n) { return (long long)rank_layout(nullptr, n).total_bytes; }

namespace {
// the status fill, the two table fills and k_rank_insert / k_rank_second: everything that does not depend on (gap, tie).  n > 0.
RankWs rank_stages(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n, void* workspace,
                   int32_t* status, hipStream_t st) {
    const RankWs w = rank_layout(workspace, n);
    (void)hipMemsetAsync(w.pkey, 0xFF, w.ff_bytes, st);
    (void)hipMemsetAsync(w.pbest, 0, w.zero_bytes, st);
    const dim3 block(256), rows((n + 255) / 256);
    const long long* q = (const long long*)query_id;
    const long long* p = (const long long*)product_id;
    if (score_f32) hipLaunchKernelGGL((k_rank_insert<float>), rows, block, 0, st, q, p, score_f32, n, w, status);
    else hipLaunchKernelGGL((k_rank_insert<double>), rows, block, 0, st, q, p, score_f64, n, w, status);
    hipLaunchKernelGGL(k_rank_second, rows, block, 0, st, n, w, status);
    return w;
}
}  // namespace

void launch_rank_submission(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n, double gap,
                            double tie, void* workspace, int max_queries, int64_t* out_query, int64_t* out_products, int32_t* out_count,
                            int32_t* status, hipStream_t st) {
    (void)hipMemsetAsync(status, 0, 16, st);
    if (n <= 0) return;
    const RankWs w = rank_stages(query_id, product_id, score_f32, score_f64, n, workspace, status, st);
    const dim3 block(256), rows((n + 255) / 256), scan((n + SCAN_ROWS - 1) / SCAN_ROWS);
    const long long* q = (const long long*)query_id;
    const long long* p = (const long long*)product_id;
    hipLaunchKernelGGL(k_rank_survive, rows, block, 0, st, n, w, gap, tie);
    hipLaunchKernelGGL(k_rank_scan_sums, scan, block, 0, st, n, w);
    hipLaunchKernelGGL(k_rank_scan_top, dim3(1), block, 0, st, (int)scan.x, w, max_queries, status);
    hipLaunchKernelGGL(k_rank_scan_apply, scan, block, 0, st, q, n, w, max_queries, (long long*)out_query);
    hipLaunchKernelGGL(k_rank_scatter, rows, block, 0, st, n, w);
    const int sel_blocks = (int)std::min<long long>(2048, ((long long)n + 3) / 4);
    hipLaunchKernelGGL(k_rank_select, dim3(sel_blocks), block, 0, st, p, w, max_queries, status, (long long*)out_products, out_count);
}

RankStats launch_rank_stats(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n, void* workspace,
                            int32_t* status, hipStream_t st) {
    (void)hipMemsetAsync(status, 0, 16, st);
    const RankWs w = rank_stages(query_id, product_id, score_f32, score_f64, n, workspace, status, st);
    return RankStats{w.enc, w.pslot, w.pbest, w.prest, w.pcnt, w.pbcnt};
}
