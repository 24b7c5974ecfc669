// Per-query normalisation of the member scores on the device (mms_normalize_members, include/mmscore.h): every member of a [M, n] score block is
// put on a common per-query scale -- min-max, z-score or rank --, value for value what ensemble.normalize_members computes on the host.
//
//   a group = the rows of one query id (any order, not adjacent); x_r = (double)members[m][r] + 0.0; IEEE double, one rounding to fp32 at the end
//
// The front is cascade.hip's (a query table, counts, one scan for the list offsets, scatter_rows), then the lists are put in order and walked.  Three
// fills (the key table to 0xFF, the value tables and the status to 0) and seven launches:
//   k_nrm_insert      row -> slot of its query (table_slot once per wave_run); rows per query (atomic add), first row per query (atomic max of
//                     the inverted row); flags over ALL members of the row
//   k_nrm_scan_*      exclusive scan over the rows of "rows of the query" / "is a first row", non-zero on a query's first row only -> list
//                     offsets, the number of queries, the largest query (block_scan / scan_top of rank_tables.h)
//   k_nrm_scatter     rows grouped by query (scatter_rows): the order inside a list is ARBITRARY, it depends on which wavefront's atomic arrives first
//   k_nrm_order       ... so it never leaves this kernel: a thread owns a list entry and counts the entries of its list with a smaller row
//                     (a counting walk, rows are distinct) -> the list in ascending row order
//   k_nrm_apply       a thread owns one output element (list entry x member) and walks its query's ordered list serially: minimum / maximum,
//                     the two sequential sums of the z-score in ascending row order, or the count of strictly greater rows; then the transform.
//                     Adjacent lanes own adjacent entries of one list, so the walk's loads are wave-wide broadcasts.  The statistics are
//                     recomputed per row instead of once per (query, member): rows x rows-of-the-query steps, ~30 x the minimum on the valid
//                     set's lists and still below the launch overhead (profiles/rd20_normalize.txt), for two kernels and a table less.
// Under a flag k_nrm_order and k_nrm_apply return at once (the lists then do not cover every row): `out` is left as it was.
// The only atomics are integer add / max / or / compare-and-swap whose final memory value is independent of the arrival order, and the values
// they return (a list position in k_nrm_scatter) never reach the output: equal inputs give equal bytes.
#include "rank_tables.h"

namespace {

constexpr int SCAN_ROWS = 1024;                             // rows per workgroup of the scan kernels: 256 threads x 4

struct NrmWs {               // device workspace carved by nrm_layout(); [cap] tables first (the 0xFF part, then the zero part), [n] arrays after
    long long* qkey;                                                             // 0xFF
    int* qcnt; int* qfill; unsigned* qfirst_inv;                                 // 0
    int* qoff;                                                                   // written before read
    int* qslot; int* qlist; int* qorder; int4* bsum;
    unsigned mask; int cap;
    size_t ff_bytes, zero_bytes, total_bytes;
};

NrmWs nrm_layout(void* base, long long n) {
    NrmWs w{};
    const int cap = rank_table_slots(n);
    w.cap = cap; w.mask = (unsigned)(cap - 1);
    Carver cv{(char*)base, 0};
    const size_t c = (size_t)cap, r = (size_t)(n > 0 ? n : 1), nb = (r + SCAN_ROWS - 1) / SCAN_ROWS;
    cv.take(w.qkey, c);
    w.ff_bytes = cv.o;
    cv.take(w.qcnt, c); cv.take(w.qfill, c); cv.take(w.qfirst_inv, c);
    w.zero_bytes = cv.o - w.ff_bytes;
    cv.take(w.qoff, c);
    cv.take(w.qslot, r); cv.take(w.qlist, r); cv.take(w.qorder, r);
    cv.take(w.bsum, nb);
    w.total_bytes = cv.o;
    return w;
}

__global__ __launch_bounds__(256) void k_nrm_insert(const long long* qid, const float* members, int n_members, int n, NrmWs w, int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool live = r < n;
    long long q = 0;
    if (live) {
        q = qid[r];
        int flags = 0;
        for (int m = 0; m < n_members; ++m)
            if (!finite_score((double)members[(size_t)m * n + r])) flags |= MMS_NORMALIZE_FLAG_NONFINITE;
        if (q == RANK_EMPTY) flags |= MMS_NORMALIZE_FLAG_RESERVED_ID;
        if (flags) { atomicOr(&status[2], flags); live = false; w.qslot[r] = -1; }
    }
    const Run run = wave_run(q, live);
    const int lane = threadIdx.x & 63;
    int qs = -1;
    if (live && lane == run.head) {                                      // the run's smallest row
        bool fresh;
        qs = table_slot(w.qkey, w.mask, q, &fresh);
        atomicMax(&w.qfirst_inv[qs], 0xFFFFFFFFu - (unsigned)r);         // min row, kept inverted so that the zero fill means "none"
        atomicAdd(&w.qcnt[qs], run.len);
    }
    qs = __shfl(qs, run.head);
    if (live) w.qslot[r] = qs;
}

// the scanned values of row r (non-zero only on the first row of a query): x = rows of the query, y = 1
__device__ __forceinline__ int4 nrm_vals(const NrmWs& w, int r, int n) {
    int4 v = make_int4(0, 0, 0, 0);
    if (r < n) {
        const int qs = w.qslot[r];
        if (qs >= 0 && 0xFFFFFFFFu - w.qfirst_inv[qs] == (unsigned)r) v = make_int4(w.qcnt[qs], 1, 0, 0);
    }
    return v;
}

__global__ __launch_bounds__(256) void k_nrm_scan_sums(int n, NrmWs w) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) t = t + nrm_vals(w, r0 + i, n);
    int4 total;
    block_scan(t, &total);
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive prefixes (in place); the number of queries -> status[0]
__global__ __launch_bounds__(256) void k_nrm_scan_top(int nb, NrmWs w, int* status) {
    const int4 total = scan_top(w.bsum, nb);
    if (threadIdx.x == 0) status[0] = total.y;
}

__global__ __launch_bounds__(256) void k_nrm_scan_apply(int n, NrmWs w, int* status) {
    const int r0 = blockIdx.x * SCAN_ROWS + threadIdx.x * 4;
    int4 v[4];
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = nrm_vals(w, r0 + i, n); t = t + v[i]; }
    int4 total;
    int4 pre = block_scan(t, &total) + w.bsum[blockIdx.x];
    int largest = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v[i].y) {                                     // first row of a query: its list starts at pre.x, and pre.x + its rows <= live rows <= n
            w.qoff[w.qslot[r0 + i]] = pre.x;
            largest = max(largest, v[i].x);
        }
        pre = pre + v[i];
    }
    if (largest) atomicMax(&status[1], largest);
}

__global__ __launch_bounds__(256) void k_nrm_scatter(int n, NrmWs w) {
    scatter_rows(n, w.qslot, w.qoff, w.qfill, w.qlist);
}

// Without a flag every row is live: the lists tile qlist[0 .. n), entry x belongs to the list of its row's query, [off, off + cnt) lies inside [0, n),
// and a row's place among the cnt distinct rows of its list is below cnt.  (k_nrm_insert has finished: the flag word is final.)
__global__ __launch_bounds__(256) void k_nrm_order(int n, NrmWs w, const int* status) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n || status[2] != 0) return;
    const int r = w.qlist[x];
    const int qs = w.qslot[r];
    const int cnt = w.qcnt[qs], off = w.qoff[qs];
    int before = 0;
    for (int y = 0; y < cnt; ++y) before += w.qlist[off + y] < r ? 1 : 0;
    w.qorder[off + before] = r;
}

// the arithmetic that defines the result: every operation rounded on its own
#pragma clang fp contract(off)
// thread (x, member blockIdx.y): entry x of the ordered lists; the walk runs over the whole list in ascending row order
template <int MODE>
__global__ __launch_bounds__(256) void k_nrm_apply(const float* members, int n, NrmWs w, float* out, const int* status) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n || status[2] != 0) return;
    const int r = w.qorder[x];
    const int qs = w.qslot[r];
    const int cnt = w.qcnt[qs];
    const int* list = w.qorder + w.qoff[qs];
    const float* mem = members + (size_t)blockIdx.y * n;
    const double v = (double)mem[r] + 0.0;                // fp32 -> fp64 is exact; + 0.0 folds -0.0 onto +0.0
    double res = 0.0;
    if (MODE == MMS_NORMALIZE_MINMAX) {
        double lo = v, hi = v;
        for (int y = 0; y < cnt; ++y) {
            const double s = (double)mem[list[y]] + 0.0;
            lo = s < lo ? s : lo;
            hi = s > hi ? s : hi;
        }
        if (hi != lo) res = (v - lo) / (hi - lo);
    } else if (MODE == MMS_NORMALIZE_ZSCORE) {
        double s1 = 0.0;
        for (int y = 0; y < cnt; ++y) s1 = s1 + ((double)mem[list[y]] + 0.0);
        const double mean = s1 / (double)cnt;
        double s2 = 0.0;
        for (int y = 0; y < cnt; ++y) {
            const double d = ((double)mem[list[y]] + 0.0) - mean;
            s2 = s2 + d * d;
        }
        const double sd = sqrt(s2 / (double)cnt);
        if (sd > 0.0) res = (v - mean) / sd;
    } else {
        int greater = 0;
        for (int y = 0; y < cnt; ++y) greater += ((double)mem[list[y]] + 0.0) > v ? 1 : 0;
        if (cnt > 1) res = (double)(cnt - 1 - greater) / (double)(cnt - 1);
    }
    out[(size_t)blockIdx.y * n + r] = (float)res;
}

}  // namespace

long long normalize_workspace_bytes(long long n, int /*n_members*/) { return (long long)nrm_layout(nullptr, n).total_bytes; }

void launch_normalize_members(const int64_t* query_id, const float* members, int n_members, long long n, int mode, float* out, int32_t* status,
                              void* workspace, hipStream_t st) {
    (void)hipMemsetAsync(status, 0, 16, st);
    if (n <= 0) return;
    if (mode == MMS_NORMALIZE_NONE) {
        (void)hipMemcpyAsync(out, members, (size_t)n * n_members * sizeof(float), hipMemcpyDeviceToDevice, st);
        return;
    }
    const int m = (int)n;
    const NrmWs w = nrm_layout(workspace, m);
    (void)hipMemsetAsync(w.qkey, 0xFF, w.ff_bytes, st);
    (void)hipMemsetAsync(w.qcnt, 0, w.zero_bytes, st);
    const dim3 block(256), rows((m + 255) / 256), scan((m + SCAN_ROWS - 1) / SCAN_ROWS), cells(rows.x, n_members);
    hipLaunchKernelGGL(k_nrm_insert, rows, block, 0, st, (const long long*)query_id, members, n_members, m, w, status);
    hipLaunchKernelGGL(k_nrm_scan_sums, scan, block, 0, st, m, w);
    hipLaunchKernelGGL(k_nrm_scan_top, dim3(1), block, 0, st, (int)scan.x, w, status);
    hipLaunchKernelGGL(k_nrm_scan_apply, scan, block, 0, st, m, w, status);
    hipLaunchKernelGGL(k_nrm_scatter, rows, block, 0, st, m, w);
    hipLaunchKernelGGL(k_nrm_order, rows, block, 0, st, m, w, status);
    if (mode == MMS_NORMALIZE_MINMAX) hipLaunchKernelGGL(k_nrm_apply<MMS_NORMALIZE_MINMAX>, cells, block, 0, st, members, m, w, out, status);
    else if (mode == MMS_NORMALIZE_ZSCORE) hipLaunchKernelGGL(k_nrm_apply<MMS_NORMALIZE_ZSCORE>, cells, block, 0, st, members, m, w, out, status);
    else hipLaunchKernelGGL(k_nrm_apply<MMS_NORMALIZE_RANK>, cells, block, 0, st, members, m, w, out, status);
}
