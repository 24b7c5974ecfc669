// The valid half of the job on the device (mms_key_relevance / mms_ndcg_at_k, include/mmscore.h): the 0/1 relevance of every (query, product) row
// against the answer key, and the nDCG@k decisions of ndcg.ndcg_from_arrays (code/imagebert_lds/src/evaluation.py:4-38) over three parallel
// arrays (query_id, product_id, score) -- a sibling of rank.hip: after scoring, handle-free, enqueue only, integer atomics only, no sort.
//
//   answer key in CSR form: key_query[Qa], key_off[Qa + 1], key_product[Tk]     (key query i owns key_product[key_off[i] .. key_off[i + 1]))
//   per key query i, over its rows in (score descending, row ascending) order -- Python's stable sorted(..., reverse=True):
//     mask  bit j set when the j-th ranked row's product is in the query's truth list (j < k)
//     ideal = min(distinct products of the truth list, k)                       (the host: len(set(truth)))
//     code[i] = mask | ideal << 8,  or -1 for a key query without rows;   hist[ideal << k | mask] += 1
//   The metric itself is host arithmetic on these integers (ndcg.ndcg_from_codes: the sequential sum of the host form, bit for bit;
//   ndcg.ndcg_from_hist: the same terms summed per bin, so it differs from the sequential sum by summation order only).
//
// Four fills (status, the histogram, the key tables to 0xFF, the counters to 0) and eight launches:
//   k_key_queries    key_query[i] -> i in an open-addressing table (capacity >= 2 Qa); a query that is already there raises flag bit 2
//   k_key_pairs      key_product[t] -> its slot in a product table, then the (key index, product slot) pair into a set (both capacity >= 2 Tk);
//                    distinct[i] counts the pairs that were new
//   k_rows           per row: key index of its query (looked up once per RUN of equal query ids inside a wavefront, wave_run), membership of
//                    (key index, product) in the set, score image, rows per key query (atomic add once per run)
//   k_scan_*         exclusive scan of the per-key row counts (block sums / top / apply; block_scan and scan_top of rank_tables.h): list offsets, the status totals
//   k_scatter        rows grouped by key query (counting sort by the offsets, scatter_rows; the order inside a list does not matter)
//   k_select         one wavefront per key query: k rounds of a wave-wide arg-max over (image, row) below the previous pick (wave_next), looping over
//                    the list when it is longer than a wavefront
// mms_key_relevance stops after k_scan_top (it needs the totals only).  No workgroup waits on another: the stages meet at kernel boundaries.
// The weight sweep (ndcg_sweep.hip, mms_ndcg_weight_sweep) runs everything up to k_scatter with no score (launch_ndcg_lists) and ranks the lists itself.
// The only atomics are integer add / or / compare-and-swap whose final memory value is independent of the arrival order, and the values they
// return (a table slot, a list position) never reach an output: equal inputs give bit-equal outputs.
#include "rank_tables.h"

namespace {

constexpr int SCAN_KEYS = 1024;                             // key queries per workgroup of the scan kernels: 256 threads x 4

struct NdcgWs {              // device workspace carved by ndcg_layout(): the 0xFF tables, the zero counters, then arrays written before they are read
    long long* kqkey; long long* pkey; long long* pairkey;                       // 0xFF: [capq], [capp], [capp]
    int* cnt; int* fill; int* distinct; int* missing;                            // 0: [Qa] x 3, [1]
    int* kqval;                                                                  // [capq] key index of a claimed slot
    int* off; int* bsum;                                                         // [Qa], [blocks of SCAN_KEYS]
    u64* enc; int* rowqi; int* list; unsigned char* rel;                         // [n]
    unsigned qmask, pmask;
    size_t ff_bytes, zero_bytes, total_bytes;
};

NdcgWs ndcg_layout(void* base, long long n, long long Qa, long long Tk) {
    NdcgWs w{};
    long long capq = 1024, capp = 1024;
    while (capq < 2 * Qa) capq <<= 1;
    while (capp < 2 * Tk) capp <<= 1;
    w.qmask = (unsigned)(capq - 1); w.pmask = (unsigned)(capp - 1);
    Carver cv{(char*)base, 0};
    const size_t r = (size_t)(n > 0 ? n : 1), a = (size_t)(Qa > 0 ? Qa : 1), nb = (a + SCAN_KEYS - 1) / SCAN_KEYS;
    cv.take(w.kqkey, (size_t)capq); cv.take(w.pkey, (size_t)capp); cv.take(w.pairkey, (size_t)capp);
    w.ff_bytes = cv.o;
    cv.take(w.cnt, a); cv.take(w.fill, a); cv.take(w.distinct, a); cv.take(w.missing, 1);
    w.zero_bytes = cv.o - w.ff_bytes;
    cv.take(w.kqval, (size_t)capq);
    cv.take(w.off, a); cv.take(w.bsum, nb);
    cv.take(w.enc, r); cv.take(w.rowqi, r); cv.take(w.list, r); cv.take(w.rel, r);
    w.total_bytes = cv.o;
    return w;
}

// slot of `key` in a table that is no longer written, or -1 (the walk ends at an empty slot: the table is at most half full)
__device__ __forceinline__ int table_find(const long long* keys, unsigned mask, long long key) {
    unsigned h = hash64((u64)key) & mask;
    for (;;) {
        const long long cur = keys[h];
        if (cur == key) return (int)h;
        if (cur == RANK_EMPTY) return -1;
        h = (h + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void k_key_queries(const long long* key_query, int Qa, NdcgWs w, int* status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Qa) return;
    const long long q = key_query[i];
    if (q == RANK_EMPTY) { atomicOr(&status[2], 8); return; }
    bool fresh;
    const int s = table_slot(w.kqkey, w.qmask, q, &fresh);
    if (fresh) w.kqval[s] = i;
    else atomicOr(&status[2], 4);                                            // this query is already in the key
}

__global__ __launch_bounds__(256) void k_key_pairs(const long long* key_off, const long long* key_product, int Qa, int Tk, NdcgWs w, int* status) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Tk) return;
    const long long p = key_product[t];
    if (p == RANK_EMPTY) { atomicOr(&status[2], 8); return; }
    int lo = 0, hi = Qa;                                                     // the last i in [0, Qa) with key_off[i] <= t (i stays inside whatever key_off holds)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (key_off[mid] <= (long long)t) lo = mid; else hi = mid;
    }
    bool fresh;
    const int ps = table_slot(w.pkey, w.pmask, p, &fresh);
    table_slot(w.pairkey, w.pmask, ((long long)lo << 32) | (long long)ps, &fresh);
    if (fresh) atomicAdd(&w.distinct[lo], 1);                                // a repeated truth product counts once
}

// S = float / double: the score's image is kept for k_select; score == nullptr (mms_key_relevance): no score is read
template <typename S>
__global__ __launch_bounds__(256) void k_rows(const long long* qid, const long long* pid, const S* score, int n, NdcgWs w, long long* labels_out,
                                              int* status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool live = r < n;
    long long q = 0, p = 0;
    if (live) {
        q = qid[r]; p = pid[r];
        int flags = 0;
        if (score) {
            const double s = (double)score[r];
            if (!finite_score(s)) flags |= 2;
            w.enc[r] = enc_score(s);
        }
        if (q == RANK_EMPTY || p == RANK_EMPTY) flags |= 8;
        if (flags) { atomicOr(&status[2], flags); live = false; }
    }
    const Run run = wave_run(q, live);
    const int lane = threadIdx.x & 63;
    int qi = -1;
    if (live && lane == run.head) {
        const int s = table_find(w.kqkey, w.qmask, q);
        if (s >= 0) {
            qi = w.kqval[s];
            atomicAdd(&w.cnt[qi], run.len);
        }
    }
    qi = __shfl(qi, run.head);
    if (!live) qi = -1;
    bool rel = false;
    if (qi >= 0) {
        const int ps = table_find(w.pkey, w.pmask, p);
        rel = ps >= 0 && table_find(w.pairkey, w.pmask, ((long long)qi << 32) | (long long)ps) >= 0;
    }
    if (r < n) {
        w.rowqi[r] = qi;
        w.rel[r] = rel ? 1 : 0;
        if (labels_out) labels_out[r] = rel ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_scan_sums(int Qa, NdcgWs w) {
    const int i0 = blockIdx.x * SCAN_KEYS + threadIdx.x * 4;
    int t = 0, miss = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < Qa) { const int c = w.cnt[i0 + j]; t += c; miss += c == 0; }
    }
    int total, mtotal;
    block_scan(t, &total);
    block_scan(miss, &mtotal);
    if (threadIdx.x == 0) {
        w.bsum[blockIdx.x] = total;
        if (mtotal) atomicAdd(w.missing, mtotal);
    }
}

// one workgroup: block sums -> exclusive prefixes (in place); the status totals
__global__ __launch_bounds__(256) void k_scan_top(int nb, int Qa, int allow_missing, NdcgWs w, int* status) {
    const int total = scan_top(w.bsum, nb);
    if (threadIdx.x == 0) {
        const int miss = *w.missing;
        status[0] = Qa - miss; status[1] = total; status[3] = miss;
        if (miss && !allow_missing) atomicOr(&status[2], 1);
    }
}

__global__ __launch_bounds__(256) void k_scan_apply(int Qa, NdcgWs w) {
    const int i0 = blockIdx.x * SCAN_KEYS + threadIdx.x * 4;
    int v[4], t = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = i0 + j < Qa ? w.cnt[i0 + j] : 0; t += v[j]; }
    int total;
    int pre = block_scan(t, &total) + w.bsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < Qa) w.off[i0 + j] = pre;
        pre += v[j];
    }
}

__global__ __launch_bounds__(256) void k_scatter(int n, NdcgWs w) {
    scatter_rows(n, w.rowqi, w.off, w.fill, w.list);
}

// one wavefront per key query, wavefronts stride over the key
__global__ __launch_bounds__(256) void k_select(const long long* pid, int Qa, int k, NdcgWs w, int* out_code, long long* out_topk, u64* hist) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < Qa; i += waves) {
        const int cnt = w.cnt[i], off = w.off[i];
        Pick prev{~0ull, 0};                              // previous pick: every image is below ~0
        unsigned mask = 0;
        for (int j = 0; j < k; ++j) {
            const Pick b = wave_next(cnt, prev, [&](int x) {             // (image descending, row ascending)
                const int r = w.list[off + x];
                return Pick{w.enc[r], (unsigned)r};
            });
            long long prod = -1;                          // exhausted: prev stays, so the remaining rounds find nothing either and write -1
            if (b.img != 0) { prod = pid[b.tie]; mask |= (unsigned)w.rel[b.tie] << j; prev = b; }
            if (out_topk && lane == 0) out_topk[(long long)i * k + j] = prod;
        }
        if (lane == 0) {
            const int ideal = min(max(w.distinct[i], 0), k);
            out_code[i] = cnt ? (int)(mask | ((unsigned)ideal << 8)) : -1;
            if (cnt) atomicAdd(&hist[((unsigned)ideal << k) | mask], 1ull);
        }
    }
}

}  // namespace

long long ndcg_workspace_bytes(long long n, long long Qa, long long Tk) { return (long long)ndcg_layout(nullptr, n, Qa, Tk).total_bytes; }

namespace {
// stages 1-7 (key tables, per-row key index and relevance, scan; with `lists` also list offsets and scatter): everything that reads no ranking.
// score_f32 == score_f64 == nullptr: no score is read and no image is written.
NdcgWs ndcg_stages(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n, const int64_t* key_query,
                   const int64_t* key_off, const int64_t* key_product, int Qa, int Tk, int allow_missing, void* workspace, int64_t* labels_out, bool lists,
                   int32_t* status, hipStream_t st) {
    const NdcgWs w = ndcg_layout(workspace, n, Qa, Tk);
    (void)hipMemsetAsync(w.kqkey, 0xFF, w.ff_bytes, st);
    (void)hipMemsetAsync(w.cnt, 0, w.zero_bytes, st);
    const dim3 block(256), rows((n + 255) / 256), keys((Qa + 255) / 256), scan((Qa + SCAN_KEYS - 1) / SCAN_KEYS);
    const long long* q = (const long long*)query_id;
    const long long* p = (const long long*)product_id;
    hipLaunchKernelGGL(k_key_queries, keys, block, 0, st, (const long long*)key_query, Qa, w, status);
    if (Tk > 0) hipLaunchKernelGGL(k_key_pairs, dim3((Tk + 255) / 256), block, 0, st, (const long long*)key_off, (const long long*)key_product, Qa, Tk, w, status);
    if (n > 0) {
        if (score_f64) hipLaunchKernelGGL((k_rows<double>), rows, block, 0, st, q, p, score_f64, n, w, (long long*)labels_out, status);
        else hipLaunchKernelGGL((k_rows<float>), rows, block, 0, st, q, p, score_f32, n, w, (long long*)labels_out, status);
    }
    hipLaunchKernelGGL(k_scan_sums, scan, block, 0, st, Qa, w);
    hipLaunchKernelGGL(k_scan_top, dim3(1), block, 0, st, (int)scan.x, Qa, allow_missing, w, status);
    if (!lists) return w;                                                    // mms_key_relevance: labels and totals only
    hipLaunchKernelGGL(k_scan_apply, scan, block, 0, st, Qa, w);
    if (n > 0) hipLaunchKernelGGL(k_scatter, rows, block, 0, st, n, w);
    return w;
}
}  // namespace

void launch_ndcg(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n, const int64_t* key_query,
                 const int64_t* key_off, const int64_t* key_product, int Qa, int Tk, int k, int allow_missing, void* workspace, int64_t* labels_out,
                 int32_t* out_code, int64_t* out_topk, int64_t* hist, int32_t* status, hipStream_t st) {
    (void)hipMemsetAsync(status, 0, 16, st);
    if (hist) (void)hipMemsetAsync(hist, 0, ((size_t)(k + 1) << k) * 8, st);
    if (Qa <= 0) {                                                           // no key: no row belongs to a key query
        if (labels_out && n > 0) (void)hipMemsetAsync(labels_out, 0, (size_t)n * 8, st);
        return;
    }
    const NdcgWs w = ndcg_stages(query_id, product_id, score_f32, score_f64, n, key_query, key_off, key_product, Qa, Tk, allow_missing, workspace, labels_out,
                                 out_code != nullptr, status, st);
    if (!out_code) return;
    const int sel_blocks = (int)std::min<long long>(2048, ((long long)Qa + 3) / 4);
    hipLaunchKernelGGL(k_select, dim3(sel_blocks), dim3(256), 0, st, (const long long*)product_id, Qa, k, w, out_code, (long long*)out_topk, (u64*)hist);
}

NdcgLists launch_ndcg_lists(const int64_t* query_id, const int64_t* product_id, int n, const int64_t* key_query, const int64_t* key_off,
                            const int64_t* key_product, int Qa, int Tk, int allow_missing, void* workspace, int32_t* status, hipStream_t st) {
    (void)hipMemsetAsync(status, 0, 16, st);
    const NdcgWs w = ndcg_stages(query_id, product_id, nullptr, nullptr, n, key_query, key_off, key_product, Qa, Tk, allow_missing, workspace, nullptr, true,
                                 status, st);
    return NdcgLists{w.cnt, w.off, w.distinct, w.list, w.rel};
}
