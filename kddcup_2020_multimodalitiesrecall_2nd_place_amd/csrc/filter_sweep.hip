// Fitting the uniqueness filter on the valid set (mms_filter_sweep, include/mmscore.h): the nDCG@k histogram -- and value, and codes -- of the SUBMISSION rows
// (code/main.py:76-104: filter, >= 5 survivors / 1..4 fallback / dropped query) for EVERY (gap, tie) pair of a grid in one call.  Per filter the outputs
// are by definition what ndcg.submission_codes yields on the host: ensemble.submission_rows graded against the answer key.
//
//   per product over ALL rows (also rows of queries outside the key):  d = best - second (two rows at the maximum: 0; one row: +inf)
//   survive(row) = not (d < gap) and |s - best| < tie                  in IEEE double on the scores widened exactly, -0.0 == +0.0
//   key query with >= 5 survivors: its best survivors; with 1..4: its best rows overall; with none: code -2, no histogram entry
//   order: score descending, then row ascending
//
// Nothing but the two comparisons above depends on the filter, so everything else runs ONCE per call:
//   launch_ndcg_lists    stages 1-7 of ndcg.hip: key tables, per-row key index and relevance, scan, scatter (no score is read)
//   launch_rank_stats    k_rank_insert / k_rank_second of rank.hip: score images, best / rows at best / max of the rest / rows per product, the
//                        repeated-pair, non-finite and reserved-id flags (into a status block of its own)
//   k_filter_pack        the listed rows in list order as 32-byte records: image, row << 1 | rel, d, e = |s - best|; thread 0 folds the rank flags into status[2]
//   k_filter_unfiltered  one wavefront per key query: the relevance mask of its K best rows overall (k_select's rounds: wave_next of rank_tables.h) -- the 1..4-survivor answer is
//                        the same for every filter, so it is computed once per CALL
//   k_filter_sweep<K>    a LANE owns a filter: a wavefront takes (key query i, tile of 64 filters) and walks the query's records serially (ndcg_sweep.hip's
//                        decomposition).  The record's address is the same in all lanes: scalar loads, the next record requested while this one is
//                        ranked.  Each lane decides survive on the record's d and e against its own (gap, tie), counts its survivors and inserts them
//                        into a private top-K list in registers (static indexing, K comparisons and selects; the inserts themselves are selects, not branches).  At the end the
//                        lane takes its survivor list (>= 5), the unfiltered mask (1..4) or code -2 (0).
//                        Workgroups stride over (tile, slab of key queries) tasks (sweep_grid / sweep_task); histogram (sweep_zero / sweep_flush): [bins][64] int32 counters in LDS per task (lane = bank),
//                        flushed with 64-bit global atomic adds of the non-zero counters.
//   launch_hist_values   value[g] = (sum over all bins in bin order of double(hist[g][b]) * bin_value[b]) / n_key_queries_total (ndcg_sweep.hip)
// Integer atomics only, and the order inside a list cannot matter because the selection key (image, row) is total: equal inputs give equal bytes.
// No kernel waits on another workgroup.
#include "rank_tables.h"

#pragma clang fp contract(off)

namespace {

// One listed row as the hot loop streams it; aligned to its size: a wavefront fetches it with one scalar load.
struct __attribute__((aligned(32))) FilterRec { u64 img; unsigned meta; unsigned pad; double d; double e; };      // meta = row << 1 | rel

struct FilterWs { char* rank; int* rstatus; FilterRec* rec; int* umask; size_t total_bytes; };

FilterWs filter_layout(void* base, long long n, long long Qa, long long Tk) {
    FilterWs f{};
    Carver cv{(char*)base, up256((size_t)ndcg_workspace_bytes(n, Qa, Tk))};
    cv.take(f.rank, (size_t)rank_workspace_bytes(n));
    cv.take(f.rstatus, 4);
    cv.take(f.rec, (size_t)(n > 0 ? n : 1));
    cv.take(f.umask, (size_t)(Qa > 0 ? Qa : 1));
    f.total_bytes = cv.o;
    return f;
}

// the listed rows (status[1] of them, at most n) in list order
__global__ __launch_bounds__(256) void k_filter_pack(int n, NdcgLists L, RankStats S, const int* __restrict__ rstatus, int* status, FilterRec* __restrict__ rec) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x == 0) {                                                            // flags of the product statistics: every row counts, listed or not
        const int t = sweep_flags_of_rank(rstatus[2]);
        if (t) atomicOr(&status[2], t);
    }
    if (x >= n || x >= status[1]) return;
    const int r = L.list[x];                                                 // inside [0, n): k_scatter wrote it
    const int ps = S.pslot[r];
    FilterRec o;
    o.img = S.enc[r];
    o.meta = ((unsigned)r << 1) | (unsigned)L.rel[r];                       // r < 2^22
    o.pad = 0;
    o.d = __builtin_huge_val();
    o.e = __builtin_huge_val();                                              // a flagged row (no product slot) survives nothing
    if (ps >= 0) {
        const double best = dec_score(S.best[ps]);
        if (S.cnt[ps] >= 2) {
            const double second = S.bcnt[ps] >= 2 ? best : dec_score(S.rest[ps]);
            o.d = best - second;
        }
        o.e = fabs(dec_score(o.img) - best);
    }
    rec[x] = o;
}

// one wavefront per key query, wavefronts stride over the key: umask[i] = relevance bits of the K best rows of ALL its rows
__global__ __launch_bounds__(256) void k_filter_unfiltered(int Qa, int K, NdcgLists L, const FilterRec* __restrict__ rec, int* __restrict__ umask) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < Qa; i += waves) {
        const int cnt = L.cnt[i], off = L.off[i];
        Pick prev{~0ull, 0};                              // previous pick: every image is below ~0
        unsigned mask = 0;
        for (int j = 0; j < K; ++j) {
            const Pick b = wave_next(cnt, prev, [&](int x) { return Pick{rec[off + x].img, rec[off + x].meta}; });
            if (b.img == 0) break;                        // exhausted: the remaining places carry relevance 0
            mask |= (b.tie & 1u) << j;
            prev = b;
        }
        if (lane == 0) umask[i] = (int)mask;
    }
}

template <int K>
__global__ __launch_bounds__(256) void k_filter_sweep(const double* __restrict__ filters, long long G, int Qa, int slabs, long long tasks, NdcgLists L,
                                                      const FilterRec* __restrict__ rec, const int* __restrict__ umask, u64* hist, int* code_out) {
    constexpr int BINS = (K + 1) << K;
    __shared__ int counters[BINS * 64];                                      // [bin][lane of the tile]
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (scalar: the query walk is wave-uniform)
    for (long long t = blockIdx.x; t < tasks; t += gridDim.x) {
        const SweepTask task = sweep_task(t, slabs, Qa);
        const long long g = task.tile * 64 + lane;
        const bool live = g < G;
        const double gap = live ? filters[g * 2] : 0.0, tie = live ? filters[g * 2 + 1] : 0.0;
        sweep_zero<BINS>(counters);
        for (int i = task.q0 + wv; i < task.q1; i += 4) {                     // (i, cnt, off: the same in every lane of the wavefront)
            const int cnt = L.cnt[i];
            if (cnt == 0) {                                                  // a key query without rows: no histogram entry
                if (code_out && live) code_out[(size_t)g * Qa + i] = -1;
                continue;
            }
            const int off = L.off[i];
            u64 E[K];                                                        // the K best survivors so far, best first; an empty place: image 0, relevance 0
            unsigned R[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { E[j] = 0; R[j] = 0xFFFFFFFEu; }
            int ns = 0;
            const int end = off + cnt;
            FilterRec cur = rec[off];
            for (int x = off; x < end; ++x) {
                const FilterRec nxt = rec[min(x + 1, end - 1)];              // the next record is on its way while this one is ranked
                const u64 img = cur.img;
                const unsigned meta = cur.meta;
                const bool sv = !(cur.d < gap) && cur.e < tie;
                cur = nxt;
                ns += sv ? 1 : 0;
                // TopK::insert's steps, written here: through the shared template this loop compiles branch-free instead of to the exec regions it
                // was measured with (profiles/rd13_rank_family_refactor.txt).  c[j] = this survivor ranks before place j (monotone in j)
                bool c[K];
#pragma unroll
                for (int j = 0; j < K; ++j) c[j] = sv && ranks_before(img, meta, E[j], R[j]);
#pragma unroll
                for (int j = K - 1; j >= 1; --j) {
                    E[j] = c[j - 1] ? E[j - 1] : (c[j] ? img : E[j]);
                    R[j] = c[j - 1] ? R[j - 1] : (c[j] ? meta : R[j]);
                }
                E[0] = c[0] ? img : E[0];
                R[0] = c[0] ? meta : R[0];
            }
            unsigned mask = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) mask |= (R[j] & 1u) << j;
            if (ns < 5) mask = (unsigned)umask[i];                           // 1..4 survivors: the best rows overall
            const unsigned ideal = (unsigned)min(max(L.distinct[i], 0), K);
            if (live) {
                if (ns > 0) atomicAdd(&counters[((ideal << K) | mask) * 64 + lane], 1);
                if (code_out) code_out[(size_t)g * Qa + i] = ns > 0 ? (int)(mask | (ideal << 8)) : -2;
            }
        }
        sweep_flush<BINS>(counters, task.tile, G, hist);
    }
}

}  // namespace

long long filter_sweep_workspace_bytes(long long n, long long Qa, long long Tk) { return (long long)filter_layout(nullptr, n, Qa, Tk).total_bytes; }

void launch_filter_sweep(const int64_t* query_id, const int64_t* product_id, const float* score_f32, const double* score_f64, int n,
                         const int64_t* key_query, const int64_t* key_off, const int64_t* key_product, int Qa, int Tk, const double* filters, long long G,
                         int k, int allow_missing, const double* bin_value, long long n_key_queries_total, void* workspace, int64_t* hist_out,
                         double* value_out, int32_t* code_out, int32_t* status, hipStream_t st) {
    const int bins = (k + 1) << k;
    if (G > 0) (void)hipMemsetAsync(hist_out, 0, (size_t)G * bins * 8, st);
    if (Qa <= 0) (void)hipMemsetAsync(status, 0, 16, st);                    // no key: no row belongs to a key query
    else {
        const NdcgLists L = launch_ndcg_lists(query_id, product_id, n, key_query, key_off, key_product, Qa, Tk, allow_missing, workspace, status, st);
        if (n <= 0) {
            if (code_out && G > 0) (void)hipMemsetAsync(code_out, 0xFF, (size_t)G * Qa * 4, st);      // every key query is without rows: -1
        } else {
            const FilterWs f = filter_layout(workspace, n, Qa, Tk);
            const RankStats S = launch_rank_stats(query_id, product_id, score_f32, score_f64, n, f.rank, f.rstatus, st);
            hipLaunchKernelGGL(k_filter_pack, dim3((n + 255) / 256), dim3(256), 0, st, n, L, S, (const int*)f.rstatus, status, f.rec);
            if (G > 0) {
                const int sel_blocks = (int)std::min<long long>(2048, ((long long)Qa + 3) / 4);
                hipLaunchKernelGGL(k_filter_unfiltered, dim3(sel_blocks), dim3(256), 0, st, Qa, k, L, (const FilterRec*)f.rec, f.umask);
                const SweepGrid sg = sweep_grid(G, Qa);
                with_k<MMS_FILTER_MAX_K>(k, [&](auto kc) {
                    hipLaunchKernelGGL((k_filter_sweep<decltype(kc)::value>), dim3(sg.grid), dim3(256), 0, st, filters, G, Qa, sg.slabs, sg.tasks, L,
                                       (const FilterRec*)f.rec, (const int*)f.umask, (u64*)hist_out, code_out);
                });
            }
        }
    }
    if (value_out && G > 0) launch_hist_values(hist_out, bin_value, G, bins, n_key_queries_total, value_out, st);
}
