// Fitting the ensemble weights on the valid set (mms_ndcg_weight_sweep, include/mmscore.h): the nDCG@k histogram -- and value -- of EVERY weight
// vector of a grid in one call.  For weight vector v and row r, with the M member scores member-major in fp32 (members[m * n + r], what
// mms_score_ensemble writes):
//     score_v[r] = (...((w[v][0] * s0) + w[v][1] * s1) + ...) + w[v][M - 1] * s_{M-1}
// in IEEE double, every product and every sum rounded on its own (code/main.py:59 as Python evaluates it) -- NO fused multiply-add: contraction
// is switched off for this file.  The outputs for v are by definition what mms_ndcg_at_k yields for score_f64 = score_v.
//
//   launch_ndcg_lists   stages 1-7 of ndcg.hip ONCE per call: key tables, per-row key index and relevance, scan, scatter (no score is read)
//   k_sweep_pack        the listed rows gathered in list order into contiguous records: the member scores padded with zeros to 4 or 8, and
//                       row << 1 | rel
//   k_sweep<K, MP>      a LANE owns a weight vector: a wavefront takes (key query i, tile of 64 weight vectors) and walks the query's packed rows
//                       serially.  The record's address is the same in all lanes: scalar loads, the next record requested while this one is
//                       ranked.  Each lane forms its own score_v[r] and inserts (score, row, rel) into a private top-K list in registers (K a
//                       template parameter: static indexing; K comparisons and selects, no data-dependent branch: TopK of rank_tables.h -- with 64 weight vectors per
//                       wavefront SOME lane inserts on most rows).  No cross-lane operation, no LDS for the ranking, 64 busy lanes whatever the
//                       rows per query -- the opposite decomposition to k_select (a lane per row), which would idle more than half a wavefront
//                       on the valid set's 9 - 30 rows per query and pay six shuffle steps per pick and per weight.
//                       Workgroups stride over (tile, slab of key queries) tasks (sweep_grid / sweep_task), the four waves of a workgroup over the slab's queries.
//                       Histogram, K <= 5 (64 x bins x 4 B <= 48 KiB): [bins][64] int32 counters in LDS per task (lane = bank: conflict-free;
//                       sweep_zero / sweep_flush), flushed with 64-bit global atomic adds of the non-zero counters; K >= 6: 64-bit global atomic adds directly.
//   k_sweep_value       value[v] = (sum over all bins in bin order of double(hist[v][b]) * bin_value[b]) / n_key_queries_total, each
//                       operation rounded on its own: ndcg.ndcg_from_hist bit for bit (an empty bin adds +0.0 to a non-negative sum).
// Integer atomics only, and the order inside a list cannot matter because the selection key (score with -0.0 == +0.0, row) is total: equal inputs give equal bytes.
#include "rank_tables.h"
#include "merge_members.h"

#pragma clang fp contract(off)

namespace {

constexpr int SWEEP_LDS_MAX_K = 5;       // (K + 1) << K bins x 64 lanes x 4 B: 48 KiB at K = 5

// One listed row as the hot loop streams it: the member scores (zero past the M-th), and row << 1 | rel.  MP = 4 (M <= 4) or 8: the record is
// 8 x MP bytes and aligned to its size, so a wavefront fetches it with one or two scalar loads.
template <int MP>
struct __attribute__((aligned(8 * MP))) SweepRec { float s[MP]; unsigned meta; unsigned pad[MP - 1]; };      // meta = row << 1 | rel

struct SweepWs { char* rec; size_t total_bytes; };

SweepWs sweep_layout(void* base, long long n, long long Qa, long long Tk, int M) {
    SweepWs s{};
    Carver cv{(char*)base, up256((size_t)ndcg_workspace_bytes(n, Qa, Tk))};
    cv.take(s.rec, (size_t)(n > 0 ? n : 1) * (size_t)member_mp(M) * 8);
    s.total_bytes = cv.o;
    return s;
}

// the listed rows (status[1] of them, at most n) in list order
template <int MP>
__global__ __launch_bounds__(256) void k_sweep_pack(const float* __restrict__ members, int M, int n, NdcgLists L, const int* __restrict__ status,
                                                    SweepRec<MP>* __restrict__ rec) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n || x >= status[1]) return;
    const int r = L.list[x];                                                 // inside [0, n): k_scatter wrote it
    SweepRec<MP> o{};
    load_members<MP>(members, M, n, r, o.s);
    o.meta = ((unsigned)r << 1) | (unsigned)L.rel[r];                       // r < 2^22
    rec[x] = o;
}

// The lists are ranked on the scores as doubles (ranks_before<double>), the merge of merge_members.h over the MP padded members.  A non-finite
// score is flagged, and with a flag the outputs are unspecified.  The kernel spells lane_weights() and merged() out, statement for statement:
// through the two functions the same loop measured 2 % slower at 176 851 weight vectors (profiles/rd17_fit_family_refactor.txt).
template <int K, int MP, bool LDS>
__global__ __launch_bounds__(256) void k_sweep(const double* __restrict__ weights, long long W, int M, int Qa, int slabs, long long tasks, NdcgLists L,
                                               const SweepRec<MP>* __restrict__ rec, u64* hist, int* status) {
    constexpr int BINS = (K + 1) << K;
    __shared__ int counters[LDS ? BINS * 64 : 1];                            // [bin][lane of the tile]
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (scalar: the query walk is wave-uniform)
    bool bad = false;
    for (long long t = blockIdx.x; t < tasks; t += gridDim.x) {
        const SweepTask task = sweep_task(t, slabs, Qa);
        const long long v = task.tile * 64 + lane;
        const bool live = v < W;
        double w[MP];
#pragma unroll
        for (int m = 0; m < MP; ++m) w[m] = (live && m < M) ? weights[v * M + m] : 0.0;
        if (LDS) sweep_zero<BINS>(counters);
        for (int i = task.q0 + wv; i < task.q1; i += 4) {                     // (i, cnt, off: the same in every lane of the wavefront)
            const int cnt = L.cnt[i];
            if (cnt == 0) continue;                                          // a key query without rows: no histogram entry
            const int off = L.off[i];
            TopK<K, double> top;                                             // the K best so far; an empty place: -inf
            top.clear(-__builtin_huge_val());
            const int end = off + cnt;
            SweepRec<MP> cur = rec[off];
            for (int x = off; x < end; ++x) {
                const SweepRec<MP> nxt = rec[min(x + 1, end - 1)];           // the next record is on its way while this one is ranked
                const unsigned meta = cur.meta;
                double s = w[0] * (double)cur.s[0];
#pragma unroll
                for (int m = 1; m < MP; ++m) {
                    const double prod = w[m] * (double)cur.s[m];
                    s = s + prod;
                }
                cur = nxt;
                bad |= live && !finite_score(s);
                top.insert(true, s, meta);
            }
            const unsigned bin = ((unsigned)min(max(L.distinct[i], 0), K) << K) | top.rel_mask();
            if (live) {
                if (LDS) atomicAdd(&counters[bin * 64 + lane], 1);
                else atomicAdd(&hist[(size_t)v * BINS + bin], 1ull);
            }
        }
        if (LDS) sweep_flush<BINS>(counters, task.tile, W, hist);
    }
    if (bad) atomicOr(&status[2], 2);
}

__global__ __launch_bounds__(256) void k_sweep_value(const u64* __restrict__ hist, const double* __restrict__ bin_value, long long W, int bins, double total,
                                                     double* __restrict__ value_out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= W) return;
    const u64* h = hist + (size_t)v * bins;
    double acc = 0.0;
    for (int b = 0; b < bins; ++b) {
        const double term = (double)(long long)h[b] * bin_value[b];
        acc = acc + term;
    }
    value_out[v] = acc / total;
}

template <int MP>
void launch_sweep_mp(hipStream_t st, const float* members, int M, int n, const double* weights, long long W, int k, int Qa, NdcgLists L, void* records,
                     u64* hist, int* status) {
    SweepRec<MP>* rec = (SweepRec<MP>*)records;
    hipLaunchKernelGGL((k_sweep_pack<MP>), dim3((n + 255) / 256), dim3(256), 0, st, members, M, n, L, (const int*)status, rec);
    const SweepGrid g = sweep_grid(W, Qa);
    with_k<MMS_NDCG_MAX_K>(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        hipLaunchKernelGGL((k_sweep<K, MP, K <= SWEEP_LDS_MAX_K>), dim3(g.grid), dim3(256), 0, st, weights, W, M, Qa, g.slabs, g.tasks, L, rec, hist, status);
    });
}

}  // namespace

long long ndcg_sweep_workspace_bytes(long long n, long long Qa, long long Tk, int M) { return (long long)sweep_layout(nullptr, n, Qa, Tk, M).total_bytes; }

void launch_ndcg_sweep(const int64_t* query_id, const int64_t* product_id, const float* members, int M, int n, const int64_t* key_query,
                       const int64_t* key_off, const int64_t* key_product, int Qa, int Tk, const double* weights, long long W, int k, int allow_missing,
                       const double* bin_value, long long n_key_queries_total, void* workspace, int64_t* hist_out, double* value_out, int32_t* status,
                       hipStream_t st) {
    const int bins = (k + 1) << k;
    if (W > 0) (void)hipMemsetAsync(hist_out, 0, (size_t)W * bins * 8, st);
    if (Qa <= 0) (void)hipMemsetAsync(status, 0, 16, st);                    // no key: no row belongs to a key query
    else {
        const NdcgLists L = launch_ndcg_lists(query_id, product_id, n, key_query, key_off, key_product, Qa, Tk, allow_missing, workspace, status, st);
        if (n > 0 && W > 0) {
            const SweepWs s = sweep_layout(workspace, n, Qa, Tk, M);
            if (member_mp(M) == 4) launch_sweep_mp<4>(st, members, M, n, weights, W, k, Qa, L, s.rec, (u64*)hist_out, status);
            else launch_sweep_mp<8>(st, members, M, n, weights, W, k, Qa, L, s.rec, (u64*)hist_out, status);
        }
    }
    if (value_out && W > 0) launch_hist_values(hist_out, bin_value, W, bins, n_key_queries_total, value_out, st);
}

void launch_hist_values(const int64_t* hist, const double* bin_value, long long n_hist, int bins, long long total, double* value_out, hipStream_t st) {
    hipLaunchKernelGGL(k_sweep_value, dim3((unsigned)((n_hist + 255) / 256)), dim3(256), 0, st, (const u64*)hist, bin_value, n_hist, bins, (double)total,
                       value_out);
}
