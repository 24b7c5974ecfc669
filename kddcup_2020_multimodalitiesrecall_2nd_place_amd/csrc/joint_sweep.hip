// Fitting the ensemble weights and the uniqueness filter JOINTLY on the valid set (mms_joint_sweep, include/mmscore.h): the nDCG@k histogram -- and
// value -- of the SUBMISSION rows for EVERY (weight vector, filter) pair of two grids in one call.  No new arithmetic: item (v, g) is by definition
// what mms_filter_sweep yields for filter g on score_f64 = score_v, the merge of mms_ndcg_weight_sweep for weight vector v
//     score_v[r] = (...((w[v][0] * s0) + w[v][1] * s1) + ...) + w[v][M - 1] * s_{M-1}       IEEE double, no fused multiply-add (contraction is off)
//     per product over ALL rows:  d = best - second (two rows at the maximum: best - best; one row: +inf)
//     survive(row) = not (d < gap) and |score_v - best| < tie;  >= 5 survivors: the best survivors; 1..4: the best rows overall; none: no entry
//     order: score descending, then row ascending, -0.0 == +0.0
// The filter's product statistics move with the weights, so they are formed PER WEIGHT VECTOR; everything that reads no score runs once per call.
//
// once per call
//   launch_ndcg_lists    stages 1-7 of ndcg.hip: key tables, per-row key index and relevance, scan, scatter
//   launch_rank_stats    k_rank_insert / k_rank_second of rank.hip on member 0: per row its product slot, the rows per product, the repeated-pair,
//                        reserved-id (and member 0's non-finite) flags into a status block of its own; its score statistics are not used
//   k_joint_scan_*       exclusive scan over the product table's slots of (rows, slot in use): list offset and DENSE index per product (block_scan / scan_top)
//   k_joint_scatter      rows grouped by product (scatter_rows)
//   k_joint_pack_p       the member scores in product-list order (MemRec<MP>: MP = 4 or 8 floats, zero past the M-th)
//   k_joint_pack_q       the key queries' rows in list order: members, row << 1 | rel, dense product index (JointRec<MP>); thread 0 folds the rank flags into status[2]
// per chunk of weight tiles (a tile = 64 weight vectors, one per lane; the chunk is what the caller's workspace holds)
//   k_joint_stats<MP>    a wavefront takes (product, tile) and walks the product's records serially (wave-uniform address: scalar loads, the next record in
//                        flight); each lane merges its own score and keeps best / rows at best / max of the rest by IEEE comparisons, then writes
//                        (best, d) to stats[tile][product][lane]: 16 B per lane, contiguous per wavefront.  A non-finite merged score of ANY row: flag bit 1
//   k_joint_unfiltered<K, MP>   k_sweep's walk with the relevance mask of the unfiltered top-K STORED ([tile][key query][lane], one byte) instead of binned: the
//                        1..4-survivor answer, the same for every filter
//   k_joint_sweep<K, MP> a task is (tile, filter, slab of key queries): the lane owns the weight vector, the filter is wave-uniform.  Walks the key query's
//                        records serially, re-forms the lane's merged score with merged() -- the statement sequence of k_joint_stats, so s - best is
//                        exact for the best row --, loads (best, d) of the record's product one record ahead, decides, counts survivors and inserts them
//                        into a register top-K (TopK::insert's steps written out: selects, no branch on the lane's decision).  Histogram: [bins][64] LDS counters per task (sweep_zero), flushed with 64-bit
//                        global atomic adds to item v * G + g (sweep_flush_strided)
//   launch_hist_values   value[v][g] of the chunk's histograms (ndcg_sweep.hip)
// Integer atomics only, and the order inside a list cannot matter because the selection key (score with -0.0 == +0.0, row) is total and best / rows at best /
// rest are order-free: equal inputs give equal bytes, whatever the chunk size.  No kernel waits on another workgroup.
#include "rank_tables.h"
#include "merge_members.h"

#pragma clang fp contract(off)

namespace {

constexpr int SCAN_SLOTS = 1024;                            // table slots per workgroup of the scan kernels: 256 threads x 4

// the member scores of one row (zero past the M-th), aligned to their size: one scalar load
template <int MP>
struct __attribute__((aligned(4 * MP))) MemRec { float s[MP]; };
// one listed row of a key query: members, row << 1 | rel, the dense index of its product (-1: a flagged row without a product slot)
template <int MP>
struct __attribute__((aligned(32))) JointRec { float s[MP]; unsigned meta; int prod; unsigned pad[MP == 4 ? 2 : 6]; };
// per (tile, product, lane)
struct __attribute__((aligned(16))) BestD { double best; double d; };

static_assert(sizeof(MemRec<4>) == 16 && sizeof(MemRec<8>) == 32 && sizeof(JointRec<4>) == 32 && sizeof(JointRec<8>) == 64 && sizeof(BestD) == 16, "joint_layout sizes the records");

struct JointWs {
    char* rank; int* rstatus;
    int* pfill;                                             // [cap] 0
    int* poff; int* pdense;                                 // [cap] written for the slots in use
    int4* bsum; int* hdr;                                   // hdr[0] = rows with a product slot, hdr[1] = products
    int* plist; int* pd_off; int* pd_cnt;                   // [n]; pd_*: per DENSE product
    char* prec; char* qrec;                                 // [n] MemRec / JointRec
    char* tiles;                                            // per tile of the chunk, tile_bytes apart: BestD [n][64], at umask_off unsigned char [Qa][64];
                                                            // without hist_out the chunk's histograms follow the last tile
    int cap;
    size_t fixed_bytes, tile_bytes, umask_off;
};

JointWs joint_layout(void* base, long long n, long long Qa, long long Tk, int M) {
    JointWs j{};
    j.cap = rank_table_slots(n);
    const size_t c = (size_t)j.cap, r = (size_t)(n > 0 ? n : 1), mp = (size_t)member_mp(M);
    Carver cv{(char*)base, up256((size_t)ndcg_workspace_bytes(n, Qa, Tk))};
    cv.take(j.rank, (size_t)rank_workspace_bytes(n));
    cv.take(j.rstatus, 4);
    cv.take(j.pfill, c); cv.take(j.poff, c); cv.take(j.pdense, c);
    cv.take(j.bsum, c / SCAN_SLOTS); cv.take(j.hdr, 4);
    cv.take(j.plist, r); cv.take(j.pd_off, r); cv.take(j.pd_cnt, r);
    cv.take(j.prec, r * mp * 4); cv.take(j.qrec, r * (mp == 4 ? 32 : 64));
    j.fixed_bytes = cv.o;
    j.tiles = (char*)base + cv.o;
    j.umask_off = up256(r * 64 * sizeof(BestD));
    j.tile_bytes = j.umask_off + up256((size_t)(Qa > 0 ? Qa : 1) * 64);
    return j;
}
inline size_t joint_tile_hist_bytes(long long G, int k) { return up256((size_t)64 * (size_t)G * (size_t)((k + 1) << k) * 8); }

// ---- once per call: product row lists ----

__device__ __forceinline__ int4 slot_vals(const int* cnt, int s) { const int c = cnt[s]; return make_int4(c, c > 0, 0, 0); }

__global__ __launch_bounds__(256) void k_joint_scan_sums(const int* __restrict__ cnt, int4* __restrict__ bsum) {
    const int s0 = blockIdx.x * SCAN_SLOTS + threadIdx.x * 4;            // (the table's capacity is a multiple of SCAN_SLOTS)
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) t = t + slot_vals(cnt, s0 + i);
    int4 total;
    block_scan(t, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_joint_scan_top(int nb, int4* bsum, int* __restrict__ hdr) {
    const int4 total = scan_top(bsum, nb);
    if (threadIdx.x == 0) { hdr[0] = total.x; hdr[1] = total.y; hdr[2] = 0; hdr[3] = 0; }
}

__global__ __launch_bounds__(256) void k_joint_scan_apply(const int* __restrict__ cnt, const int4* __restrict__ bsum, int* __restrict__ poff,
                                                          int* __restrict__ pdense, int* __restrict__ pd_off, int* __restrict__ pd_cnt) {
    const int s0 = blockIdx.x * SCAN_SLOTS + threadIdx.x * 4;
    int4 v[4];
    int4 t = make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = slot_vals(cnt, s0 + i); t = t + v[i]; }
    int4 total;
    int4 pre = block_scan(t, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (v[i].y) {                                                    // a product: pre.y < products <= n, pre.x + its rows <= n
            poff[s0 + i] = pre.x; pdense[s0 + i] = pre.y;
            pd_off[pre.y] = pre.x; pd_cnt[pre.y] = v[i].x;
        }
        pre = pre + v[i];
    }
}

__global__ __launch_bounds__(256) void k_joint_scatter(int n, const int* pslot, const int* poff, int* pfill, int* plist) {
    scatter_rows(n, pslot, poff, pfill, plist);
}

// the rows that have a product slot (hdr[0] of them, at most n) in product-list order
template <int MP>
__global__ __launch_bounds__(256) void k_joint_pack_p(const float* __restrict__ members, int M, int n, const int* __restrict__ plist, const int* __restrict__ hdr,
                                                      MemRec<MP>* __restrict__ prec) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= n || x >= hdr[0]) return;
    const int r = plist[x];                                                  // inside [0, n): k_joint_scatter wrote it
    MemRec<MP> o;
    load_members<MP>(members, M, n, r, o.s);
    prec[x] = o;
}

// the listed rows (status[1] of them, at most n) in key-query-list order
template <int MP>
__global__ __launch_bounds__(256) void k_joint_pack_q(const float* __restrict__ members, int M, int n, NdcgLists L, const int* __restrict__ pslot,
                                                      const int* __restrict__ pdense, const int* __restrict__ rstatus, int* status, JointRec<MP>* __restrict__ qrec) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x == 0) {                                                            // flags of the product statistics: every row counts, listed or not
        const int t = sweep_flags_of_rank(rstatus[2]);
        if (t) atomicOr(&status[2], t);
    }
    if (x >= n || x >= status[1]) return;
    const int r = L.list[x];                                                 // inside [0, n): k_scatter wrote it
    const int ps = pslot[r];
    JointRec<MP> o{};
    load_members<MP>(members, M, n, r, o.s);
    o.meta = ((unsigned)r << 1) | (unsigned)L.rel[r];                       // r < 2^22
    o.prod = ps >= 0 ? pdense[ps] : -1;
    qrec[x] = o;
}

// ---- per chunk of weight tiles ----

// wavefronts stride over (tile of the chunk, product) tasks; hdr[1] products (known on the device only)
template <int MP>
__global__ __launch_bounds__(256) void k_joint_stats(const double* __restrict__ weights, long long W, int M, long long tile0, int tiles, const int* __restrict__ hdr,
                                                     const int* __restrict__ pd_off, const int* __restrict__ pd_cnt, const MemRec<MP>* __restrict__ prec,
                                                     BestD* __restrict__ stats, size_t tile_stride, int* status) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (scalar: the product walk is wave-uniform)
    const int P = hdr[1];
    const long long tasks = (long long)P * tiles, waves = (long long)gridDim.x * 4;
    bool bad = false;
    for (long long t = (long long)blockIdx.x * 4 + wv; t < tasks; t += waves) {
        const int tl = (int)(t / P), pr = (int)(t - (long long)tl * P);
        const long long v = (tile0 + tl) * 64 + lane;
        const bool live = v < W;
        double w[MP];
        lane_weights<MP>(weights, v, live, M, w);
        const int off = pd_off[pr], cnt = pd_cnt[pr], end = off + cnt;      // cnt >= 1
        double best = -__builtin_huge_val(), rest = -__builtin_huge_val();
        int nbest = 0;
        MemRec<MP> cur = prec[off];
        for (int x = off; x < end; ++x) {
            const MemRec<MP> nxt = prec[min(x + 1, end - 1)];                // the next record is on its way while this one is merged
            const double s = merged<MP>(w, cur.s);
            cur = nxt;
            bad |= live && !finite_score(s);
            const bool gt = s > best, eq = s == best;
            rest = gt ? best : ((!eq && s > rest) ? s : rest);
            nbest = gt ? 1 : nbest + (eq ? 1 : 0);
            best = gt ? s : best;
        }
        BestD o;
        o.best = best;
        o.d = cnt < 2 ? __builtin_huge_val() : (nbest >= 2 ? best - best : best - rest);
        *(BestD*)((char*)stats + (size_t)tl * tile_stride + ((size_t)pr * 64 + lane) * sizeof(BestD)) = o;
    }
    if (bad) atomicOr(&status[2], 2);
}

// tasks (tile of the chunk, slab of key queries): umask[tile][i][lane] = relevance bits of the K best rows of ALL rows of key query i for the lane's vector
template <int K, int MP>
__global__ __launch_bounds__(256) void k_joint_unfiltered(const double* __restrict__ weights, long long W, int M, long long tile0, int Qa, int slabs, long long tasks,
                                                          NdcgLists L, const JointRec<MP>* __restrict__ rec, unsigned char* __restrict__ umask, size_t tile_stride) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (long long t = blockIdx.x; t < tasks; t += gridDim.x) {
        const SweepTask task = sweep_task(t, slabs, Qa);
        const long long v = (tile0 + task.tile) * 64 + lane;
        double w[MP];
        lane_weights<MP>(weights, v, v < W, M, w);
        unsigned char* um = umask + (size_t)task.tile * tile_stride + lane;
        for (int i = task.q0 + wv; i < task.q1; i += 4) {
            const int cnt = L.cnt[i];
            if (cnt == 0) continue;
            const int off = L.off[i], end = off + cnt;
            TopK<K, double> top;
            top.clear(-__builtin_huge_val());
            JointRec<MP> cur = rec[off];
            for (int x = off; x < end; ++x) {
                const JointRec<MP> nxt = rec[min(x + 1, end - 1)];
                const unsigned meta = cur.meta;
                const double s = merged<MP>(w, cur.s);
                cur = nxt;
                top.insert(true, s, meta);
            }
            um[(size_t)i * 64] = (unsigned char)top.rel_mask();
        }
    }
}

__device__ __forceinline__ BestD load_stats(const BestD* st, int prod) { return st[(size_t)max(prod, 0) * 64]; }

// tasks (unit = tile of the chunk x filter, slab of key queries); hist: the chunk's histograms, item (tile * 64 + lane) * G + g
template <int K, int MP>
__global__ __launch_bounds__(256) void k_joint_sweep(const double* __restrict__ weights, long long W, int M, const double* __restrict__ filters, int G, long long tile0,
                                                     int Qa, int slabs, long long tasks, NdcgLists L, const JointRec<MP>* __restrict__ rec,
                                                     const char* __restrict__ tiles, size_t tile_stride, size_t umask_off, u64* hist,
                                                     unsigned char* __restrict__ code_out, long long Wp) {
    constexpr int BINS = (K + 1) << K;
    __shared__ int counters[BINS * 64];                                      // [bin][lane of the tile]
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (scalar: the query walk is wave-uniform)
    for (long long t = blockIdx.x; t < tasks; t += gridDim.x) {
        const SweepTask task = sweep_task(t, slabs, Qa);                     // task.tile: the unit
        const int tl = (int)(task.tile / G), g = (int)(task.tile - (long long)tl * G);
        const long long v = (tile0 + tl) * 64 + lane;
        const bool live = v < W;
        double w[MP];
        lane_weights<MP>(weights, v, live, M, w);
        const double gap = filters[2 * g], tie = filters[2 * g + 1];
        const BestD* st = (const BestD*)(tiles + (size_t)tl * tile_stride) + lane;
        const unsigned char* um = (const unsigned char*)(tiles + (size_t)tl * tile_stride + umask_off) + lane;
        // the byte codes of (filter g, key query i) for the tile's 64 vectors: one aligned 64-byte line (v < Wp, a multiple of 64: lanes past W write
        // bytes that are never read); nullptr: no codes are kept (a wave-uniform branch)
        unsigned char* cd = code_out ? code_out + (size_t)g * Qa * Wp + v : nullptr;
        sweep_zero<BINS>(counters);
        for (int i = task.q0 + wv; i < task.q1; i += 4) {                     // (i, cnt, off: the same in every lane of the wavefront)
            const int cnt = L.cnt[i];
            if (cnt == 0) continue;                                          // a key query without rows: no histogram entry
            const int off = L.off[i], end = off + cnt;
            double E[K];                                                     // the K best survivors so far, best first; an empty place: -inf, relevance 0
            unsigned R[K];
#pragma unroll
            for (int j = 0; j < K; ++j) { E[j] = -__builtin_huge_val(); R[j] = 0xFFFFFFFEu; }
            int ns = 0;
            JointRec<MP> cur = rec[off];
            JointRec<MP> nxt = rec[min(off + 1, end - 1)];
            BestD bd = load_stats(st, cur.prod);
            for (int x = off; x < end; ++x) {
                const JointRec<MP> nx2 = rec[min(x + 2, end - 1)];           // two records ahead, so that the next record's statistics are requested
                const BestD bdn = load_stats(st, nxt.prod);                  // while this one is ranked
                const unsigned meta = cur.meta;
                const double s = merged<MP>(w, cur.s);
                const bool sv = cur.prod >= 0 && !(bd.d < gap) && fabs(s - bd.best) < tie;
                cur = nxt; nxt = nx2; bd = bdn;
                ns += sv ? 1 : 0;
                // TopK::insert's steps, written here as in k_filter_sweep, with `&` / `|` on the comparisons: no branch on the lane's decision.
                // c[j] = this survivor ranks before place j (monotone in j)
                bool c[K];
#pragma unroll
                for (int j = 0; j < K; ++j) c[j] = sv & ((s > E[j]) | ((s == E[j]) & (meta < R[j])));
#pragma unroll
                for (int j = K - 1; j >= 1; --j) {
                    E[j] = c[j - 1] ? E[j - 1] : (c[j] ? s : E[j]);
                    R[j] = c[j - 1] ? R[j - 1] : (c[j] ? meta : R[j]);
                }
                E[0] = c[0] ? s : E[0];
                R[0] = c[0] ? meta : R[0];
            }
            unsigned mask = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) mask |= (R[j] & 1u) << j;
            if (ns < 5) mask = um[(size_t)i * 64];                           // 1..4 survivors: the best rows overall
            const unsigned ideal = (unsigned)min(max(L.distinct[i], 0), K);
            if (live && ns > 0) atomicAdd(&counters[((ideal << K) | mask) * 64 + lane], 1);
            if (cd) cd[(size_t)i * Wp] = ns > 0 ? (unsigned char)((ideal << 5) | mask) : (unsigned char)0xFE;      // 0xFE: rows but no output row
        }
        sweep_flush_strided<BINS>(counters, ((long long)tl * 64) * G + g, G, W - (tile0 + tl) * 64, hist);
    }
}

struct JointCall { const float* members; int M, n; const double* weights; long long W; const double* filters; int G, k, Qa; NdcgLists L; int* status; hipStream_t st;
                   unsigned char* code_out; };

template <int MP>
void launch_joint_once(const JointCall& c, const JointWs& j, const RankStats& S) {
    const dim3 block(256), rows((c.n + 255) / 256), scan(j.cap / SCAN_SLOTS);
    hipLaunchKernelGGL(k_joint_scan_sums, scan, block, 0, c.st, S.cnt, j.bsum);
    hipLaunchKernelGGL(k_joint_scan_top, dim3(1), block, 0, c.st, (int)scan.x, j.bsum, j.hdr);
    hipLaunchKernelGGL(k_joint_scan_apply, scan, block, 0, c.st, S.cnt, (const int4*)j.bsum, j.poff, j.pdense, j.pd_off, j.pd_cnt);
    hipLaunchKernelGGL(k_joint_scatter, rows, block, 0, c.st, c.n, S.pslot, (const int*)j.poff, j.pfill, j.plist);
    hipLaunchKernelGGL((k_joint_pack_p<MP>), rows, block, 0, c.st, c.members, c.M, c.n, (const int*)j.plist, (const int*)j.hdr, (MemRec<MP>*)j.prec);
    hipLaunchKernelGGL((k_joint_pack_q<MP>), rows, block, 0, c.st, c.members, c.M, c.n, c.L, S.pslot, (const int*)j.pdense, (const int*)j.rstatus, c.status,
                       (JointRec<MP>*)j.qrec);
}

template <int K, int MP>
void launch_joint_chunk(const JointCall& c, const JointWs& j, long long tile0, int tiles, u64* hist) {
    const dim3 block(256);
    const unsigned stat_blocks = (unsigned)std::min<long long>(SWEEP_MAX_BLOCKS, ((long long)c.n * tiles + 3) / 4);
    hipLaunchKernelGGL((k_joint_stats<MP>), dim3(stat_blocks), block, 0, c.st, c.weights, c.W, c.M, tile0, tiles, (const int*)j.hdr, (const int*)j.pd_off,
                       (const int*)j.pd_cnt, (const MemRec<MP>*)j.prec, (BestD*)j.tiles, j.tile_bytes, c.status);
    const SweepGrid ug = sweep_grid((long long)tiles * 64, c.Qa);
    hipLaunchKernelGGL((k_joint_unfiltered<K, MP>), dim3(ug.grid), block, 0, c.st, c.weights, c.W, c.M, tile0, c.Qa, ug.slabs, ug.tasks, c.L,
                       (const JointRec<MP>*)j.qrec, (unsigned char*)(j.tiles + j.umask_off), j.tile_bytes);
    const SweepGrid sg = sweep_grid((long long)tiles * c.G * 64, c.Qa);      // a unit per (tile, filter)
    hipLaunchKernelGGL((k_joint_sweep<K, MP>), dim3(sg.grid), block, 0, c.st, c.weights, c.W, c.M, c.filters, c.G, tile0, c.Qa, sg.slabs, sg.tasks, c.L,
                       (const JointRec<MP>*)j.qrec, (const char*)j.tiles, j.tile_bytes, j.umask_off, hist, c.code_out,
                       (c.W + 63) / 64 * 64);
}

template <int MP>
void launch_joint_chunk_k(const JointCall& c, const JointWs& j, long long tile0, int tiles, u64* hist) {
    with_k<MMS_FILTER_MAX_K>(c.k, [&](auto kc) { launch_joint_chunk<decltype(kc)::value, MP>(c, j, tile0, tiles, hist); });
}

}  // namespace

long long joint_sweep_workspace_bytes(long long n, long long Qa, long long Tk, int M, long long tiles_per_chunk) {
    const JointWs j = joint_layout(nullptr, n, Qa, Tk, M);
    return (long long)(j.fixed_bytes + j.tile_bytes * (size_t)tiles_per_chunk);
}

long long joint_sweep_chunk_tiles(long long n, long long Qa, long long Tk, int M, long long W, long long G, int k, bool have_hist, long long workspace_bytes) {
    const JointWs j = joint_layout(nullptr, n, Qa, Tk, M);
    if (W <= 0 || G <= 0) return workspace_bytes >= 0 && (size_t)workspace_bytes >= j.fixed_bytes ? 1 : 0;      // nothing is swept: the per-call stages alone
    const size_t per_tile = j.tile_bytes + (have_hist ? 0 : joint_tile_hist_bytes(G, k));
    if (workspace_bytes < 0 || (size_t)workspace_bytes < j.fixed_bytes + per_tile) return 0;
    return std::max<long long>(1, std::min<long long>(((size_t)workspace_bytes - j.fixed_bytes) / per_tile, (W + 63) / 64));
}

void launch_joint_sweep(const int64_t* query_id, const int64_t* product_id, const float* members, int M, int n, const int64_t* key_query,
                        const int64_t* key_off, const int64_t* key_product, int Qa, int Tk, const double* weights, long long W, const double* filters,
                        long long G, int k, int allow_missing, const double* bin_value, long long n_key_queries_total, void* workspace,
                        long long workspace_bytes, int64_t* hist_out, double* value_out, uint8_t* code_out, int32_t* status, hipStream_t st) {
    // every byte 0xFF, "no rows": k_joint_sweep skips the key queries without rows (and nothing is swept without rows or without a key)
    if (code_out && Qa > 0 && W > 0 && G > 0) (void)hipMemsetAsync(code_out, 0xFF, (size_t)G * (size_t)Qa * (size_t)((W + 63) / 64 * 64), st);
    const int bins = (k + 1) << k;
    const long long items = W * G;
    if (hist_out && items > 0) (void)hipMemsetAsync(hist_out, 0, (size_t)items * bins * 8, st);
    bool swept = false;
    if (Qa <= 0) (void)hipMemsetAsync(status, 0, 16, st);                    // no key: no row belongs to a key query
    else {
        const NdcgLists L = launch_ndcg_lists(query_id, product_id, n, key_query, key_off, key_product, Qa, Tk, allow_missing, workspace, status, st);
        if (n > 0) {
            const JointWs j = joint_layout(workspace, n, Qa, Tk, M);
            const RankStats S = launch_rank_stats(query_id, product_id, members, nullptr, n, j.rank, j.rstatus, st);
            (void)hipMemsetAsync(j.pfill, 0, (size_t)j.cap * 4, st);
            const JointCall c{members, M, n, weights, W, filters, (int)G, k, Qa, L, status, st, code_out};
            const bool mp4 = member_mp(M) == 4;
            if (mp4) launch_joint_once<4>(c, j, S);
            else launch_joint_once<8>(c, j, S);
            if (items > 0) {
                swept = true;
                const long long chunk = joint_sweep_chunk_tiles(n, Qa, Tk, M, W, G, k, hist_out != nullptr, workspace_bytes);   // >= 1: the entry point checked
                for (long long tile0 = 0; tile0 * 64 < W; tile0 += chunk) {
                    const int tiles = (int)std::min<long long>(chunk, (W + 63) / 64 - tile0);
                    const long long v0 = tile0 * 64, nv = std::min<long long>(W - v0, (long long)tiles * 64);
                    // without hist_out the chunk's histograms [vectors of the chunk][G][bins] are one block behind the tables of the chunk's last tile
                    u64* hist = hist_out ? (u64*)hist_out + (size_t)v0 * G * bins : (u64*)(j.tiles + (size_t)chunk * j.tile_bytes);
                    if (!hist_out) (void)hipMemsetAsync(hist, 0, (size_t)nv * G * bins * 8, st);
                    if (mp4) launch_joint_chunk_k<4>(c, j, tile0, tiles, hist);
                    else launch_joint_chunk_k<8>(c, j, tile0, tiles, hist);
                    if (value_out) launch_hist_values((const int64_t*)hist, bin_value, nv * G, bins, n_key_queries_total, value_out + v0 * G, st);
                }
            }
        }
    }
    if (!swept && value_out && items > 0) {
        if (hist_out) launch_hist_values(hist_out, bin_value, items, bins, n_key_queries_total, value_out, st);
        else (void)hipMemsetAsync(value_out, 0, (size_t)items * 8, st);      // zero histograms: every value is +0.0
    }
}
