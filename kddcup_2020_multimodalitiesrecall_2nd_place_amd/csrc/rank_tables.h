// Device helpers shared by the four "after scoring" translation units -- rank.hip (mms_rank_submission), ndcg.hip (mms_ndcg_at_k / mms_key_relevance),
// ndcg_sweep.hip (mms_ndcg_weight_sweep) and filter_sweep.hip (mms_filter_sweep) -- one copy of each idea:
//   tables     enc_score / dec_score (the order-preserving integer image of a score), finite_score, table_slot (open-addressing key table),
//              wave_run (per-wavefront run batching of hot-slot atomics), Carver (the workspace carver of the *_layout functions)
//   lists      block_scan / scan_top (exclusive scan over a workgroup, block sums -> prefixes), scatter_rows (counting-sort scatter by wavefront
//              runs), ranks_before / wave_next (one round of the wave-wide arg-max selection)
//   sweeps     TopK (register top-K list of k_sweep; k_filter_sweep writes the same steps out), sweep_task / sweep_zero / sweep_flush / sweep_grid (the (tile, slab) task walk and its
//              [bins][64] LDS histogram; sweep_flush_strided: the flush of joint_sweep.hip, whose tile's items lie n_filters apart),
//              sweep_flags_of_rank (the rank flags as the submission sweeps report them)
// Comparisons, integer work and data movement only: the floating-point arithmetic that defines a result stays in the .hip files, below their
// own fp-contract pragma -- with one exception, the merge of the member scores that two sweeps share: merge_members.h, under a pragma of its
// own.  Each translation unit gets its own copy.
#pragma once
#include "kernels.h"
#include "../../include/mmscore.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr long long RANK_EMPTY = MMS_RANK_RESERVED_ID;      // empty slot of the key tables (hipMemsetAsync 0xFF)

typedef unsigned long long u64;

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves a workspace into 256-byte aligned arrays: take(p, count) points p at the next `count` elements of its type.  o: the bytes taken so far.
struct Carver {
    char* base; size_t o;
    template <typename T> void take(T*& p, size_t count) { p = (T*)(base + o); o += up256(count * sizeof(T)); }
};

__device__ __forceinline__ bool finite_score(double s) { return fabs(s) <= 1.79769313486231570815e308; }     // false for NaN, +-inf

// order-preserving image of a finite double: a < b  <=>  enc(a) < enc(b);  enc(-0.0) == enc(+0.0);  never 0
__device__ __forceinline__ u64 enc_score(double d) {
    u64 b = (u64)__double_as_longlong(d);
    if (d == 0.0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// the exact inverse of enc_score (up to the sign of zero)
__device__ __forceinline__ double dec_score(u64 e) {
    const u64 b = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFull) : ~e;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ unsigned hash64(u64 x) {       // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (unsigned)x;
}

// slot of `key` in an open-addressing table (linear probing; at most cap / 2 distinct keys ever enter, so a walk ends).  *fresh: this call claimed the slot.
__device__ __forceinline__ int table_slot(long long* keys, unsigned mask, long long key, bool* fresh) {
    unsigned h = hash64((u64)key) & mask;
    *fresh = false;
    for (;;) {
        long long cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == RANK_EMPTY) {
            const long long old = (long long)atomicCAS((u64*)&keys[h], (u64)RANK_EMPTY, (u64)key);
            if (old == RANK_EMPTY) { *fresh = true; return (int)h; }
            cur = old;
        }
        if (cur == key) return (int)h;
        h = (h + 1) & mask;
    }
}

// Runs of adjacent live lanes of a wavefront that hold the same key.  head: first lane of my run; len: its length.  Every lane of the wavefront must call it.
struct Run { int head, len; };
__device__ __forceinline__ Run wave_run(long long key, bool live) {
    const int lane = threadIdx.x & 63;
    const long long prev = __shfl_up(key, 1);
    const int plive = __shfl_up((int)live, 1);
    const bool is_head = live && (lane == 0 || !plive || prev != key);
    const u64 heads = __ballot(is_head), lives = __ballot(live);
    const u64 upto = (2ull << lane) - 1;                  // lanes 0 .. lane (lane 63: all ones)
    Run r;
    r.head = 63 - __clzll((long long)((heads & upto) | 1ull));
    const u64 above = (heads | ~lives) & ~upto;
    r.len = (above ? __ffsll((long long)above) - 1 : 64) - r.head;
    return r;
}

// ---- lists: scan, scatter, selection ----

__device__ __forceinline__ int scan_shfl_up(int a, int d) { return __shfl_up(a, d); }
__device__ __forceinline__ int4 scan_shfl_up(int4 a, int d) { return make_int4(__shfl_up(a.x, d), __shfl_up(a.y, d), __shfl_up(a.z, d), __shfl_up(a.w, d)); }

// exclusive scan of one T (int, or int4 summed member by member) per thread over the 256 threads of a workgroup; *total = the workgroup's sum
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* total) {
    __shared__ T wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = scan_shfl_up(inc, d);
        if (lane >= d) inc = inc + o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    T base{}, tot{};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < wv) base = base + wsum[i];
        tot = tot + wsum[i];
    }
    *total = tot;
    __syncthreads();
    return base + inc - v;
}

// one workgroup of 256 threads: the block sums bsum[0 .. nb) -> their exclusive prefixes (in place); returns the total in every thread
template <typename T>
__device__ __forceinline__ T scan_top(T* bsum, int nb) {
    const int per = (nb + 255) / 256, b0 = threadIdx.x * per;
    T t{};
    for (int i = b0; i < b0 + per && i < nb; ++i) t = t + bsum[i];
    T total;
    T run = block_scan(t, &total);
    for (int i = b0; i < b0 + per && i < nb; ++i) {
        const T v = bsum[i];
        bsum[i] = run;
        run = run + v;
    }
    return total;
}

// Counting-sort scatter, one thread per row: row r goes into the list of slot[r] (-1: no list), which starts at off[slot[r]]; one atomic per RUN of
// equal slots inside a wavefront.  off + fill stays below the rows counted for the slot: inside [0, n).  The order inside a list is arbitrary.
__device__ __forceinline__ void scatter_rows(int n, const int* slot, const int* off, int* fill, int* list) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int s = r < n ? slot[r] : -1;
    const bool live = s >= 0;
    const Run run = wave_run((long long)s, live);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (live && lane == run.head) base = off[s] + atomicAdd(&fill[s], run.len);
    base = __shfl(base, run.head);
    if (live) list[base + lane - run.head] = r;
}

// (key a, tie a) ranks before (key b, tie b): key descending -- a score image, or a finite double with -0.0 == +0.0 (the IEEE comparison, which
// orders finite doubles as enc_score's images do) --, then tie ascending (a row, or row << 1 | rel: a list holds a row once, so the order is total)
template <typename S>
__device__ __forceinline__ bool ranks_before(S ka, unsigned ta, S kb, unsigned tb) { return ka > kb || (ka == kb && ta < tb); }

// One round of the selection, by a whole wavefront: the best of load(0 .. cnt) that ranks strictly after the previous pick, in every lane; image 0:
// there is none.  No real image is 0, so load returns image 0 for an entry to skip; the first round starts from {~0, 0}: every image is below ~0
// (no finite score has the image ~0 either: it would be the bit pattern of a NaN, and a non-finite score is flagged before any list is ranked).
struct Pick { u64 img; unsigned tie; };
template <typename Load>
__device__ __forceinline__ Pick wave_next(int cnt, Pick prev, Load load) {
    Pick b{0, 0xFFFFFFFFu};
    for (int x = threadIdx.x & 63; x < cnt; x += 64) {
        const Pick c = load(x);
        if (ranks_before(prev.img, prev.tie, c.img, c.tie) && ranks_before(c.img, c.tie, b.img, b.tie)) b = c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const Pick o{__shfl_xor(b.img, d), __shfl_xor(b.tie, d)};
        if (ranks_before(o.img, o.tie, b.img, b.tie)) b = o;
    }
    return b;
}

// ---- sweeps: a lane owns a grid point and ranks a key query's rows serially ----

// The K best (key, meta = row << 1 | rel) seen so far in registers, best first (static indexing: K comparisons and selects per insert, no
// data-dependent branch).  An empty place holds the key passed to clear() -- one that no row ranks after -- with row 2^31 - 1, relevance 0.
template <int K, typename S>
struct TopK {
    S E[K];
    unsigned R[K];
    __device__ __forceinline__ void clear(S empty) {
#pragma unroll
        for (int j = 0; j < K; ++j) { E[j] = empty; R[j] = 0xFFFFFFFEu; }
    }
    // c[j] = this row ranks before place j (monotone in j: the list is sorted by a total order); on == false: nothing changes.  (key and meta by
    // reference: with copies of them k_sweep's loop compiles to more registers and instructions, profiles/rd13_rank_family_refactor.txt)
    __device__ __forceinline__ void insert(bool on, const S& key, const unsigned& meta) {
        bool c[K];
#pragma unroll
        for (int j = 0; j < K; ++j) c[j] = on && ranks_before(key, meta, E[j], R[j]);
#pragma unroll
        for (int j = K - 1; j >= 1; --j) {
            E[j] = c[j - 1] ? E[j - 1] : (c[j] ? key : E[j]);
            R[j] = c[j - 1] ? R[j - 1] : (c[j] ? meta : R[j]);
        }
        E[0] = c[0] ? key : E[0];
        R[0] = c[0] ? meta : R[0];
    }
    __device__ __forceinline__ unsigned rel_mask() const {                   // bit j: the j-th place is relevant (an empty place is not)
        unsigned mask = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) mask |= (R[j] & 1u) << j;
        return mask;
    }
};

// status[2] of launch_rank_stats (mms_rank_submission's bits) as mms_filter_sweep / mms_joint_sweep report it: non-finite (2) and reserved id (8)
// stay, the repeated pair moves from bit 0 to bit 4 (bit 2, the output overflow, belongs to a stage the sweeps do not run)
__device__ __forceinline__ int sweep_flags_of_rank(int f) { return (f & 2) | (f & 8) | ((f & 1) << 4); }

// The one switch over a sweep's K: f(std::integral_constant<int, K>) with K = k for k in [1, KMAX] (the entry points check the range; above it: KMAX)
template <int KMAX, typename F>
void with_k(int k, F f) {
    if constexpr (KMAX > 1) { if (k < KMAX) return with_k<KMAX - 1>(k, f); }
    f(std::integral_constant<int, KMAX>{});
}

constexpr int SWEEP_MAX_BLOCKS = 4096;   // bounded grid: workgroups stride over the tasks
constexpr int SWEEP_TARGET_TASKS = 2048; // small grids: the key queries are cut into slabs until there are about this many tasks

// A task is (tile of 64 grid points, slab of key queries): `items` grid points, Qa key queries -> slabs per tile, tasks, workgroups
struct SweepGrid { int slabs; long long tasks; unsigned grid; };
inline SweepGrid sweep_grid(long long items, int Qa) {
    const long long tiles = (items + 63) / 64;
    const int slabs = (int)std::max<long long>(1, std::min<long long>((SWEEP_TARGET_TASKS + tiles - 1) / tiles, ((long long)Qa + 3) / 4));
    return SweepGrid{slabs, tiles * slabs, (unsigned)std::min<long long>(tiles * slabs, SWEEP_MAX_BLOCKS)};
}
// task t -> its tile and its key queries [q0, q1)
struct SweepTask { long long tile; int q0, q1; };
__device__ __forceinline__ SweepTask sweep_task(long long t, int slabs, int Qa) {
    const int per = (Qa + slabs - 1) / slabs;
    const long long tile = t / slabs;
    const int slab = (int)(t - tile * slabs);
    return SweepTask{tile, slab * per, min(Qa, (slab + 1) * per)};
}
// The task's histogram in LDS, counters[bin * 64 + lane of the tile] (lane = bank: conflict-free): zeroed by the workgroup before the task, and
// its non-zero counters added to hist[item][bin] with 64-bit global atomics after it (items >= n_items are padding)
template <int BINS>
__device__ __forceinline__ void sweep_zero(int* counters) {
    for (int x = threadIdx.x; x < BINS * 64; x += 256) counters[x] = 0;
    __syncthreads();
}
template <int BINS>
__device__ __forceinline__ void sweep_flush(const int* counters, long long tile, long long n_items, u64* hist) {
    __syncthreads();
    for (int x = threadIdx.x; x < BINS * 64; x += 256) {
        const int c = counters[x];
        const long long item = tile * 64 + (x & 63);
        if (c != 0 && item < n_items) atomicAdd(&hist[(size_t)item * BINS + (x >> 6)], (u64)c);
    }
    __syncthreads();
}
// the same with the tile's lanes `stride` items apart: lane l of the tile adds to item item0 + l * stride (lanes >= n_lanes are padding)
template <int BINS>
__device__ __forceinline__ void sweep_flush_strided(const int* counters, long long item0, long long stride, long long n_lanes, u64* hist) {
    __syncthreads();
    for (int x = threadIdx.x; x < BINS * 64; x += 256) {
        const int c = counters[x];
        const long long l = x & 63;
        if (c != 0 && l < n_lanes) atomicAdd(&hist[(size_t)(item0 + l * stride) * BINS + (x >> 6)], (u64)c);
    }
    __syncthreads();
}

}  // namespace
