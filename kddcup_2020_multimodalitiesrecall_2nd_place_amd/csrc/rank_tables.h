// Device helpers shared by rank.hip (mms_rank_submission) and ndcg.hip (mms_ndcg_at_k / mms_key_relevance): the order-preserving integer image of a
// score, the open-addressing key table and the per-wavefront run batching of hot-slot atomics.  Each translation unit gets its own copy.
#pragma once
#include "kernels.h"
#include "../../include/mmscore.h"

namespace {

constexpr long long RANK_EMPTY = MMS_RANK_RESERVED_ID;      // empty slot of the key tables (hipMemsetAsync 0xFF)

typedef unsigned long long u64;

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

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

}  // namespace
