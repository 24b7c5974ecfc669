// The arithmetic contract that ndcg_sweep.hip and joint_sweep.hip share, in ONE copy: the merge of the fp32 member scores in IEEE double,
//     score_v[r] = (...((w[v][0] * s0) + w[v][1] * s1) + ...) + w[v][M - 1] * s_{M-1}
// every product and every sum rounded on its own (ndcg.merge_members on the host) -- NO fused multiply-add: contraction is off from here on.
// The kernels walk MP = 4 or 8 padded members.  A padded member (m >= M) has score 0 and weight 0: its term adds +0.0, which can change the
// sign of a zero sum and nothing else -- and -0.0 compares, ranks and subtracts as +0.0: the MP-term sum ranks and flags as the M-term sum.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

inline int member_mp(int M) { return M <= 4 ? 4 : 8; }

// the member scores of row r (members: fp32 [M][n], member-major), zero past the M-th
template <int MP>
__device__ __forceinline__ void load_members(const float* __restrict__ members, int M, int n, int r, float (&s)[MP]) {
#pragma unroll
    for (int m = 0; m < MP; ++m) s[m] = m < M ? members[(size_t)m * n + r] : 0.0f;
}

// the lane's weight vector v (weights: fp64 [W][M]), zero past the M-th and for a lane past the grid
template <int MP>
__device__ __forceinline__ void lane_weights(const double* __restrict__ weights, long long v, bool live, int M, double (&w)[MP]) {
#pragma unroll
    for (int m = 0; m < MP; ++m) w[m] = (live && m < M) ? weights[v * M + m] : 0.0;
}

// ONE statement sequence for the kernels of joint_sweep.hip: its product statistics and its sweep subtract what this returns, so s - best is exact
// for the best row.  (k_sweep of ndcg_sweep.hip spells the same statements out: it measured slower through this function.)
template <int MP>
__device__ __forceinline__ double merged(const double (&w)[MP], const float (&m)[MP]) {
    double s = w[0] * (double)m[0];
#pragma unroll
    for (int i = 1; i < MP; ++i) {
        const double prod = w[i] * (double)m[i];
        s = s + prod;
    }
    return s;
}

}  // namespace
