// Resampling the joint fit (mms_resample_select, include/mmscore.h): k-fold, repeated k-fold and bootstrap estimates of the held-out nDCG@k from ONE
// joint sweep.  The sweep keeps the byte code of every (weight vector v, filter g, key query i) (mms_joint_sweep_codes: code[(g * Qa + i) * Wp + v]); a
// replicate r is a row of small integer counts over the key queries, and its value for item (v, g) is
//     fit[r][item] = (sum over i = 0 .. Qa - 1, in key order, of double(count_fit[r][i]) * byte_value[code[item][i]]) / double(sum_i count_fit[r][i])
// IEEE double from +0.0, every product, every sum and the division rounded on its own (contraction is off).  A term with count 0 adds +0.0 to a sum that
// is never negative: the same bits as leaving it out.  Per replicate the FIRST item v * G + g at the maximum wins; the [R][W * G] matrix is never stored.
//   k_resample_sums    per replicate the integer sums of its two count rows (the divisors); an empty fit row raises flag bit 5 of status[2]
//   k_resample_counts  count_fit transposed and padded to cnt_t[i][Rp] (Rp = R rounded up to RB, zeros past R): the RB counts that a block of
//                      replicates needs for key query i are then RB consecutive bytes at a wave-uniform address -- one scalar load
//   k_resample         a task is (four units, block of RB replicates); a unit is (filter g, tile of 64 vectors), one per wavefront, a lane owning one
//                      item.  The lane walks the key queries in order: its code byte (64 consecutive bytes per wavefront), the byte's value from a
//                      2 KiB LDS table, then RB multiply + add pairs into RB fp64 accumulators in registers.  After the walk the division, a wavefront
//                      reduction and a workgroup reduction by the total order (value descending, item ascending): one (value, item) per (replicate,
//                      task row) into part[r][ub]
//   k_resample_pick    a workgroup per replicate: the best of its partials by the same total order -- neither the arrival order nor the unit order
//                      can matter --, then thread t walks the codes of the winner (t = 0) or of probe t - 1 in key order for the fit and eval sums
// No floating-point atomics, no kernel waits on another workgroup, bounded grids: equal inputs give equal bytes.
#include "rank_tables.h"

#pragma clang fp contract(off)

namespace {

constexpr int RB = 16;                                      // replicates per task: 16 fp64 accumulators per lane, their counts one 16-byte scalar load
constexpr int RS_MAX_BLOCKS = 4096;                         // bounded grids: workgroups stride over the tasks
constexpr int NO_ITEM = 0x7FFFFFFF;

struct __attribute__((aligned(16))) Part { double value; int item; int pad; };
struct __attribute__((aligned(16))) Cnt16 { unsigned w[4]; };

struct ResWs { int* sums; unsigned char* cnt_t; Part* part; long long Rp, units, UB; size_t bytes; };

ResWs res_layout(void* base, long long W, long long G, long long Qa, long long R) {
    ResWs s{};
    s.Rp = (R + RB - 1) / RB * RB;
    s.units = G * ((W + 63) / 64);
    s.UB = (s.units + 3) / 4;
    Carver cv{(char*)base, 0};
    cv.take(s.sums, (size_t)(2 * s.Rp > 0 ? 2 * s.Rp : 1));
    cv.take(s.cnt_t, (size_t)(Qa * s.Rp > 0 ? Qa * s.Rp : 1));
    cv.take(s.part, (size_t)(s.UB * s.Rp > 0 ? s.UB * s.Rp : 1));
    s.bytes = cv.o;
    return s;
}

// (value descending, item ascending): a total order on the partials, whose items are distinct (or NO_ITEM with value -1: a lane without an item)
__device__ __forceinline__ bool before(double va, int ia, double vb, int ib) { return (va > vb) | ((va == vb) & (ia < ib)); }

__device__ __forceinline__ void wave_best(double& v, int& it) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(it, d, 64);
        const bool take = before(ov, oi, v, it);
        v = take ? ov : v;
        it = take ? oi : it;
    }
}

// sums[2r] / sums[2r + 1] = the integer sums of count_fit[r] / count_eval[r] (at most 255 * 2^20); rows r in [R, Rp): 0
__global__ __launch_bounds__(256) void k_resample_sums(const unsigned char* __restrict__ count_fit, const unsigned char* __restrict__ count_eval, int R, int Rp, int Qa,
                                                       int* __restrict__ sums, int* status) {
    __shared__ int acc[2];
    for (int r = blockIdx.x; r < Rp; r += gridDim.x) {
        if (threadIdx.x < 2) acc[threadIdx.x] = 0;
        __syncthreads();
        int f = 0, e = 0;
        if (r < R)
            for (int i = threadIdx.x; i < Qa; i += 256) { f += count_fit[(size_t)r * Qa + i]; e += count_eval[(size_t)r * Qa + i]; }
        if (f) atomicAdd(&acc[0], f);                                        // integer sums: the order cannot matter
        if (e) atomicAdd(&acc[1], e);
        __syncthreads();
        if (threadIdx.x == 0) {
            sums[2 * r] = acc[0]; sums[2 * r + 1] = acc[1];
            if (r < R && acc[0] == 0) atomicOr(&status[2], MMS_FLAG_EMPTY_FIT);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_resample_counts(const unsigned char* __restrict__ count_fit, int R, int Rp, int Qa, unsigned char* __restrict__ cnt_t) {
    const long long total = (long long)Qa * Rp;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long long)gridDim.x * 256) {
        const int i = (int)(x / Rp), r = (int)(x - (long long)i * Rp);
        cnt_t[x] = r < R ? count_fit[(size_t)r * Qa + i] : (unsigned char)0;
    }
}

// tasks = UB * (Rp / RB), the replicate block fastest: the workgroups in flight together read the same code lines
__global__ __launch_bounds__(256) void k_resample(const unsigned char* __restrict__ code, int W, long long Wp, int G, int Qa, const unsigned char* __restrict__ cnt_t,
                                                  int Rp, const int* __restrict__ sums, const double* __restrict__ byte_value, long long units, long long UB,
                                                  long long tasks, Part* __restrict__ part) {
    __shared__ double bv[256];
    __shared__ double wval[4][RB];
    __shared__ int witem[4][RB];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // (scalar: the unit and the counts are wave-uniform)
    bv[threadIdx.x] = byte_value[threadIdx.x];
    __syncthreads();
    const int VT = (int)(Wp >> 6), rblocks = Rp / RB;
    for (long long t = blockIdx.x; t < tasks; t += gridDim.x) {
        const long long ub = t / rblocks;
        const int rb = (int)(t - ub * rblocks);
        const long long unit = ub * 4 + wv;
        const bool unit_live = unit < units;
        const int g = unit_live ? (int)(unit / VT) : 0, v = (unit_live ? (int)(unit - (long long)g * VT) : 0) * 64 + lane;     // g < G, v < Wp
        const bool live = unit_live && v < W;
        double acc[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) acc[j] = 0.0;
        if (unit_live && Qa > 0) {
            const unsigned char* cp = code + (size_t)g * Qa * Wp + v;       // (g * Qa + i) * Wp + v < G * Qa * Wp
            const unsigned char* ct = cnt_t + (size_t)rb * RB;               // i * Rp + rb * RB + j < Qa * Rp
            // four key queries per step, the next step's code bytes and counts in flight while this one is summed (indices clamped to Qa - 1: inside the arrays)
            unsigned cur[4];
            Cnt16 cc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = min(u, Qa - 1);
                cur[u] = cp[(size_t)i * Wp];
                cc[u] = *(const Cnt16*)(ct + (size_t)i * Rp);                // Rp and rb * RB are multiples of 16, cnt_t is 256-byte aligned
            }
            for (int i0 = 0; i0 < Qa; i0 += 4) {
                unsigned nxt[4];
                Cnt16 nc[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = min(i0 + 4 + u, Qa - 1);
                    nxt[u] = cp[(size_t)i * Wp];
                    nc[u] = *(const Cnt16*)(ct + (size_t)i * Rp);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (i0 + u < Qa) {                                       // (wave-uniform) key order: u ascending
                        const double val = bv[cur[u]];
#pragma unroll
                        for (int j = 0; j < RB; ++j) {
                            const double prod = (double)((cc[u].w[j >> 2] >> ((j & 3) * 8)) & 0xFFu) * val;
                            acc[j] = acc[j] + prod;
                        }
                    }
                    cur[u] = nxt[u];
                    cc[u] = nc[u];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int sf = sums[2 * (rb * RB + j)];
            double val = live && sf > 0 ? acc[j] / (double)sf : -1.0;        // (an empty fit row: k_resample_pick reads no partial of it)
            int item = live ? v * G + g : NO_ITEM;                           // < W * G <= 2^22
            wave_best(val, item);
            if (lane == 0) { wval[wv][j] = val; witem[wv][j] = item; }
        }
        __syncthreads();
        if (threadIdx.x < RB) {
            double val = wval[0][threadIdx.x];
            int item = witem[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const double ov = wval[w][threadIdx.x];
                const int oi = witem[w][threadIdx.x];
                const bool take = before(ov, oi, val, item);
                val = take ? ov : val;
                item = take ? oi : item;
            }
            Part o;
            o.value = val; o.item = item; o.pad = 0;
            part[(size_t)(rb * RB + threadIdx.x) * UB + ub] = o;             // r < Rp, ub < UB
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_resample_pick(const Part* __restrict__ part, long long UB, int R, const int* __restrict__ sums,
                                                       const unsigned char* __restrict__ code, int W, long long Wp, int G, int Qa,
                                                       const unsigned char* __restrict__ count_fit, const unsigned char* __restrict__ count_eval,
                                                       const double* __restrict__ byte_value, const int64_t* __restrict__ probe_item, int P,
                                                       int64_t* __restrict__ best, double* __restrict__ fit_value, double* __restrict__ eval_value,
                                                       double* __restrict__ probe_fit, double* __restrict__ probe_eval) {
    __shared__ double bv[256];
    __shared__ double wval[4];
    __shared__ int witem[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bv[threadIdx.x] = byte_value[threadIdx.x];
    const long long items = (long long)W * G;
    const double nan = __builtin_nan("");
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const int sf = sums[2 * r], se = sums[2 * r + 1];
        double val = -1.0;
        int item = NO_ITEM;
        for (long long u = threadIdx.x; u < UB; u += 256) {
            const Part p = part[(size_t)r * UB + u];
            const bool take = before(p.value, p.item, val, item);
            val = take ? p.value : val;
            item = take ? p.item : item;
        }
        wave_best(val, item);
        __syncthreads();                                                     // (the table is written; the previous replicate's readers are done)
        if (lane == 0) { wval[wv] = val; witem[wv] = item; }
        __syncthreads();
        val = wval[0]; item = witem[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const bool take = before(wval[w], witem[w], val, item);
            val = take ? wval[w] : val;
            item = take ? witem[w] : item;
        }
        const bool empty = sf == 0 || item == NO_ITEM;                        // an empty fit row (flagged by k_resample_sums): no winner
        for (int t = threadIdx.x; t <= P; t += 256) {
            const long long it = t == 0 ? (empty ? -1 : (long long)item) : probe_item[t - 1];
            double f = nan, e = nan;
            if (it >= 0 && it < items) {                                     // (a probe outside the grid: NaN, nothing is read)
                const int v = (int)(it / G), g = (int)(it - (long long)v * G);
                const unsigned char* cp = code + (size_t)g * Qa * Wp + v;
                const unsigned char* cf = count_fit + (size_t)r * Qa;
                const unsigned char* ce = count_eval + (size_t)r * Qa;
                double af = 0.0, ae = 0.0;
                for (int i = 0; i < Qa; ++i) {
                    const double x = bv[cp[(size_t)i * Wp]];
                    const double pf = (double)cf[i] * x;
                    const double pe = (double)ce[i] * x;
                    af = af + pf;
                    ae = ae + pe;
                }
                f = af / (double)sf;                                         // 0.0 / 0.0: NaN
                e = ae / (double)se;
            }
            if (t == 0) { best[r] = it; fit_value[r] = empty ? nan : val; eval_value[r] = e; }
            else { probe_fit[(size_t)r * P + t - 1] = f; probe_eval[(size_t)r * P + t - 1] = e; }
        }
    }
}

}  // namespace

long long resample_workspace_bytes(long long n_weights, long long n_filters, long long n_key_queries, long long n_replicates) {
    return (long long)res_layout(nullptr, n_weights, n_filters, n_key_queries, n_replicates).bytes;
}

void launch_resample_select(const uint8_t* code, long long W, long long G, int Qa, const uint8_t* count_fit, const uint8_t* count_eval, int R,
                            const double* byte_value, const int64_t* probe_item, int P, void* workspace, int64_t* best, double* fit_value,
                            double* eval_value, double* probe_fit, double* probe_eval, int32_t* status, hipStream_t st) {
    if (R <= 0) return;
    const ResWs s = res_layout(workspace, W, G, Qa, R);
    const dim3 block(256);
    const int Rp = (int)s.Rp;
    hipLaunchKernelGGL(k_resample_sums, dim3((unsigned)std::min<long long>(Rp, RS_MAX_BLOCKS)), block, 0, st, count_fit, count_eval, R, Rp, Qa, s.sums, status);
    const long long tasks = s.UB * (s.Rp / RB);
    if (tasks > 0 && Qa > 0) {
        const long long cells = (long long)Qa * Rp;
        hipLaunchKernelGGL(k_resample_counts, dim3((unsigned)std::min<long long>((cells + 255) / 256, RS_MAX_BLOCKS)), block, 0, st, count_fit, R, Rp, Qa, s.cnt_t);
    }
    if (tasks > 0)
        hipLaunchKernelGGL(k_resample, dim3((unsigned)std::min<long long>(tasks, RS_MAX_BLOCKS)), block, 0, st, code, (int)W, (W + 63) / 64 * 64, (int)G, Qa,
                           (const unsigned char*)s.cnt_t, Rp, (const int*)s.sums, byte_value, s.units, s.UB, tasks, s.part);
    hipLaunchKernelGGL(k_resample_pick, dim3((unsigned)std::min<int>(R, RS_MAX_BLOCKS)), block, 0, st, (const Part*)s.part, s.UB, R, (const int*)s.sums, code, (int)W,
                       (W + 63) / 64 * 64, (int)G, Qa, count_fit, count_eval, byte_value, probe_item, P, best, fit_value, eval_value, probe_fit, probe_eval);
}
