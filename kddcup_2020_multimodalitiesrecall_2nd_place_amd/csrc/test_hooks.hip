// libmmscore test and lab hooks: the mms_dbg_* entry points declared under MMS_TEST_HOOKS in include/mmscore.h -- fp32 in / fp32 out around the production
// kernels, for the kernel-level GPU tests and the A/B tools under tools/.  No hook here reads an mms_handle; those that do (mms_dbg_counter, mms_debug_read_x,
// the timing readers) live next to the handle in api.hip.  Every hook reads: check the arguments, build the operands in ONE DbgPool, launch, finish.
#include <cstdlib>
#include <string>
#include <vector>

#define MMS_TEST_HOOKS
#include "../../include/mmscore.h"
#include "kernels.h"

extern "C" __global__ void k_fill_random(float* p, long long n, unsigned seed) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        unsigned x = (unsigned)(i * 2654435761u) ^ seed;
        x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
        p[i] = (float)(int)x * (1.0f / 2147483648.0f);   // uniform [-1, 1)
    }
}

namespace {

constexpr int H = MMS_HIDDEN;

int fail(int rc, const std::string& m) { set_global_error(m.c_str()); return rc; }      // what mms_global_error() returns next
int refuse(const std::string& m) { return fail(MMS_ERR_ARG, m); }
#define DBG_TRY(expr) do { if ((expr) != hipSuccess) return fail(MMS_ERR_HIP, #expr); } while (0)

// The device buffers of one hook call, freed on EVERY way out: a HIP error, a refusal, success.  Freeing device memory waits for the device, so a pool that
// unwinds on an early return while kernels are still queued on the caller's stream is safe.  A failed allocation comes back as nullptr and is remembered in
// `bad`: a hook builds all its operands (the helpers below launch nothing on a nullptr), then checks `bad` once.
struct DbgPool {
    std::vector<void*> p;
    const char* bad = nullptr;
    DbgPool() = default;
    DbgPool(const DbgPool&) = delete;
    ~DbgPool() { for (void* q : p) (void)hipFree(q); }
    template <class T>
    T* get(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 4) != hipSuccess) { bad = "hipMalloc"; return nullptr; }
        p.push_back(q);
        return (T*)q;
    }
};
// ... and the event pair of the bench hook
struct DbgEvents {
    hipEvent_t e[2] = {nullptr, nullptr};
    DbgEvents() = default;
    DbgEvents(const DbgEvents&) = delete;
    ~DbgEvents() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
    hipError_t create() {
        for (hipEvent_t& v : e) if (hipError_t rc = hipEventCreate(&v)) return rc;
        return hipSuccess;
    }
};

// ---- operand builders: each allocates from the pool and queues its preparation kernel on st ----
struct DbgPlanes { bf16* hi = nullptr; bf16* lo = nullptr; };      // split planes in the hl32 layout (common.h): ONE buffer, lo == hi + 32
DbgPlanes dbg_planes(DbgPool& pool, int64_t elems) {
    DbgPlanes pl;
    pl.hi = pool.get<bf16>((size_t)elems * 4);
    if (pl.hi) pl.lo = pl.hi + MMS_PLANE_LO;
    return pl;
}
DbgPlanes dbg_planes_from(DbgPool& pool, const float* src_f32, int64_t elems, hipStream_t st) {
    const DbgPlanes pl = dbg_planes(pool, elems);
    if (pl.hi) launch_split_f32(src_f32, pl.hi, pl.lo, elems, st);
    return pl;
}
// W [N][K] tiled: the hi plane (== RNE bf16 of the weights), the lo plane N * K elements behind it
bf16* dbg_tiled_weights(DbgPool& pool, const float* w_f32_nk, int64_t N, int64_t K, hipStream_t st) {
    bf16* w = pool.get<bf16>((size_t)N * K * 4);
    if (w) launch_tile_weights(w_f32_nk, w, w + N * K, N, K, st);
    return w;
}
// the device-side live-row count (GemmParams::m_dev): nullptr when host < 0 (every row is live).  `host` must outlive the hook's last wait.
const int* dbg_live(DbgPool& pool, const int32_t& host, hipStream_t st) {
    int* d = pool.get<int>(16);
    if (d && hipMemcpyAsync(d, &host, 4, hipMemcpyHostToDevice, st) != hipSuccess) pool.bad = "hipMemcpyAsync of the live-row count";
    return host >= 0 ? d : nullptr;
}
// two-pass GEMM on split planes with identity row maps; a caller sets what else its launch needs
GemmParams dbg_gemm_params(DbgPlanes a, int64_t lda, const bf16* w, int64_t M, int64_t N, int64_t K, const float* bias, int act) {
    GemmParams p{};
    p.a_hi = a.hi; p.a_lo = a.lo; p.lda = (int)lda; p.w = w; p.bias = bias; p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act;
    p.amap = RowMap{0, 0, 0}; p.cmap = RowMap{0, 0, 0}; p.rmap = RowMap{0, 0, 0};
    return p;
}
// the end of a hook: the output planes (if any, and if something ran) back to fp32, wait, check; a launch no kernel took is MMS_ERR_ARG with `refused`
int dbg_finish(hipStream_t st, DbgPlanes c = DbgPlanes{}, float* c_f32 = nullptr, int64_t n = 0, bool taken = true, const std::string& refused = "") {
    if (taken && c.hi) launch_planes_to_f32(c.hi, c.lo, c_f32, n, st);
    DBG_TRY(hipStreamSynchronize(st));
    DBG_TRY(hipGetLastError());
    return taken ? MMS_OK : refuse(refused);
}

// ---- host-side checks of the addressing hooks (mms_rows_spec): nothing is launched until every row a launch can address lies inside its buffer ----
inline int64_t dbg_rowmap(const int32_t m[3], int64_t r) { return m[0] ? (r / m[0]) * (int64_t)m[1] + m[2] + r % m[0] : r; }
inline RowMap dbg_rowmap_dev(const int32_t m[3]) { return m[0] ? RowMap{m[0], m[1], m[2]} : RowMap{0, 0, 0}; }
// every logical row r < M (the padded bound, not the live count) maps into [0, rows): through the device index when there is one, else through the map
bool dbg_rows_inside(const int32_t m[3], const int32_t* index_dev, int64_t M, int64_t rows) {
    if (rows <= 0) return false;
    if (index_dev) {
        std::vector<int32_t> h((size_t)M);
        if (hipMemcpy(h.data(), index_dev, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (int32_t v : h) if (v < 0 || v >= rows) return false;
        return true;
    }
    if (m[0] < 0) return false;
    for (int64_t r = 0; r < M; ++r) { const int64_t v = dbg_rowmap(m, r); if (v < 0 || v >= rows) return false; }
    return true;
}
// the physical output image of a spec: elements, or -1 when the spec's output fields contradict each other / a row r < M leaves the image
int64_t dbg_out_elems(int32_t out_kind, int64_t M, int64_t N, int32_t ldo, int64_t c_rows, const int32_t cmap[3], int32_t hm_rows, int32_t hm_col0, int32_t hm_blocks) {
    if (out_kind == 2) {
        if (N % 64 || hm_rows <= 0 || hm_blocks <= 0 || hm_col0 < 0 || hm_col0 % 64 || (hm_col0 + N) / 64 > hm_blocks) return -1;
        if (!dbg_rows_inside(cmap, nullptr, M, hm_rows)) return -1;
        return (int64_t)hm_blocks * hm_rows * 64;
    }
    if (out_kind != 0 && out_kind != 1) return -1;
    if (c_rows <= 0 || ldo < N || ldo % (out_kind == 1 ? 32 : 4) || c_rows * (int64_t)ldo > (1ll << 31)) return -1;
    if (!dbg_rows_inside(cmap, nullptr, M, c_rows)) return -1;
    return c_rows * (int64_t)ldo;
}
// per-pair rows of a ragged stream, checked on the host before a kernel reads through them: 1 <= cnt <= S, [off, off + cnt) inside the stream
bool dbg_pairs_ok(const int32_t* off_dev, const int32_t* cnt_dev, int64_t B, int S, int64_t rows) {
    std::vector<int32_t> off((size_t)B), cnt((size_t)B);
    if (hipMemcpy(off.data(), off_dev, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(cnt.data(), cnt_dev, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int64_t b = 0; b < B; ++b)
        if (cnt[b] < 1 || cnt[b] > S || off[b] < 0 || (int64_t)off[b] + cnt[b] > rows) return false;
    return true;
}

// ---- the two-pass GEMM hooks: mms_dbg_gemm_rows, and mms_dbg_gemm / mms_dbg_gemm_ex as identity specs of it ----
// the launcher of ONE named engine, without the fall-backs of gemm_dispatch.hip's run_engine: what the engine refuses comes back as false
bool dbg_launch_named(const GemmParams& p, int nsplit, hipStream_t st) {
    switch ((Engine)p.engine) {
        case ENG_TILE_128: return launch_gemm_tile(p, nsplit, ENG_TILE_128, st);
        case ENG_TILE_DMA: case ENG_TILE: case ENG_TILE_256: return nsplit != 3 && launch_gemm_tile(p, nsplit, (Engine)p.engine, st);      // (three passes: the 128 x 128 tile only)
        case ENG_PP: return launch_gemm_pp(p, nsplit, 0, st);
        case ENG_PP_PERSIST: return launch_gemm_pp(p, nsplit, 0, st, true);
        case ENG_PPW: return nsplit == 3 && launch_gemm_ppw(p, st);
        case ENG_SKINNY: return launch_gemm_skinny(p, nsplit, st);
        case ENG_SKINNY_K4: case ENG_SKINNY_K8: { GemmParams q = p; q.wave_k_slices = p.engine == ENG_SKINNY_K4 ? 4 : 8; return launch_gemm_skinny(q, nsplit, st); }
        default: return false;
    }
}
// the dense launch of mms_dbg_gemm / _ex as a spec: identity maps, every row live unless m_live says otherwise, output [M][N] (head-major: N / 64 blocks of M rows)
mms_rows_spec dbg_dense_spec(int64_t M, int64_t N, int64_t K, int64_t lda, int32_t act, int32_t nsplit, int32_t engine, int32_t out_kind) {
    mms_rows_spec s{};
    s.M = (int32_t)M; s.N = (int32_t)N; s.K = (int32_t)K; s.nsplit = nsplit; s.engine = engine; s.act = act; s.m_live = -1;
    s.a_rows = s.r_rows = s.c_rows = s.hm_rows = (int32_t)M; s.lda = (int32_t)lda; s.out_kind = out_kind; s.ldo = (int32_t)N; s.hm_blocks = (int32_t)(N / 64);
    return s;
}
// One launch of a CHECKED spec (n_out: the elements of its physical output image).  named: the spec's engine through its own launcher alone; else through
// launch_gemm, i.e. ENG_AUTO and the fall-backs of a forward.  out_kind 1: the planes start as the split of the caller's image c_f32 (a value with an exact
// hi / lo split comes back as it went in) and the WHOLE physical buffer is converted back -- unless nothing was launched: then c_f32 is not touched at all.
int dbg_gemm_run(const char* who, bool named, const mms_rows_spec& s, int64_t n_out, const float* a_f32, const int32_t* a_index, const float* w_f32_nk,
                 const float* bias, const float* resid_f32, const int32_t* r_index, float* c_f32, hipStream_t st) {
    const int64_t N = s.N, K = s.K;
    DbgPool pool;
    const DbgPlanes a = dbg_planes_from(pool, a_f32, (int64_t)s.a_rows * s.lda, st);
    const bf16* w = dbg_tiled_weights(pool, w_f32_nk, N, K, st);
    const DbgPlanes r = resid_f32 ? dbg_planes_from(pool, resid_f32, (int64_t)s.r_rows * N, st) : DbgPlanes{};
    const DbgPlanes c = s.out_kind == 1 ? dbg_planes_from(pool, c_f32, n_out, st) : DbgPlanes{};
    const int* live = dbg_live(pool, s.m_live, st);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string(who) + ": " + pool.bad);
    GemmParams p = dbg_gemm_params(a, s.lda, w, s.M, N, K, bias, s.act);
    p.w_lo = w + N * K;
    p.amap = dbg_rowmap_dev(s.amap); p.a_index = (const int*)a_index; p.cmap = dbg_rowmap_dev(s.cmap);
    p.engine = s.engine;      // enum Engine (regimes.h)
    p.reverse = s.reverse;    // the tile walk of every second big launch of a forward: the ragged row tile comes FIRST
    p.m_dev = live;
    if (resid_f32) { p.r_hi = r.hi; p.r_lo = r.lo; p.ldr = (int)N; p.rmap = dbg_rowmap_dev(s.rmap); p.r_index = (const int*)r_index; }
    if (s.out_kind == 1) { p.out_kind = OUT_PLANES; p.c_hi = c.hi; p.c_lo = c.lo; p.ldp = s.ldo; }
    else {
        p.out_kind = OUT_F32; p.c_f32 = c_f32; p.ldc = s.ldo;
        if (s.out_kind == 2) { p.hm_rows = s.hm_rows; p.hm_col0 = s.hm_col0; }
    }
    const bool taken = named ? dbg_launch_named(p, s.nsplit, st) : launch_gemm(p, s.nsplit, st);
    return dbg_finish(st, c, c_f32, n_out, taken, std::string(who) + (named ? ": the engine refuses this launch" : ": no engine takes this shape"));
}

// mms_dbg_gemm_bench's `what` beyond the engines of regimes.h: other kernels timed on the same random operands (tools/gemm_bench.py)
enum BenchMode : int {
    BENCH_MX = 50,               // lab: the fp16 + MX-fp8 "1.5 pass" engine (gemm_mx.hip)
    BENCH_MX_HI = 51,            // lab: its high pass alone
    BENCH_MX8 = 52,              // precision mode 4: gemm_mx8_kernel (e4m3 x e4m3)
    BENCH_LN_RESID = 60,         // the LayerNorm kernel with the residual planes on M rows
    BENCH_LN = 61,               // ... without
    BENCH_PROJ_LN_2K = 62,       // N = 768 projection + residual + LayerNorm as two kernels (fp32 tensor in between)
    BENCH_PROJ_LN_FUSED = 63,    // ... as ONE launch with the fused epilogue
};

// n floats on the null stream for the bench hook: uniform [-1, 1), or zeros
float* dbg_random(DbgPool& pool, int64_t n, unsigned seed, int blocks, bool zero = false) {
    float* p = pool.get<float>((size_t)n * 4);
    if (p && !zero) hipLaunchKernelGGL(k_fill_random, dim3(blocks), dim3(256), 0, 0, p, n, seed);
    if (p && zero && hipMemset(p, 0, (size_t)n * 4) != hipSuccess) pool.bad = "hipMemset";
    return p;
}

}  // namespace

extern "C" {

int mms_dbg_gemm(const float* a_f32, int64_t M, int64_t K, int64_t lda, const float* w_f32_nk, int64_t N, const float* bias,
                 const float* resid_f32, int32_t act, int32_t nsplit, int32_t out_planes, int32_t engine, float* c_f32, void* stream) {
    if (!a_f32 || !w_f32_nk || !c_f32 || M <= 0 || N % 128 || K % 64 || lda < K || lda % 32 || engine < 0) return refuse("mms_dbg_gemm: bad argument");
    // engine: ENG_AUTO = the per-shape choice of the forward; else ONE named engine
    const mms_rows_spec s = dbg_dense_spec(M, N, K, lda, act, nsplit, engine, out_planes ? 1 : 0);
    return dbg_gemm_run("mms_dbg_gemm", false, s, M * N, a_f32, nullptr, w_f32_nk, bias, resid_f32, nullptr, c_f32, (hipStream_t)stream);
}

// mms_dbg_gemm with the two fields of a forward's launches it leaves at their defaults: a device-side live-row count (m_live >= 0: rows >= min(M, m_live)
// are not written; the output is zero-filled first) and the head-major fp32 layout of the QKV projections (out_kind 2: c_f32 [N / 64][M][64]).
// out_kind 0: plain fp32 [M][N]; 1: split planes, joined to fp32 [M][N].  reverse: GemmParams::reverse (tiles walked from the last row tile down).
// Two-pass bf16 planes (precision mode 2), no residual.
int mms_dbg_gemm_ex(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act, int32_t out_kind,
                    int32_t engine, int64_t m_live, int32_t reverse, float* c_f32, void* stream) {
    if (!a_f32 || !w_f32_nk || !c_f32 || M <= 0 || M > (1 << 24) || N % 128 || K % 64 || engine < 0 || out_kind < 0 || out_kind > 2 || (reverse & ~1) || (out_kind == 2 && N % 64))
        return refuse("mms_dbg_gemm_ex: bad argument");
    hipStream_t st = (hipStream_t)stream;
    mms_rows_spec s = dbg_dense_spec(M, N, K, K, act, 2, engine, out_kind);
    s.m_live = (int32_t)m_live; s.reverse = reverse;
    DBG_TRY(hipMemsetAsync(c_f32, 0, (size_t)M * N * 4, st));
    return dbg_gemm_run("mms_dbg_gemm_ex", false, s, M * N, a_f32, nullptr, w_f32_nk, bias, nullptr, nullptr, c_f32, st);
}

// the caller's pre-filled image survives where nothing is written, and survives entirely on a refusal
int mms_dbg_gemm_rows(const mms_rows_spec* s, const float* a_f32, const int32_t* a_index, const float* w_f32_nk, const float* bias, const float* resid_f32,
                      const int32_t* r_index, float* c_f32, void* stream) {
    if (!s || !a_f32 || !w_f32_nk || !c_f32 || s->M <= 0 || s->M > (1 << 24) || s->N <= 0 || s->N % 128 || s->K <= 0 || s->K % 64 || s->nsplit < 1 || s->nsplit > 3 ||
        s->act < ACT_NONE || s->act > ACT_TANH || (s->reverse & ~1) || s->a_rows <= 0 || s->lda < s->K || s->lda % 32 || (r_index && !resid_f32))
        return refuse("mms_dbg_gemm_rows: bad argument");
    // every row (and head-major block) a logical row r < M can address, BEFORE anything is launched: a slip in a caller's spec ends here, not in a fault
    if (!dbg_rows_inside(s->amap, a_index, s->M, s->a_rows)) return refuse("mms_dbg_gemm_rows: an A row lies outside a_f32");
    if (resid_f32 && !dbg_rows_inside(s->rmap, r_index, s->M, s->r_rows)) return refuse("mms_dbg_gemm_rows: a residual row lies outside resid_f32");
    const int64_t n_out = dbg_out_elems(s->out_kind, s->M, s->N, s->ldo, s->c_rows, s->cmap, s->hm_rows, s->hm_col0, s->hm_blocks);
    if (n_out < 0) return refuse("mms_dbg_gemm_rows: an output row lies outside c_f32 (or bad output fields)");
    return dbg_gemm_run("mms_dbg_gemm_rows", true, *s, n_out, a_f32, a_index, w_f32_nk, bias, resid_f32, r_index, c_f32, (hipStream_t)stream);
}

int mms_dbg_gemm_f8(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act,
                    int32_t out_f8, float* c_f32, void* stream) {
    return mms_dbg_gemm_f8_rows(a_f32, M, K, w_f32_nk, N, bias, act, out_f8, c_f32, nullptr, stream);
}
int mms_dbg_gemm_f8_rows(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act,
                         int32_t out_f8, float* c_f32, const mms_rows_spec* rows, void* stream) {
    if (!a_f32 || !w_f32_nk || !c_f32 || M <= 0 || M > (1 << 24) || N % 256 || K % 128) return refuse("mms_dbg_gemm_f8: bad argument (N % 256, K % 128)");
    // rows: the caller's pre-filled physical image with a row map, a live count, a row stride and (fp32) the head-major layout; checked before anything is launched
    const int32_t ident[3] = {0, 0, 0};
    int64_t n_out = M * N;
    if (rows) {
        if (out_f8 && (rows->out_kind != 0 || rows->ldo % 32)) return refuse("mms_dbg_gemm_f8: e4m3 output is row-major, ldo % 32 == 0");
        n_out = dbg_out_elems(rows->out_kind, M, N, rows->ldo, rows->c_rows, rows->cmap, rows->hm_rows, rows->hm_col0, rows->hm_blocks);
        if (n_out < 0 || rows->out_kind == 1) return refuse("mms_dbg_gemm_f8: an output row lies outside the image (or bad output fields)");
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t Mp = (M + 255) / 256 * 256;
    const int32_t m_live = rows ? rows->m_live : -1;
    DbgPool pool;
    unsigned char* a8 = pool.get<unsigned char>((size_t)Mp * K);
    unsigned char* w8 = pool.get<unsigned char>((size_t)N * K);
    unsigned* ws4 = pool.get<unsigned>((size_t)N);
    unsigned char* c8 = out_f8 ? pool.get<unsigned char>((size_t)n_out) : nullptr;
    const int* live = dbg_live(pool, m_live, st);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_gemm_f8: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(a8, 0, (size_t)Mp * K, st));
    launch_f32_to_f8(a_f32, a8, M * K, st);
    launch_quant_rows_f8(w_f32_nk, w8, nullptr, ws4, (int)N, (int)K, st);
    GemmParams p{};
    p.a8 = a8; p.lda = (int)K; p.amap = RowMap{0, 0, 0}; p.cmap = dbg_rowmap_dev(rows ? rows->cmap : ident); p.rmap = RowMap{0, 0, 0};
    p.w8 = w8; p.w8_scale4 = ws4; p.bias = bias; p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act;
    p.m_dev = live;
    const int ldo = rows ? rows->ldo : (int)N;
    if (out_f8) {
        if (rows) launch_f32_to_f8(c_f32, c8, n_out, st);      // the pre-filled image as bytes
        p.out_kind = OUT_F8; p.c_f8 = c8; p.ldf8 = ldo;
    } else {
        p.out_kind = OUT_F32; p.c_f32 = c_f32; p.ldc = ldo;
        if (rows && rows->out_kind == 2) { p.hm_rows = rows->hm_rows; p.hm_col0 = rows->hm_col0; }
    }
    const bool taken = launch_gemm_mx8(p, st);
    if (taken && out_f8) launch_f8_to_f32(c8, c_f32, n_out, st);
    return dbg_finish(st, DbgPlanes{}, nullptr, 0, taken, "mms_dbg_gemm_f8: shape not supported");
}

#ifdef MMS_LAB
// precision mode 5 GEMM (gemm_mx.hip) on fp32 operands: A goes through the h3 split (fp16 + e4m3 residual), W through the weight
// preparation of the forward (fp16 copy + e4m3 copy + per-channel scales); out_h3: the result leaves as h3 planes (and is converted back)
int mms_dbg_gemm_mx(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, int64_t N, const float* bias, int32_t act,
                    int32_t out_h3, float* c_f32, void* stream) {
    if (!a_f32 || !w_f32_nk || !c_f32 || M <= 0 || N % 256 || K % 256) return refuse("mms_dbg_gemm_mx: bad argument (N % 256, K % 256)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t Mp = (M + 255) / 256 * 256;
    DbgPool pool;
    f16* a16 = pool.get<f16>((size_t)Mp * K * 2);
    unsigned char* a8 = pool.get<unsigned char>((size_t)Mp * K);
    f16* w16 = pool.get<f16>((size_t)N * K * 2);
    unsigned char* w8 = pool.get<unsigned char>((size_t)N * K);
    unsigned* ws4 = pool.get<unsigned>((size_t)N);
    float* cs = pool.get<float>((size_t)N * 4);
    f16* c16 = out_h3 ? pool.get<f16>((size_t)M * N * 2) : nullptr;
    unsigned char* c8 = out_h3 ? pool.get<unsigned char>((size_t)M * N) : nullptr;
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_gemm_mx: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(a16, 0, (size_t)Mp * K * 2, st)); DBG_TRY(hipMemsetAsync(a8, 0, (size_t)Mp * K, st));
    launch_split_h3(a_f32, a16, a8, M * K, st);
    launch_prep_w_mx(w_f32_nk, w16, w8, ws4, cs, (int)N, (int)K, st);
    GemmParams p{};
    p.a_hi = (const bf16*)a16; p.a8 = a8; p.lda = (int)K; p.amap = RowMap{0, 0, 0}; p.cmap = RowMap{0, 0, 0}; p.rmap = RowMap{0, 0, 0};
    p.w = (const bf16*)w16; p.w8 = w8; p.w8_scale4 = ws4; p.col_scale = cs; p.bias = bias; p.M = (int)M; p.N = (int)N; p.K = (int)K; p.act = act;
    if (out_h3) { p.out_kind = OUT_H3; p.c_h16 = c16; p.c_l8 = c8; p.ldh = (int)N; }
    else { p.out_kind = OUT_F32; p.c_f32 = c_f32; p.ldc = (int)N; }
    if (!launch_gemm_mx(p, st)) return refuse("mms_dbg_gemm_mx: shape not supported");
    if (out_h3) launch_h3_to_f32(c16, c8, c_f32, M * N, st);
    return dbg_finish(st);
}

unsigned long long* g_ln_dbg = nullptr;   // lab: device buffer for the per-tile phase stamps of the next mms_dbg_gemm_ln (tools/ln_trace.py)
int mms_lab_ln_trace(unsigned long long* dev_buf) { g_ln_dbg = dev_buf; return MMS_OK; }
#endif  // MMS_LAB

int mms_dbg_gemm_ln(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                    const float* gamma, const float* beta, int32_t flags, float* c_f32, int32_t* mode_out, void* stream) {
    const int64_t N = H;
    const bool f8 = flags & 1, reverse = flags & 2;      // bit 0: fp8 operands (refused below); bit 1: GemmParams::reverse, the last row panel in the FIRST round
    if (!a_f32 || !w_f32_nk || !resid_f32 || !gamma || !beta || !c_f32 || M <= 0 || K % 128 || (flags & ~3)) return refuse("mms_dbg_gemm_ln: bad argument");
    if (f8) return refuse("mms_dbg_gemm_ln: the fused LayerNorm epilogue exists for the bf16 two-pass engine only");
    hipStream_t st = (hipStream_t)stream;
    DbgPool pool;
    const DbgPlanes a = dbg_planes_from(pool, a_f32, M * K, st);
    const bf16* w = dbg_tiled_weights(pool, w_f32_nk, N, K, st);
    const DbgPlanes r = dbg_planes_from(pool, resid_f32, M * N, st);
    const DbgPlanes c = dbg_planes(pool, M * N);
    float* t = pool.get<float>((size_t)M * N * 4);
    float* stats = pool.get<float>((size_t)(M + 256) * 48);
    int* ctl = pool.get<int>(8);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_gemm_ln: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(stats, 0, (size_t)(M + 256) * 48, st)); DBG_TRY(hipMemsetAsync(ctl, 0, 8, st));
    GemmParams p = dbg_gemm_params(a, K, w, M, N, K, bias, ACT_NONE);
    p.r_hi = r.hi; p.r_lo = r.lo; p.ldr = (int)N;
    p.c_hi = c.hi; p.c_lo = c.lo; p.ldp = (int)N;
    p.out_kind = OUT_F32; p.c_f32 = t; p.ldc = (int)N;
    p.ln_gamma = gamma; p.ln_beta = beta; p.ln_stats = stats; p.ln_tag = 0x5EED0001u; p.ln_ctl = ctl;
    p.reverse = reverse;
#ifdef MMS_LAB
    p.ln_dbg = g_ln_dbg;
#endif
    if (!launch_gemm_pp_ln(p, 2, st)) return refuse("mms_dbg_gemm_ln: shape not supported");
    LnResid res;
    res.hi = r.hi; res.lo = r.lo; res.ld = (int)N; res.skip = ctl + 1; res.reverse = reverse;
    launch_ln_to_planes(t, (int)N, gamma, beta, c.hi, c.lo, (int)N, (int)M, st, nullptr, res);
    int ctl_h[2] = {0, 0};
    DBG_TRY(hipMemcpyAsync(ctl_h, ctl, 8, hipMemcpyDeviceToHost, st));
    if (int rc = dbg_finish(st, c, c_f32, M * N)) return rc;
    if (mode_out) *mode_out = ctl_h[1];
    return MMS_OK;
}

// out = LayerNorm(A W^T + bias + resid) over N = 768 on the SMALL-launch route: the register-staged tile engine with the contraction split
// `splits` ways (1, or a divisor of K / 64: fp32 partials) and the LayerNorm kernel that sums the partials, adds bias + residual and normalises
// -- the kernel pair proj_ln() launches for calls of a few hundred pairs
int mms_dbg_proj_ln_splitk(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                           const float* gamma, const float* beta, int32_t splits, float* c_f32, void* stream) {
    return mms_dbg_proj_ln_splitk_rows(a_f32, M, K, w_f32_nk, bias, resid_f32, gamma, beta, splits, c_f32, nullptr, nullptr, nullptr, stream);
}
int mms_dbg_proj_ln_splitk_rows(const float* a_f32, int64_t M, int64_t K, const float* w_f32_nk, const float* bias, const float* resid_f32,
                                const float* gamma, const float* beta, int32_t splits, float* c_f32, const mms_rows_spec* rows, const int32_t* a_index,
                                const int32_t* r_index, void* stream) {
    const int64_t N = H;
    const bool skinny_parts = splits < 0;      // negative: the partials come from gemm_skinny.hip (K slices dealt to workgroups; M <= 512) instead of the tile engine
    if (skinny_parts) splits = -splits;
    if (!a_f32 || !w_f32_nk || !resid_f32 || !gamma || !beta || !c_f32 || M <= 0 || M > (1 << 24) || splits == 0 || K % (64 * splits))
        return refuse("mms_dbg_proj_ln_splitk_rows: bad argument");
    // rows: A [a_rows][lda] through amap / a_index, the residual [r_rows][768] through rmap / r_index -- every row of r < M inside its buffer, or nothing is launched
    const int32_t ident[3] = {0, 0, 0};
    const int64_t a_rows = rows ? rows->a_rows : M, lda = rows ? rows->lda : K, r_rows = rows ? rows->r_rows : M;
    if ((!rows && (a_index || r_index)) || lda < K || lda % 32 || !dbg_rows_inside(rows ? rows->amap : ident, a_index, M, a_rows) ||
        !dbg_rows_inside(rows ? rows->rmap : ident, r_index, M, r_rows))
        return refuse("mms_dbg_proj_ln_splitk_rows: a row lies outside its buffer (or bad lda)");
    hipStream_t st = (hipStream_t)stream;
    DbgPool pool;
    const DbgPlanes a = dbg_planes_from(pool, a_f32, a_rows * lda, st);
    const bf16* w = dbg_tiled_weights(pool, w_f32_nk, N, K, st);
    const DbgPlanes r = dbg_planes_from(pool, resid_f32, r_rows * N, st);
    const DbgPlanes c = dbg_planes(pool, M * N);
    float* parts = pool.get<float>((size_t)splits * M * N * 4);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_proj_ln_splitk: ") + pool.bad);
    GemmParams p = dbg_gemm_params(a, lda, w, M, N, K, splits == 1 ? bias : nullptr, ACT_NONE);
    p.amap = dbg_rowmap_dev(rows ? rows->amap : ident); p.a_index = (const int*)a_index;
    p.out_kind = OUT_F32; p.c_f32 = parts; p.ldc = (int)N;
    p.k_splits = splits; p.c_split_stride = (long long)M * N;
    p.engine = skinny_parts && splits > 1 ? ENG_SKINNY_PARTS : ENG_TILE;
    const bool taken = launch_gemm(p, 2, st);
    LnResid res;
    res.hi = r.hi; res.lo = r.lo; res.ld = (int)N; res.rmap = dbg_rowmap_dev(rows ? rows->rmap : ident); res.r_index = (const int*)r_index;
    if (splits > 1) { res.nparts = splits; res.part_stride = p.c_split_stride; res.bias = bias; }
    if (taken) launch_ln_to_planes(parts, (int)N, gamma, beta, c.hi, c.lo, (int)N, (int)M, st, nullptr, res);
    return dbg_finish(st, c, c_f32, M * N, taken, "mms_dbg_proj_ln_splitk_rows: no engine takes this shape");
}

// GEMM micro-benchmark on random operands: returns the average kernel time (ms) over `iters` launches.  Everything runs on the null stream.
int mms_dbg_gemm_bench(int64_t M, int64_t N, int64_t K, int32_t nsplit, int32_t act, int32_t out_planes, int32_t resid,
                       int32_t what, int32_t iters, float* ms_out) {      // what: an Engine (regimes.h) or a BenchMode above
    if (M <= 0 || N % 128 || K % 64 || iters <= 0 || !ms_out) return refuse("mms_dbg_gemm_bench: bad argument");
    const bool mx8 = what == BENCH_MX8, mx = what == BENCH_MX || what == BENCH_MX_HI, proj_ln = what == BENCH_PROJ_LN_2K || what == BENCH_PROJ_LN_FUSED;
    if (mx8 && (N % 256 || K % 128 || resid)) return refuse("mms_dbg_gemm_bench: mx8 engine needs N % 256 == 0, K % 128 == 0, no residual");
    if (mx && (N % 256 || K % 256 || resid)) return refuse("mms_dbg_gemm_bench: mx engine needs N % 256 == 0, K % 256 == 0, no residual");
    if (proj_ln && (N != H || nsplit != 2)) return refuse("mms_dbg_gemm_bench: the projection + LayerNorm modes need N == 768, nsplit == 2");
#ifdef MMS_LAB
    const bool zero_fill = getenv("MMS_GB_ZERO") != nullptr;   // DVFS probe: zero operands draw less power (never a bench number)
#else
    const bool zero_fill = false;
#endif
    DbgPool pool;
    DbgEvents ev;
    float* af = dbg_random(pool, M * K, 1u, 4096, zero_fill);
    float* wf = dbg_random(pool, N * K, 2u, 4096, zero_fill);
    float* rf = dbg_random(pool, M * N, 3u, 4096);
    float* bias = dbg_random(pool, N, 4u, 64);
    float* cf = pool.get<float>((size_t)M * N * 4);
    const DbgPlanes a = af ? dbg_planes_from(pool, af, M * K, 0) : DbgPlanes{};
    const bf16* w = wf ? dbg_tiled_weights(pool, wf, N, K, 0) : nullptr;
    const DbgPlanes r = rf ? dbg_planes_from(pool, rf, M * N, 0) : DbgPlanes{};
    const DbgPlanes c = dbg_planes(pool, M * N);
    // BENCH_MX8 / BENCH_MX / BENCH_MX_HI: the same random operands as e4m3 bytes / as h3 planes with the weight preparation of gemm_mx.hip
    const int64_t Mp = (M + 255) / 256 * 256;
    unsigned char* a8 = mx8 || mx ? pool.get<unsigned char>((size_t)Mp * K) : nullptr;
    unsigned char* w8 = mx8 || mx ? pool.get<unsigned char>((size_t)N * K) : nullptr;
    unsigned* ws4 = mx8 || mx ? pool.get<unsigned>((size_t)N) : nullptr;
    unsigned char* c8 = mx8 || mx ? pool.get<unsigned char>((size_t)M * N) : nullptr;
    f16* a16 = mx ? pool.get<f16>((size_t)Mp * K * 2) : nullptr;
    f16* w16 = mx ? pool.get<f16>((size_t)N * K * 2) : nullptr;
    f16* c16 = mx ? pool.get<f16>((size_t)M * N * 2) : nullptr;
    float* cs = mx ? pool.get<float>((size_t)N * 4) : nullptr;
    // BENCH_PROJ_LN_2K / BENCH_PROJ_LN_FUSED: the statistics and control words of the fused epilogue (gemm_pp_ln.h); both modes leave split planes
    float* ln_stats = proj_ln ? pool.get<float>((size_t)(M + 256) * 48) : nullptr;
    int* ln_ctl = proj_ln ? pool.get<int>(8) : nullptr;
    unsigned ln_tag = 0x1000u;
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_gemm_bench: ") + pool.bad);
    DBG_TRY(ev.create());
    GemmParams p = dbg_gemm_params(a, K, w, M, N, K, bias, act);
    p.w_lo = w + N * K;
    if (resid) { p.r_hi = r.hi; p.r_lo = r.lo; p.ldr = (int)N; }
    if (out_planes) { p.out_kind = OUT_PLANES; p.c_hi = c.hi; p.c_lo = c.lo; p.ldp = (int)N; }
    else { p.out_kind = OUT_F32; p.c_f32 = cf; p.ldc = (int)N; }
    p.engine = engine_is_named(what) ? what : ENG_AUTO;
    GemmParams pm = p;
    pm.w_lo = nullptr;
    if (mx8) {
        DBG_TRY(hipMemset(a8, 0, (size_t)Mp * K));
        launch_f32_to_f8(af, a8, M * K, 0);
        launch_quant_rows_f8(wf, w8, nullptr, ws4, (int)N, (int)K, 0);
        pm.a8 = a8; pm.w8 = w8; pm.w8_scale4 = ws4;
        if (out_planes) { pm.out_kind = OUT_F8; pm.c_f8 = c8; pm.ldf8 = (int)N; }
    } else if (mx) {
        DBG_TRY(hipMemset(a16, 0, (size_t)Mp * K * 2)); DBG_TRY(hipMemset(a8, 0, (size_t)Mp * K));
        launch_split_h3(af, a16, a8, M * K, 0);
        launch_prep_w_mx(wf, w16, w8, ws4, cs, (int)N, (int)K, 0);
        pm.a_hi = (const bf16*)a16; pm.a8 = a8; pm.w = (const bf16*)w16; pm.w8 = w8; pm.w8_scale4 = ws4; pm.col_scale = cs;
        if (out_planes) { pm.out_kind = OUT_H3; pm.c_h16 = c16; pm.c_l8 = c8; pm.ldh = (int)N; }
    }
    if (proj_ln) DBG_TRY(hipMemset(ln_stats, 0, (size_t)(M + 256) * 48));
    auto run = [&]() {
        if (proj_ln) {      // the N = 768 projection + residual + LayerNorm as two kernels (fp32 tensor in between) / as ONE launch with the fused epilogue
            GemmParams q = p;
            q.out_kind = OUT_F32; q.c_f32 = cf; q.ldc = H; q.r_hi = nullptr; q.r_lo = nullptr;
            LnResid res;
            res.hi = r.hi; res.lo = r.lo; res.ld = H;
            if (what == BENCH_PROJ_LN_2K) {
                launch_gemm(q, 2, 0);
                launch_ln_to_planes(cf, H, bias, bias, c.hi, c.lo, H, (int)M, 0, nullptr, res);
                return true;
            }
            q.r_hi = r.hi; q.r_lo = r.lo; q.ldr = H; q.c_hi = c.hi; q.c_lo = c.lo; q.ldp = H;
            q.ln_gamma = bias; q.ln_beta = bias; q.ln_stats = ln_stats; q.ln_tag = ++ln_tag; q.ln_ctl = ln_ctl;
            if (hipMemsetAsync(ln_ctl, 0, 8, 0) != hipSuccess) return false;
            if (!launch_gemm_pp_ln(q, 2, 0)) return false;
            res.skip = ln_ctl + 1;
            launch_ln_to_planes(cf, H, bias, bias, c.hi, c.lo, H, (int)M, 0, nullptr, res);
            return true;
        }
        if (what == BENCH_LN_RESID || what == BENCH_LN) {     // the LayerNorm kernel (with / without the residual planes) on M rows: HBM-bound, 9 / 6 KB per row
            if (N != H) return false;
            LnResid res;
            if (what == BENCH_LN_RESID) { res.hi = r.hi; res.lo = r.lo; res.ld = H; }
            launch_ln_to_planes(cf, H, bias, bias, c.hi, c.lo, H, (int)M, 0, nullptr, res);
            return true;
        }
        if (mx8) return launch_gemm_mx8(pm, 0);
#ifdef MMS_LAB
        if (what == BENCH_MX_HI) return launch_gemm_mx_hi_only(pm, 0);
        if (mx) return launch_gemm_mx(pm, 0);
#else
        if (mx) return false;     // 50 / 51: lab build only
#endif
        launch_gemm(p, nsplit, 0);
        return true;
    };
    if (!run()) return refuse("mms_dbg_gemm_bench: engine / mode not available");
    run();
    DBG_TRY(hipEventRecord(ev.e[0], 0));
    for (int i = 0; i < iters; ++i) run();
    DBG_TRY(hipEventRecord(ev.e[1], 0));
    DBG_TRY(hipEventSynchronize(ev.e[1]));
    float ms = 0;
    DBG_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    *ms_out = ms / iters;
    DBG_TRY(hipGetLastError());
    return MMS_OK;
}

int mms_dbg_attention(const float* q, const float* k, const float* v, int64_t B, int32_t Sq, int32_t Sk, const float* key_add,
                      float* out_f32, void* stream) {
    if (!q || !k || !v || !out_f32 || B <= 0 || Sq <= 0 || Sk <= 0 || Sq > 48 || Sk > 48) return refuse("mms_dbg_attention: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = B * Sq * H;
    DbgPool pool;
    const DbgPlanes o = dbg_planes(pool, n);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_attention: ") + pool.bad);
    AttnParams a{};
    a.q = q; a.ldq = H; a.k = k; a.v = v; a.ldkv = H; a.hs_q = a.hs_kv = MMS_HEAD_DIM; a.q_base = 0; a.Sq = Sq; a.kv_base = 0; a.Sk = Sk;
    a.key_add = key_add; a.o_hi = o.hi; a.o_lo = o.lo; a.ldo = H; a.B = (int)B;
    if (!launch_attention(a, st)) return refuse("mms_dbg_attention: no kernel for this (Sq, Sk)");
    return dbg_finish(st, o, out_f32, n);
}

int mms_dbg_qkv_attn(const float* x, int64_t rows1, int64_t rows2, const int32_t* off1, const int32_t* cnt1, const int32_t* off2, const int32_t* cnt2,
                     int64_t n_pairs, int32_t S1, int32_t S2, const float* w_qkv, const float* bias_qkv, const float* key_add1, const float* key_add2,
                     int32_t mode, float* ctx_f32, int32_t* n_sub_out, void* stream) {
    if (!x || !w_qkv || !bias_qkv || !ctx_f32 || rows1 <= 0 || rows2 < 0 || n_pairs <= 0 || S1 <= 0 || (rows2 > 0 && S2 <= 0) || (mode != 1 && mode != 2) ||
        (off1 == nullptr) != (cnt1 == nullptr) || (off2 == nullptr) != (cnt2 == nullptr)) return refuse("mms_dbg_qkv_attn: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const bool cross = rows2 > 0;
    const int64_t rows = rows1 + rows2;
    DbgPool pool;
    const DbgPlanes xp = dbg_planes_from(pool, x, rows * H, st);
    const DbgPlanes cp = dbg_planes(pool, rows * H);
    bf16* wt = pool.get<bf16>((size_t)3 * H * H * 2);
    float* whm = pool.get<float>((size_t)3 * H * H * 4);
    float* bhm = pool.get<float>((size_t)3 * H * 4);
    int4* sub = pool.get<int4>((size_t)(n_pairs + 2) * sizeof(int4));
    int4* sub2 = pool.get<int4>((size_t)(n_pairs + 2) * sizeof(int4));
    int* nsub = pool.get<int>(16);
    int* rec = pool.get<int>((size_t)(n_pairs + 2) * 4);
    int* scratch = pool.get<int>((size_t)qkv_plan_scratch_ints((int)n_pairs) * 4);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_qkv_attn: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(cp.hi, 0, (size_t)rows * H * 4, st));
    // [Wq; Wk; Wv] (torch Linear rows) -> head-major [12][Q 64 | K 64 | V 64] rows, as load_att() builds it for the scorers
    for (int hd = 0; hd < MMS_HEADS; ++hd)
        for (int i = 0; i < 3; ++i) {
            const size_t src = (size_t)i * H + (size_t)hd * MMS_HEAD_DIM, dst = ((size_t)hd * 3 + i) * MMS_HEAD_DIM;
            DBG_TRY(hipMemcpyAsync(whm + dst * H, w_qkv + src * H, (size_t)MMS_HEAD_DIM * H * 4, hipMemcpyDeviceToDevice, st));
            DBG_TRY(hipMemcpyAsync(bhm + dst, bias_qkv + src, (size_t)MMS_HEAD_DIM * 4, hipMemcpyDeviceToDevice, st));
        }
    launch_tile_weights(whm, wt, nullptr, 3 * H, H, st);
    bool planned;
    if (cross) planned = launch_qkv_cross_plan((const int*)off1, (const int*)cnt1, (const int*)off2, (const int*)cnt2, (int)n_pairs, S1, S2, sub, sub2, nsub, 2, st, rec, scratch);
    else planned = launch_qkv_tile_plan((const int*)off1, (const int*)cnt1, (int)n_pairs, S1, sub, nsub, 2, st, rec, scratch);
    if (!planned) return refuse("mms_dbg_qkv_attn: too many pairs for one plan");
    QkvAttnParams q{};
    q.a_hi = xp.hi; q.lda = H; q.w = wt; q.bias = bhm; q.K = H;
    q.sub = sub; q.n_sub = nsub; q.pair_rec = rec; q.pair_off = (const int*)off1; q.pair_cnt = (const int*)cnt1; q.S = S1;
    q.key_add = key_add1; q.o_hi = cp.hi; q.o_lo = cp.lo; q.ldo = H; q.M = (int)rows1; q.fast = mode == 2;
    if (cross) { q.sub2 = sub2; q.pair_off2 = (const int*)off2; q.pair_cnt2 = (const int*)cnt2; q.S2 = S2; q.key_add2 = key_add2; q.row0_b = rows1; q.M2 = (int)rows2; }
    if (!launch_qkv_attn(q, st)) return refuse("mms_dbg_qkv_attn: shape not supported by this route");
    if (int rc = dbg_finish(st, cp, ctx_f32, rows * H)) return rc;
    if (n_sub_out) DBG_TRY(hipMemcpy(n_sub_out, nsub, 4, hipMemcpyDeviceToHost));
    return MMS_OK;
}

int mms_dbg_layernorm(const float* x, const float* gamma, const float* beta, int64_t M, float* out_f32, void* stream) {
    if (!x || !gamma || !beta || !out_f32 || M <= 0) return refuse("mms_dbg_layernorm: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DbgPool pool;
    const DbgPlanes o = dbg_planes(pool, M * H);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_layernorm: ") + pool.bad);
    launch_ln_to_planes(x, H, gamma, beta, o.hi, o.lo, H, (int)M, st);
    return dbg_finish(st, o, out_f32, M * H);
}

// ---- hooks of the ragged attention, plan, de-duplication and row kernels: the launch forms the forwards use (att_block, last_block_cls, the pack plans) ----
int mms_dbg_attention_ex(const float* q, const float* k, const float* v, int64_t B, int32_t Sq, int32_t Sk, int64_t q_rows, int64_t kv_rows,
                         const int32_t* q_off, const int32_t* q_cnt, const int32_t* kv_off, const int32_t* kv_cnt, const float* key_add,
                         int32_t flags, float* out_f32, void* stream) {
    const bool hm = flags & 1, cls = flags & 4, f8 = flags & 8;
    if (!q || !k || !v || !out_f32 || B <= 0 || B > (1 << 20) || Sq <= 0 || Sk <= 0 || Sq > 48 || Sk > 48 || q_rows <= 0 || kv_rows <= 0 || (flags & ~15) ||
        (q_off == nullptr) != (q_cnt == nullptr) || (kv_off == nullptr) != (kv_cnt == nullptr) || (cls && (Sq != 1 || q_off || q_rows != B)))
        return refuse("mms_dbg_attention_ex: bad argument");
    if ((q_off ? !dbg_pairs_ok(q_off, q_cnt, B, Sq, q_rows) : (!cls && B * Sq > q_rows)) || (kv_off ? !dbg_pairs_ok(kv_off, kv_cnt, B, Sk, kv_rows) : B * Sk > kv_rows))
        return refuse("mms_dbg_attention_ex: a pair's rows lie outside its stream");
    hipStream_t st = (hipStream_t)stream;
    const int64_t out_rows = cls ? B : q_rows, n = out_rows * H;
    DbgPool pool;
    const DbgPlanes o = dbg_planes(pool, n);
    unsigned char* o8 = pool.get<unsigned char>((size_t)n);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_attention_ex: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(o.hi, 0, (size_t)n * 4, st));
    DBG_TRY(hipMemsetAsync(o8, 0, (size_t)n, st));
    AttnParams a{};
    a.q = q; a.k = k; a.v = v;
    if (cls) { a.ldq = H; a.hs_q = MMS_HEAD_DIM; a.q_stride = 1; a.o_compact = 1; }                    // last_block_cls
    else if (hm) { a.ldq = MMS_HEAD_DIM; a.hs_q = q_rows * MMS_HEAD_DIM; }                            // attn_q
    else { a.ldq = H; a.hs_q = MMS_HEAD_DIM; }
    if (hm) { a.ldkv = MMS_HEAD_DIM; a.hs_kv = kv_rows * MMS_HEAD_DIM; }                              // attn_kv
    else { a.ldkv = H; a.hs_kv = MMS_HEAD_DIM; }
    a.q_base = 0; a.Sq = Sq; a.kv_base = 0; a.Sk = Sk; a.key_add = key_add;
    a.o_hi = o.hi; a.o_lo = o.lo; a.ldo = H; a.B = (int)B;
    a.q_off = (const int*)q_off; a.q_cnt = (const int*)q_cnt; a.kv_off = (const int*)kv_off; a.kv_cnt = (const int*)kv_cnt;
    a.reverse = (flags & 2) ? 1 : 0;
    if (f8) a.o_f8 = o8;
    if (!launch_attention(a, st)) return refuse("mms_dbg_attention_ex: no kernel for this (Sq, Sk)");
    if (f8) launch_f8_to_f32(o8, out_f32, n, st);
    return f8 ? dbg_finish(st) : dbg_finish(st, o, out_f32, n);
}

int mms_dbg_pack_plan(int32_t kind, int64_t n, int32_t T, const void* in_a, const void* in_b, int32_t* off, int32_t* cnt, int32_t* tok_src, float* key_add,
                      int32_t* off2, int32_t* cnt2, int32_t* src2, float* add2, int32_t* rows_dev, void* stream) {
    const bool two = kind == 0 || kind == 1 || kind == 3;
    if (kind < 0 || kind > 4 || n <= 0 || n > (1 << 22) || T <= 0 || T > 32 || !in_a || (kind != 4 && !in_b) || !off || !cnt || !tok_src || !key_add || !rows_dev ||
        (two && (!off2 || !cnt2 || !src2)) || (kind == 3 && !add2)) return refuse("mms_dbg_pack_plan: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DbgPool pool;
    if (kind == 0) {
        if (!launch_zk_plans_small((const int*)in_a, (const int*)in_b, T, (int)n, cnt2, off2, src2, cnt, off, tok_src, key_add, rows_dev, st))
            return refuse("mms_dbg_pack_plan: the one-block zk plan takes at most 1024 pairs");
    } else if (kind == 1) {
        launch_zk_box_plan((const int*)in_a, (const int*)in_b, T, (int)n, cnt2, off2, src2, rows_dev + 1, st);
        launch_zk_pack_plan((const int*)in_a, (const int*)in_b, T, (int)n, off, cnt, tok_src, key_add, rows_dev, st);
    } else if (kind == 2) {
        int* nz = src2 ? src2 : pool.get<int>((size_t)n * MMS_NBOX * 4);      // the not-all-zero flags come back when the caller asks for them
        if (!nz) return fail(MMS_ERR_HIP, "mms_dbg_pack_plan: hipMalloc");
        launch_lds_pack_plan((const float*)in_a, (const int64_t*)in_b, T, (int)n, nz, off, cnt, tok_src, key_add, rows_dev, st);
    } else {
        launch_lx_pack_plan((const int64_t*)in_a, kind == 3 ? (const float*)in_b : nullptr, T, (int)n, off, cnt, tok_src, key_add, rows_dev,
                            off2, cnt2, src2, add2, rows_dev + 1, st);
    }
    return dbg_finish(st);
}

int mms_dbg_dedup(int32_t kind, const void* ids, const int64_t* mask, int32_t T, int64_t rows, int32_t* count_out, int32_t* index, int32_t* uniq32,
                  int64_t* uniq64, int32_t* rows_of, void* stream) {
    if (kind < 0 || kind > 2 || !ids || rows <= 0 || rows > ((int64_t)1 << 24) || !count_out || !index || (kind == 2 && (!mask || !rows_of || T <= 0)))
        return refuse("mms_dbg_dedup: bad argument");
    hipStream_t st = (hipStream_t)stream;
    int cap = 1024;      // ensure_dedup_ws / lxmert's lq_cap: the smallest power of two >= max(1024, 2 * rows)
    while (cap < 2 * rows) cap <<= 1;
    DbgPool pool;
    int* slots = pool.get<int>((size_t)cap * (kind == 2 ? 2 : 1) * 4);
    int* rep = pool.get<int>((size_t)rows * 4);
    int* uid = pool.get<int>((size_t)rows * 4);
    int* counter = pool.get<int>(16);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_dedup: ") + pool.bad);
    if (kind == 0) launch_label_dedup_i32((const int32_t*)ids, (int)rows, slots, cap, rep, uid, counter, uniq32, uniq64, index, st);
    else if (kind == 1) launch_label_dedup_i64((const int64_t*)ids, (int)rows, slots, cap, rep, uid, counter, uniq32, uniq64, index, st);
    else launch_query_dedup((const int64_t*)ids, mask, T, (int)rows, slots, cap, rep, uid, counter, rows_of, index, st);
    DBG_TRY(hipMemcpyAsync(count_out, counter, 4, hipMemcpyDeviceToHost, st));
    return dbg_finish(st);
}

int mms_dbg_layernorm_ex(const float* x, const float* gamma, const float* beta, int64_t M, const float* resid_f32, int64_t resid_rows, const int32_t* r_index,
                         int64_t m_live, int32_t flags, float* out_f32, float* out_f8, void* stream) {
    return mms_dbg_layernorm_rows(x, gamma, beta, M, resid_f32, resid_rows, r_index, m_live, flags, out_f32, out_f8, nullptr, stream);
}
int mms_dbg_layernorm_rows(const float* x, const float* gamma, const float* beta, int64_t M, const float* resid_f32, int64_t resid_rows, const int32_t* r_index,
                           int64_t m_live, int32_t flags, float* out_f32, float* out_f8, const int32_t* rmap, void* stream) {
    const bool f8 = flags & 2;
    if (!x || !gamma || !beta || !out_f32 || M <= 0 || M > (1 << 24) || (flags & ~7) || (f8 && !out_f8) || (resid_f32 && resid_rows <= 0) || (r_index && !resid_f32) ||
        (rmap && (!resid_f32 || r_index)) || (resid_f32 && !r_index && !rmap && resid_rows < M)) return refuse("mms_dbg_layernorm_ex: bad argument");
    if (rmap && !dbg_rows_inside(rmap, nullptr, M, resid_rows)) return refuse("mms_dbg_layernorm_ex: rmap leaves the residual");
    if (r_index) {
        std::vector<int32_t> ri((size_t)M);
        DBG_TRY(hipMemcpy(ri.data(), r_index, (size_t)M * 4, hipMemcpyDeviceToHost));
        for (int32_t r : ri) if (r < 0 || r >= resid_rows) return refuse("mms_dbg_layernorm_ex: r_index outside the residual");
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = M * H;
    DbgPool pool;
    const DbgPlanes o = dbg_planes(pool, n);
    unsigned char* o8 = pool.get<unsigned char>((size_t)n);
    int* ctl = pool.get<int>(16);
    const DbgPlanes rp = resid_f32 ? dbg_planes_from(pool, resid_f32, resid_rows * H, st) : DbgPlanes{};
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_layernorm_ex: ") + pool.bad);
    DBG_TRY(hipMemsetAsync(o.hi, 0, (size_t)n * 4, st));
    DBG_TRY(hipMemsetAsync(o8, 0, (size_t)n, st));
    const int host_ctl[2] = {(int)m_live, (flags & 4) ? 1 : 0};      // [0] device-side row count, [1] the skip word
    DBG_TRY(hipMemcpyAsync(ctl, host_ctl, 8, hipMemcpyHostToDevice, st));
    LnResid r;
    if (resid_f32) {
        r.hi = rp.hi; r.lo = rp.lo; r.ld = H; r.r_index = (const int*)r_index;
        if (rmap) r.rmap = dbg_rowmap_dev(rmap);
    }
    r.reverse = flags & 1;
    if (f8) r.o_f8 = o8;
    r.skip = ctl + 1;
    launch_ln_to_planes(x, H, gamma, beta, o.hi, o.lo, H, (int)M, st, m_live >= 0 ? ctl : nullptr, r);
    if (f8) launch_f8_to_f32(o8, out_f8, n, st);
    return dbg_finish(st, o, out_f32, n);
}

int mms_dbg_convert(int32_t kind, const void* in, void* out, int64_t n, void* stream) {
    if (kind < 0 || kind > 3 || !in || !out || n <= 0 || n % 32) return refuse("mms_dbg_convert: bad argument (n % 32)");
    hipStream_t st = (hipStream_t)stream;
    DbgPool pool;
    if (kind == 0) launch_f32_to_f8((const float*)in, (unsigned char*)out, n, st);
    else if (kind == 1) launch_f8_to_f32((const unsigned char*)in, (float*)out, n, st);
    else {
        const DbgPlanes pl = dbg_planes_from(pool, (const float*)in, n, st);
        if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_convert: ") + pool.bad);
        if (kind == 2) launch_planes_to_f32(pl.hi, pl.lo, (float*)out, n, st);
        else launch_planes_to_f8(pl.hi, pl.lo, (unsigned char*)out, n, st);
    }
    return dbg_finish(st);
}

int mms_dbg_splitk_reduce(const float* parts, int32_t S, int64_t M, int64_t N, const float* bias, int32_t act, int64_t m_live, int32_t out_kind, int32_t ldo,
                          int64_t c_rows, int32_t hm_rows, int32_t hm_col0, int32_t hm_blocks, float* c_f32, void* stream) {
    if (!parts || !c_f32 || S < 1 || S > 64 || M <= 0 || M > (1 << 24) || N <= 0 || N % 4 || act < ACT_NONE || act > ACT_TANH) return refuse("mms_dbg_splitk_reduce: bad argument");
    const int32_t ident[3] = {0, 0, 0};
    const int64_t n_out = dbg_out_elems(out_kind, M, N, ldo, c_rows, ident, hm_rows, hm_col0, hm_blocks);      // the kernel writes row r to row r: M rows must fit
    if (n_out < 0) return refuse("mms_dbg_splitk_reduce: an output row lies outside c_f32 (or bad output fields)");
    hipStream_t st = (hipStream_t)stream;
    const int32_t host_live = (int32_t)m_live;
    DbgPool pool;
    const DbgPlanes c = out_kind == 1 ? dbg_planes_from(pool, c_f32, n_out, st) : DbgPlanes{};      // the caller's pre-filled image
    const int* live = dbg_live(pool, host_live, st);
    if (pool.bad) return fail(MMS_ERR_HIP, std::string("mms_dbg_splitk_reduce: ") + pool.bad);
    launch_splitk_reduce(parts, S, M * N, (int)M, (int)N, live, bias, act, c.hi ? nullptr : c_f32, ldo, out_kind == 2 ? hm_rows : 0, hm_col0, c.hi, c.lo, ldo, st);
    return dbg_finish(st, c, c_f32, n_out);
}

}  // extern "C"
