// knn.hip -- brute-force kNN (COSINE / IP / L2) over an HBM-resident style bank (gfx950 / MI355X).
//
// Replaces MilvusClient.search on the COSINE collection of the reference
// (/root/reference/milvus/search_embeddings.py:15-22, /root/reference/src/search_milvus.py:140-147).
// Result definition = oracle/knn.py: fp64 score, order (closer first, row asc).  COSINE is what the reference's collection
// uses; IP and L2 (squared distance, Milvus' convention) are the other two metrics of the MilvusClient surface, and L2 with
// k = 1 is the arg-min of the speech tokenizer's vector quantiser (astts/frontend_nets.py).
// Internally every metric is a score S to MAXIMISE: cos, <q,b>, -|q-b|^2; the scan proposes with
// T = <q,b>/|b| (COSINE), <q,b> (IP), <q,b> - |b|^2/2 (L2: the same order as -|q-b|^2 for one query).
// Optional row mask (a Milvus `filter` evaluated by the host, or the rows already returned by earlier passes of a
// k > 32 search): masked rows are never candidates, in the approximate and in the exact path alike.
//
// This file: creation of the handle (the struct and its layout invariants: knn_handle.h), the plan of a search (make_plan: the ONE place
// that decides its query groups and every group's (scan, finish) route), one launcher per step and the C entry
// points.  The kernels: knn_kernels.h.  Appending rows, tombstones and compaction: knn_mutable.hip.  A handle with tombstones
// (h->live) searches as a masked one: its live mask is the row mask, ANDed with the caller's when there is one.
//
// Pipeline (five launches on one stream, no host sync, no allocation):
//   1 knn_prep_queries     fp32 queries -> power-of-two scaled fp16 image + padded fp32 copy + fp64 norms
//   2 knn_scan             fp16 MFMA (32x32x16) scan of the whole bank: S[q][n] ~ <q,b_n>/|b_n|  (HBM-bound)
//   3 knn_select           per query: top-C candidates of S by (score desc, row asc)
//   4 knn_rescore_finalize fp64 cosine of every candidate (one wave each), order by it, emit top-k and
//                          CERTIFY the candidate set: kth exact score > best possible score of any
//                          non-candidate (+ error bound); otherwise queue the query for the exact path
//     (exact path: inside knn_rescore_finalize -- a query that cannot be certified is re-scanned in fp64 by its own block)
//
// HBM layout: the SCAN plane is stored pre-tiled in the order the scan consumes it -- fp16
// [N/32 row tiles][Dp/64 lines][4 k-steps][64 lanes][8 halfs]: one (row tile, line) block is a contiguous 4 KB, one
// wave instruction reads a contiguous 1 KB (lane (r, h) of k-step i holds bank[32*rt + r][64*line + 32*h + 8*i .. +8]),
// so the whole scan is sequential streaming instead of 32 rows 2*Dp bytes apart.  Dp = D rounded up to 64, rows
// padded to a multiple of 32 with zeros.  The EXACT plane (fp64 re-score / exact path) stays row-major [N][Dp]:
// fp16 when the bank is fp16-exact, else fp32.  fp64 row norms [N]; fp32 inverse norms [N].
#include "common.h"
#include "knn_handle.h"
#include "knn_kernels.h"

#include <cstdlib>
#include <cstring>
#include <vector>

// ==========================================================================================
// host side
// ==========================================================================================
using namespace astts;

static_assert(kKnnMaxRows == (int64_t)1024 * kSelSeg, "the row limit of the handle is 1024 selection segments");

namespace {

static constexpr int kPassK = 32;         // hits per pass (the certified top-k kernel keeps k <= 32 of a 64-entry candidate list)
static constexpr int kGemmMinQ = 64;      // query groups below this never take the GEMM scan (one 64-row tile of the ring kernels)

// The experiment switches of the environment, read once per process: the ONE place where this file looks at it.
struct KnnSwitches {
    int ksplit;       // ASTTS_KNN_KSPLIT=n: tuning override of the small-bank K split
    bool no_gemm;     // ASTTS_KNN_NO_GEMM: large query groups keep the register-streaming scan
    bool no_direct;   // ASTTS_KNN_NO_DIRECT: the three-launch form for small banks
    bool no_stream;   // ASTTS_KNN_NO_STREAM_SELECT: per-segment selection + merge for large query groups
    bool no_blocks;   // ASTTS_KNN_NO_BLOCK_MAX: the GEMM scan without its block-maximum epilogue
    bool n_first;     // ASTTS_KNN_GEMM_N_FIRST: the projections' tile order (bank read once per panel), reported on stderr when set
};

const KnnSwitches& knn_switches() {
    static const KnnSwitches sw = [] {
        auto env = [](const char* name) { return getenv(name); };
        const char* ks = env("ASTTS_KNN_KSPLIT");
        return KnnSwitches{ks ? atoi(ks) : 0, env("ASTTS_KNN_NO_GEMM") != nullptr, env("ASTTS_KNN_NO_DIRECT") != nullptr,
                           env("ASTTS_KNN_NO_STREAM_SELECT") != nullptr, env("ASTTS_KNN_NO_BLOCK_MAX") != nullptr,
                           exp_env_int("ASTTS_KNN_GEMM_N_FIRST", 0) != 0};
    }();
    return sw;
}

struct KnnRoute {
    int scan, finish;   // ASTTS_KNN_SCAN_* / ASTTS_KNN_FINISH_*: what a query group launches (include/astts.h; the table: DESIGN.md section 3)
};

struct KnnPlan {
    int qt, rt, ksplit, lines_per_split, tiles, qpad, c, nseg, seg_len;
    int nblk, bm_ld; // 64-row blocks of the bank; block maxima beside the GEMM scan's scores when nblk <= 8192 (one selection segment)
    int passes;      // k > 32: ceil(k / 32) selection + re-score passes over ONE scan, per chunk of <= 256 queries
    bool gemm;       // query groups of >= 64: the scan is a plain GEMM on the ring kernel (MFMA-side regime)
    // query group g is rows [g * gstep, min(nq, (g + 1) * gstep)) of the search.  Its route: `route` with >= 64 rows, else `tail` (which
    // differs from `route` in a GEMM plan only, where it can only be the last group: the register-streaming scan on the one score plane)
    int gstep;
    KnnRoute route, tail;
    const KnnRoute& of(int qg) const { return qg >= kGemmMinQ ? route : tail; }
    // workspace (a function of the bank, nq and k alone: astts_knn_workspace_bytes knows no more; off_nflag is its first word)
    size_t off_nflag, off_qh, off_qf, off_qrow, off_qn, off_qscale, off_spart, off_cidx, off_cs, off_sidx, off_ss, off_mask, off_bmax, total;
};

// The ONE place that decides how a search runs: scan geometry, query groups, every group's (scan, finish) route, workspace layout.
// astts_knn_search launches what it says and astts_knn_route reports it.  masked: a caller's row mask; aligned: the caller's queries
// sit at a 16-byte aligned address; ring_ok: gemm_scan_blockmax_ok for this bank (the ring kernels will carry the block-maximum
// epilogue) -- these three and sw.no_direct / no_stream / no_blocks / n_first choose among routes, never the layout.  tomb: the bank
// has tombstones -- its search is a masked one, and the workspace holds the live mask ANDed with the caller's (up to one per query).
KnnPlan make_plan(int64_t n, int d, int nq, int k, bool masked, bool aligned, const KnnSwitches& sw, bool ring_ok, bool tomb = false) {
    KnnPlan p{};
    masked = masked || tomb;
    const int dp = (int)align_up((size_t)d, 64), nld = (int)align_up((size_t)n, 128);
    const bool single = k <= kPassK && nq <= kMaxQPerPass;      // one pass and one query group: the whole search can finish in one launch
    p.passes = 1;
    if (k > kPassK) {        // multi-pass search: chunks of <= 256 queries, 32 hits per pass, per-query masks of the rows already returned
        p.passes = (int)cdiv(k, kPassK);
        if (nq > kMaxQPerPass) nq = kMaxQPerPass;
        k = kPassK;
    }
    const bool multi = p.passes > 1;
    const int qgroup = nq < kMaxQPerPass ? nq : kMaxQPerPass;
    p.qt = qgroup <= 32 ? 1 : qgroup <= 64 ? 2 : qgroup <= 128 ? 4 : 8;
    p.qpad = p.qt * 32;
    // row tiles per wave: ONE for up to 32 queries -- the scan is an HBM stream and what it needs is waves in flight (48 VGPRs: eight waves
    // per SIMD), not reuse of the query fragments (L2 hits): 100k x 6144, Q = 8: 336 us per search with four tiles per wave (782 blocks of
    // 160 VGPRs), 277 with one; 100k x 768: 75.8 -> 57.6.  Two tiles for 33 .. 63 queries on a large bank (342 against 383 us at Q = 48).
    p.rt = (n >= 16384 && p.qt == 2) ? 2 : 1;
    p.tiles = (int)cdiv(n, 32 * p.rt);
    const int total_lines = dp / 64;
    // K split: a small bank needs it to fill the chip at all (32 tiles x 16 slices); a mid-sized one gets enough slices for ~six blocks per CU
    int ks = (int)cdiv(p.tiles >= 256 ? 1536 : 512, p.tiles);
    int ks_max = total_lines / 4;
    if (ks_max < 1) ks_max = 1;
    if (ks > ks_max) ks = ks_max;
    if (ks < 1) ks = 1;
    if (sw.ksplit > 0) ks = sw.ksplit < ks_max ? sw.ksplit : ks_max;
    p.lines_per_split = (int)cdiv(total_lines, ks);
    p.ksplit = (int)cdiv(total_lines, p.lines_per_split);
    // ... once the GEMM grid fills the chip with 64 x 64 tiles; a small bank keeps the K-split scan (16 blocks x 96 K tiles would crawl).
    // (Round 6: counted in 64-row query tiles, not 128 -- the speech tokenizer's quantiser, 4096 codes x 1280 against groups of 240
    // frames, took the register-streaming scan with eight query tiles per wave at 95 us per group; as a GEMM: see DESIGN section 3.)
    p.gemm = !sw.no_gemm && qgroup >= kGemmMinQ && cdiv(qgroup, 64) * cdiv(n, 64) >= 256;
    if (p.gemm) {        // one score plane; a tail group of < 64 queries runs the register-streaming scan unsplit
        p.ksplit = 1;
        p.lines_per_split = total_lines;
    }
    p.c = k <= 8 ? 16 : 64;
    // selection segments: one block per (query, 8192-score segment), at most 64 segments per query
    p.nseg = (int)cdiv(n, 8192);          // segments of <= kSelSeg scores (staged in LDS by knn_select)
    if (p.nseg < 1) p.nseg = 1;           // (astts_knn_create bounds n so that nseg <= 1024)
    p.seg_len = (int)align_up((size_t)cdiv(n, p.nseg), 64);
    p.nseg = (int)cdiv(n, p.seg_len);
    p.nblk = (int)cdiv(n, 64);
    p.bm_ld = (int)align_up((size_t)p.nblk, 4);         // (the GEMM stores a tile's four maxima of a row as one vector)

    // query groups of <= 256; behind the GEMM scan EQUAL groups (300 queries = 150 + 150, not 256 + a tail of 44 that falls back to the
    // register-streaming scan with eight query tiles per wave: 3.1 ms of a 3.5 ms search at 100k x 6144)
    p.gstep = p.gemm ? (int)cdiv(nq, cdiv(nq, kMaxQPerPass)) : kMaxQPerPass;
    // finish behind the register-streaming scan: one segment and one group = selection + re-score in one launch; one segment = a selection
    // block per query straight into the candidate lists; else one per (query, segment) and a merge
    const bool one_seg = p.nseg == 1;
    p.tail = KnnRoute{ASTTS_KNN_SCAN_REGISTER,
                      one_seg ? (single ? ASTTS_KNN_FINISH_FUSED : ASTTS_KNN_FINISH_SELECT) : ASTTS_KNN_FINISH_SELECT_MERGE};
    p.route = p.tail;
    if (single && nq <= 32 && one_seg && dp == d && (dp & 127) == 0 && dp <= 8192 && !sw.no_direct && aligned) {
        // small bank, one query tile: no preparation launch, the scan reads the caller's fp32 queries (whole 128-float lines of them; the
        // finishing kernel stages the query in its 8192-float segment buffer)
        p.route = p.tail = KnnRoute{ASTTS_KNN_SCAN_DIRECT, ASTTS_KNN_FINISH_FUSED};
    } else if (p.gemm) {
        // S[q][n] = <q, b_n> as one GEMM: activations = the group's queries (row-major fp16), "weights" = the bank's row-major fp16 plane
        // [n][dp]; the LDS-DMA ring kernel runs it at 400+ TFLOP/s where the register-streaming scan (built for the HBM-bound small-Q
        // regime) re-reads the query tile from L2 per bank tile.  Block maxima beside the scores (and the scores scaled by the GEMM's
        // epilogue): unmasked single-pass searches of a long row whose maxima fit one selection segment, on the ring kernels
        const bool blocks = !sw.n_first && !sw.no_blocks && ring_ok && p.nblk <= kSelSeg && !one_seg && !multi && !masked;
        p.route.scan = sw.n_first ? ASTTS_KNN_SCAN_GEMM_N_FIRST : blocks ? ASTTS_KNN_SCAN_GEMM_BLOCKS : ASTTS_KNN_SCAN_GEMM;
        // a long row per query, >= 64 queries: from the maxima, else one streaming block per query
        if (!one_seg) p.route.finish = blocks ? ASTTS_KNN_FINISH_BLOCKS : !sw.no_stream ? ASTTS_KNN_FINISH_STREAM : ASTTS_KNN_FINISH_SELECT_MERGE;
    }

    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    p.off_nflag = take(256);
    p.off_qh = take(sizeof(_Float16) * (align_up((size_t)nq, 32) + 256) * dp);  // whole 32-query tiles (+ one group's tail)
    p.off_qf = take(sizeof(float) * (size_t)nq * dp);
    p.off_qrow = take(p.gemm ? sizeof(_Float16) * (size_t)nq * dp : 16);
    p.off_qn = take(sizeof(double) * (size_t)nq);
    p.off_qscale = take(sizeof(float) * (size_t)nq);
    p.off_spart = take(sizeof(float) * (size_t)p.ksplit * p.qpad * nld);
    p.off_cidx = take(sizeof(int) * (size_t)nq * 64);
    p.off_cs = take(sizeof(float) * (size_t)nq * 64);
    p.off_sidx = take(sizeof(int) * (size_t)kMaxQPerPass * p.nseg * 64);
    p.off_ss = take(sizeof(float) * (size_t)kMaxQPerPass * p.nseg * 64);
    p.off_mask = take(multi || tomb ? (size_t)nq * (size_t)n : 16);
    p.off_bmax = take(p.gemm && p.nblk <= kSelSeg ? sizeof(float) * (size_t)kMaxQPerPass * p.bm_ld : 16);
    p.total = o;
    return p;
}

// the plan under the switches and the ring kernels' state in force (astts_op_gemm_set_ring_mode / ASTTS_GEMM_RING).  ws: the search's
// workspace, where the GEMM's fp16 query rows sit at multiples of 128 bytes (null: a host query, no workspace yet)
KnnPlan plan_search(int64_t n, int d, int nq, int k, bool masked, bool aligned, const void* ws, bool tomb = false) {
    const int qgroup = nq < kMaxQPerPass ? nq : kMaxQPerPass;
    return make_plan(n, d, nq, k, masked, aligned, knn_switches(), gemm_scan_blockmax_ok(qgroup, n, (int)align_up((size_t)d, 64), ws),
                     tomb);
}

template <int QT, int RT, bool DIRECT = false>
int launch_scan(const astts_knn* h, const KnnPlan& p, const _Float16* qh, int nq_group, float* spart,
                const float* qscale_g, hipStream_t st, const float* qdirect = nullptr, int* nflag_clear = nullptr) {
    dim3 grid(p.tiles, p.ksplit);
    size_t lds = (size_t)3 * QT * RT * 16 * 64 * sizeof(float);
    if (lds > 64 * 1024) {
        static bool once = false;
        if (!once) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&knn_scan<QT, RT, DIRECT>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) {
                set_error("hipFuncSetAttribute failed: %s", hipGetErrorString(e));
                return ASTTS_ERR_HIP;
            }
            once = true;
        }
    }
    hipLaunchKernelGGL((knn_scan<QT, RT, DIRECT>), grid, dim3(kScanThreads), lds, st, h->scan, qh,
                       h->inv_norm, spart, h->n, h->dp, h->nld, p.qpad, nq_group, p.lines_per_split, h->bias, qscale_g, qdirect, nflag_clear);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // namespace

namespace astts {

int knn_build_rows(astts_knn* h, const void* rows, int64_t row0, int64_t m, int dtype, int* flags, hipStream_t st) {
    const int rows_per_block = 4;
    dim3 grid((unsigned)cdiv(m, rows_per_block));
    if (dtype == ASTTS_DTYPE_F32)
        hipLaunchKernelGGL((knn_build_bank<float>), grid, dim3(256), 0, st, (const float*)rows, row0, row0 + m, h->d, h->dp, h->scan,
                           h->plane16, h->plane32, h->norm64, h->inv_norm, flags, h->metric, h->bias);
    else
        hipLaunchKernelGGL((knn_build_bank<_Float16>), grid, dim3(256), 0, st, (const _Float16*)rows, row0, row0 + m, h->d, h->dp, h->scan,
                           h->plane16, h->plane32, h->norm64, h->inv_norm, flags, h->metric, h->bias);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

int knn_rescale(astts_knn* h, int64_t row0, int64_t m, hipStream_t st) {
    hipLaunchKernelGGL(knn_rescale_rows, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, st, h->plane32, row0, row0 + m, h->dp, h->scan, h->plane16,
                       h->norm64, h->inv_norm, h->metric);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

// Error bound of the fp16 scan on the cosine scale (DESIGN.md "certification"):
//   query rounded to fp16 (11-bit significand, power-of-two pre-scale): 2^-11 (Cauchy-Schwarz)
//   fp32 accumulation of dp exact products inside the MFMA chain + cross-wave/ksplit adds: 2*dp*2^-24
//   bank rounded to fp16 when it is not fp16-exact: 2^-11
//   inv_norm rounding, final scaling: 2^-20
void knn_set_err_bound(astts_knn* h) {
    h->err_bound = ldexp(1.0, -11) + 2.0 * (double)h->dp * ldexp(1.0, -24) + ldexp(1.0, -20) + (h->exact16 ? 0.0 : ldexp(1.0, -11));
}

}  // namespace astts

extern "C" {

int astts_knn_create(const void* bank, int64_t n, int32_t d, int32_t dtype, int32_t metric,
                     astts_stream_t stream, astts_knn_t** out) {
    ASTTS_REQUIRE(out != nullptr, ASTTS_ERR_INVALID, "astts_knn_create: out is null");
    *out = nullptr;
    ASTTS_REQUIRE(bank != nullptr, ASTTS_ERR_INVALID, "astts_knn_create: bank is null");
    ASTTS_REQUIRE(n >= 1 && n <= 0x7fffffff - 4096, ASTTS_ERR_INVALID,
                  "astts_knn_create: n=%lld out of range", (long long)n);
    ASTTS_REQUIRE(n <= (int64_t)1024 * kSelSeg, ASTTS_ERR_UNSUPPORTED,
                  "astts_knn_create: n=%lld rows (selection covers at most 1024 segments of %d scores)", (long long)n, kSelSeg);
    ASTTS_REQUIRE(d >= 1 && d <= (1 << 20), ASTTS_ERR_INVALID, "astts_knn_create: d=%d out of range", d);
    ASTTS_REQUIRE(dtype == ASTTS_DTYPE_F16 || dtype == ASTTS_DTYPE_F32, ASTTS_ERR_INVALID,
                  "astts_knn_create: dtype %d (want ASTTS_DTYPE_F16|F32)", dtype);
    ASTTS_REQUIRE(metric == ASTTS_METRIC_COSINE || metric == ASTTS_METRIC_IP || metric == ASTTS_METRIC_L2, ASTTS_ERR_INVALID,
                  "astts_knn_create: metric %d (want ASTTS_METRIC_COSINE|IP|L2)", metric);
    hipStream_t st = (hipStream_t)stream;
    astts_knn* h = new astts_knn();
    h->n = n;
    h->d = d;
    h->dp = (int)align_up((size_t)d, 64);
    h->nld = (int)align_up((size_t)n, 128);
    h->capacity = h->nld;         // exactly the tiles of the bank: the first append over a tile edge grows it (astts_knn_append)
    h->metric = metric;
    int* flags = nullptr;
    auto fail = [&](int code) {
        if (flags) (void)hipFree(flags);
        astts_knn_destroy(h);
        return code;
    };
#define KNN_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_error("%s failed: %s", #expr, hipGetErrorString(_e));                        \
            return fail(ASTTS_ERR_HIP);                                                      \
        }                                                                                    \
    } while (0)
    const size_t cap = (size_t)h->capacity;  // every row tile a scan block may touch exists
    KNN_TRY(hipMalloc(&h->scan, sizeof(_Float16) * cap * h->dp));
    KNN_TRY(hipMemsetAsync(h->scan, 0, sizeof(_Float16) * cap * h->dp, st));
    // (the row-major plane is the GEMM scan's "weight" matrix: the ring kernels clamp their row index to n - 1, the tile kernels that
    // serve the GEMM while the ring kernels are switched off read whole tiles of up to 128 rows -- rows of zeros behind the bank)
    KNN_TRY(hipMalloc(&h->plane16, sizeof(_Float16) * cap * h->dp));
    if (cap > (size_t)n) KNN_TRY(hipMemsetAsync(h->plane16 + (size_t)n * h->dp, 0, sizeof(_Float16) * (cap - (size_t)n) * h->dp, st));
    KNN_TRY(hipMalloc(&h->norm64, sizeof(double) * cap));
    KNN_TRY(hipMalloc(&h->inv_norm, sizeof(float) * cap));
    if (metric == ASTTS_METRIC_L2) KNN_TRY(hipMalloc(&h->bias, sizeof(float) * cap));
    KNN_TRY(hipMalloc(&flags, 4 * sizeof(int)));
    KNN_TRY(hipMemsetAsync(flags, 0, 4 * sizeof(int), st));
    if (dtype == ASTTS_DTYPE_F32) KNN_TRY(hipMalloc(&h->plane32, sizeof(float) * cap * h->dp));      // kept when the bank is not fp16-exact
    if (knn_build_rows(h, bank, 0, n, dtype, flags, st) != ASTTS_OK) return fail(ASTTS_ERR_HIP);
    int hf[4] = {0, 0, 0, 0};
    KNN_TRY(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    KNN_TRY(hipStreamSynchronize(st));
    memcpy(&h->bmax, &hf[2], sizeof(double));
    if (hf[1]) {
        set_error("astts_knn_create: bank holds non-finite values");
        return fail(ASTTS_ERR_RANGE);
    }
    h->exact16 = (hf[0] == 0);
    if (!h->exact16) {
        // the fp32 image stays for exact re-scoring; approximate planes re-written with a per-row power-of-two scale (see knn_rescale_rows)
        if (knn_rescale(h, 0, n, st) != ASTTS_OK) return fail(ASTTS_ERR_HIP);
        KNN_TRY(hipStreamSynchronize(st));
    } else if (h->plane32) {
        (void)hipFree(h->plane32);
        h->plane32 = nullptr;
    }
    (void)hipFree(flags);
    flags = nullptr;
#undef KNN_TRY
    knn_set_err_bound(h);
    *out = h;
    return ASTTS_OK;
}

int astts_knn_destroy(astts_knn_t* h) {
    if (!h) return ASTTS_OK;
    if (h->scan) (void)hipFree(h->scan);
    if (h->plane16) (void)hipFree(h->plane16);
    if (h->plane32) (void)hipFree(h->plane32);
    if (h->norm64) (void)hipFree(h->norm64);
    if (h->inv_norm) (void)hipFree(h->inv_norm);
    if (h->bias) (void)hipFree(h->bias);
    if (h->live) (void)hipFree(h->live);
    for (auto& e : h->ev) (void)hipEventDestroy(e);
    delete h;
    return ASTTS_OK;
}

int astts_knn_info(const astts_knn_t* h, int64_t* n, int32_t* d, int32_t* scan_plane_exact) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_info: handle is null");
    if (n) *n = h->n;
    if (d) *d = h->d;
    if (scan_plane_exact) *scan_plane_exact = h->exact16 ? 1 : 0;
    return ASTTS_OK;
}

size_t astts_knn_workspace_bytes(const astts_knn_t* h, int32_t nq, int32_t k) {
    if (!h || nq < 1 || k < 1 || k > ASTTS_KNN_MAX_K) return 0;
    // (the layout does not depend on the route; it follows the current n, and a bank with tombstones adds the combined mask)
    return make_plan(h->n, h->d, nq, k, false, true, knn_switches(), false, h->live != nullptr).total;
}

}  // extern "C"

namespace {

// The arguments every re-score launch shares, gathered once per chunk (the kernels keep scalar parameters: a by-value struct is not
// preloaded, see the Makefile); `k` = hits per query = the row stride of the outputs; at(q0): the same from query q0 of the chunk on
struct KnnRescoreArgs {
    const float* qf; const double* qn; const float* qscale; const double* norm64; int64_t n; int dp, c, k; double err_bound; int force;
    int64_t* out_idx; float* out_score; double* out_score64; int* nflag; int metric; double bmax;
    KnnRescoreArgs at(int q0) const {
        const size_t o = (size_t)q0 * k;
        return {qf + (size_t)q0 * dp, qn + q0, qscale + q0, norm64, n, dp, c, k, err_bound, force, out_idx + o, out_score + o,
                out_score64 ? out_score64 + o : nullptr, nflag, metric, bmax};
    }
};

// One chunk of queries and ONE launcher per step of its plan; none of them decides anything, the route says which to call
struct KnnChunk {
    astts_knn* h; const KnnPlan& p; hipStream_t st; const float* queries; int nq;
    _Float16 *qh, *qrow;                 // fp16 query images: scan tiles / row-major for the GEMM (null in a plan without one)
    float* spart; int* cidx; float* cs;  // score plane(s); candidate lists [nq][64]
    int* sidx; float *ss, *blkmax;       // per-segment lists [256][nseg][64]; block maxima of the GEMM scan [256][bm_ld]
    const uint8_t* mask; int64_t mstride;  // the caller's row mask, or the chunk's own per-query masks (k > 32)
    KnnRescoreArgs rs;

    const uint8_t* mask_at(int q0) const { return mask ? mask + (int64_t)q0 * mstride : nullptr; }
    // a plain GEMM leaves bare dot products: the selection behind it applies 1 / |b_n| (and L2's constant)
    static bool raw(int scan) { return scan == ASTTS_KNN_SCAN_GEMM || scan == ASTTS_KNN_SCAN_GEMM_N_FIRST; }
    // the exact plane in its own type -- fp16 when the bank is fp16-exact, else fp32 -- handed to `launch`
    template <typename F>
    void with_plane(F&& launch) const {
        if (h->exact16) launch((const _Float16*)h->plane16);
        else launch((const float*)h->plane32);
    }
    template <typename P>
    using RowOf = std::remove_cv_t<std::remove_pointer_t<P>>;

    // ONE scan launch for queries [q0, q0 + qg), between a pair of profiling events (bench.py divides by the pairs)
    int scan(KnnRoute r, int q0, int qg) const {
        const bool prof = h->profile && h->ev_used + 2 <= h->ev.size();
        if (prof) ASTTS_CHECK_HIP(hipEventRecord(h->ev[h->ev_used], st));
        const _Float16 *qh_g = qh + (size_t)q0 * h->dp, *qrow_g = qrow ? qrow + (size_t)q0 * h->dp : nullptr;
        const float* qs_g = rs.qscale + q0;
        int rc = ASTTS_ERR_INVALID;
        switch (r.scan * 100 + (r.scan == ASTTS_KNN_SCAN_REGISTER ? p.qt * 10 + p.rt : 0)) {
            case ASTTS_KNN_SCAN_DIRECT * 100: rc = launch_scan<1, 1, true>(h, p, nullptr, qg, spart, nullptr, st, queries, rs.nflag); break;
            case ASTTS_KNN_SCAN_REGISTER * 100 + 11: rc = launch_scan<1, 1>(h, p, qh_g, qg, spart, qs_g, st); break;
            case ASTTS_KNN_SCAN_REGISTER * 100 + 21: rc = launch_scan<2, 1>(h, p, qh_g, qg, spart, qs_g, st); break;
            case ASTTS_KNN_SCAN_REGISTER * 100 + 22: rc = launch_scan<2, 2>(h, p, qh_g, qg, spart, qs_g, st); break;
            case ASTTS_KNN_SCAN_REGISTER * 100 + 41: rc = launch_scan<4, 1>(h, p, qh_g, qg, spart, qs_g, st); break;
            case ASTTS_KNN_SCAN_REGISTER * 100 + 81: rc = launch_scan<8, 1>(h, p, qh_g, qg, spart, qs_g, st); break;
            case ASTTS_KNN_SCAN_GEMM * 100: rc = gemm_scan(qrow_g, h->plane16, spart, qg, h->n, h->dp, h->nld, st); break;
            case ASTTS_KNN_SCAN_GEMM_BLOCKS * 100:
                rc = gemm_scan(qrow_g, h->plane16, spart, qg, h->n, h->dp, h->nld, st, h->inv_norm, h->bias, qs_g, blkmax, p.bm_ld);
                break;
            case ASTTS_KNN_SCAN_GEMM_N_FIRST * 100:
                rc = astts_op_gemm(qrow_g, 1, h->plane16, nullptr, nullptr, nullptr, spart, 0, qg, (int32_t)h->n, h->dp, h->dp, 1, h->dp,
                                   h->nld, 0, qg, qg, 1, 1, 0, ASTTS_ACT_NONE, 1.0f, 0.1f, nullptr, (astts_stream_t)st);
                break;
            default: set_error("astts_knn_search: no scan variant for scan=%d qt=%d rt=%d", r.scan, p.qt, p.rt);
        }
        if (rc != ASTTS_OK) return rc;
        if (prof) {
            ASTTS_CHECK_HIP(hipEventRecord(h->ev[h->ev_used + 1], st));
            h->ev_used += 2;
        }
        return ASTTS_OK;
    }

    // FUSED: selection + fp64 re-score + certification of the whole search in one launch (one segment, one query group)
    int finish_fused(KnnRoute r) const {
        const float *inv = raw(r.scan) ? h->inv_norm : nullptr, *bias = raw(r.scan) ? h->bias : nullptr;
        const int direct = r.scan == ASTTS_KNN_SCAN_DIRECT ? 1 : 0;
        const KnnRescoreArgs& a = rs;
        with_plane([&](auto plane) {
            hipLaunchKernelGGL((knn_select_rescore<RowOf<decltype(plane)>>), dim3(nq), dim3(1024), 0, st, spart, p.ksplit, p.qpad,
                               h->nld, p.seg_len, inv, a.qf, a.qn, a.qscale, plane, a.norm64, a.n, a.dp, a.c, a.k, a.err_bound, a.force,
                               a.out_idx, a.out_score, a.out_score64, a.nflag, a.metric, a.bmax, bias, mask, mstride, direct);
        });
        ASTTS_CHECK_LAUNCH();
        return ASTTS_OK;
    }

    // BLOCKS: the scan left block maxima -- c blocks of 64 scores per query instead of the row, and the fp64 re-score in the same launch
    int finish_blocks(int q0, int qg) const {
        const KnnRescoreArgs a = rs.at(q0);
        with_plane([&](auto plane) {
            hipLaunchKernelGGL((knn_blocks_rescore<RowOf<decltype(plane)>>), dim3(qg), dim3(1024), 0, st, spart, h->nld,
                               (const float*)blkmax, p.bm_ld, p.nblk, a.qf, a.qn, a.qscale, plane, a.norm64, a.n, a.dp, a.c, a.k, a.err_bound,
                               a.force, a.out_idx, a.out_score, a.out_score64, a.nflag, a.metric, a.bmax);
        });
        ASTTS_CHECK_LAUNCH();
        return ASTTS_OK;
    }

    // STREAM / SELECT / SELECT_MERGE: the candidate lists of queries [q0, q0 + qg) (their re-score is a launch of its own: rescore)
    int select(KnnRoute r, int q0, int qg) const {
        const float *inv = raw(r.scan) ? h->inv_norm : nullptr, *bias = raw(r.scan) ? h->bias : nullptr, *qs_g = rs.qscale + q0;
        const uint8_t* mask_g = mask_at(q0);
        int* ci = cidx + (size_t)q0 * 64;
        float* cs_g = cs + (size_t)q0 * 64;
        if (r.finish == ASTTS_KNN_FINISH_STREAM) {          // a long row behind a GEMM: one streaming block per query
            if (bias || mask_g)     // (a third / fourth load per score: half the span keeps the registers)
                hipLaunchKernelGGL((knn_select_stream<8, true>), dim3(qg), dim3(kSelThreads), 0, st, spart, h->nld, h->n, p.c, ci, cs_g, inv,
                                   bias, qs_g, mask_g, mstride);
            else
                hipLaunchKernelGGL((knn_select_stream<16, false>), dim3(qg), dim3(kSelThreads), 0, st, spart, h->nld, h->n, p.c, ci, cs_g, inv,
                                   bias, qs_g, mask_g, mstride);
        } else if (r.finish == ASTTS_KNN_FINISH_SELECT) {   // one segment: a block per query, straight into the candidate lists
            hipLaunchKernelGGL(knn_select, dim3(qg, 1), dim3(kSelThreads), 0, st, spart, p.ksplit, p.qpad, h->nld, h->n, p.c, p.seg_len, ci,
                               cs_g, inv, bias, qs_g, mask_g, mstride);
        } else {                                            // SELECT_MERGE: a block per (query, segment), then a one-wave merge
            hipLaunchKernelGGL(knn_select, dim3(qg, p.nseg), dim3(kSelThreads), 0, st, spart, p.ksplit, p.qpad, h->nld, h->n, p.c, p.seg_len,
                               sidx, ss, inv, bias, qs_g, mask_g, mstride);
            ASTTS_CHECK_LAUNCH();
            hipLaunchKernelGGL(knn_select_merge, dim3(qg), dim3(64), 0, st, sidx, ss, p.nseg, p.c, ci, cs_g);
        }
        ASTTS_CHECK_LAUNCH();
        return ASTTS_OK;
    }

    // fp64 re-score + certification of `kp` hits for queries [q0, q0 + qg) from their candidate lists, into columns out_off .. of the
    // outputs (this group's queries only: grid offset through the pointer arguments)
    int rescore(int q0, int qg, int kp, int out_off) const {
        const KnnRescoreArgs a = rs.at(q0);
        with_plane([&](auto plane) {
            hipLaunchKernelGGL((knn_rescore_finalize<RowOf<decltype(plane)>>), dim3(qg), dim3(1024), 0, st, a.qf, a.qn, a.qscale,
                               plane, a.norm64, a.n, a.dp, a.c, kp, (const int*)(cidx + (size_t)q0 * 64), (const float*)(cs + (size_t)q0 * 64),
                               a.err_bound, a.force, a.out_idx, a.out_score, a.out_score64, a.nflag, a.metric, a.bmax, mask_at(q0), mstride,
                               a.k, out_off);
        });
        ASTTS_CHECK_LAUNCH();
        return ASTTS_OK;
    }
};

// One chunk of queries (all of them when k <= 32; <= 256 when k > 32): preparation, then per query group ONE scan and the finish of the
// group's route.  k > 32: `passes` rounds of selection + fp64 re-score that each emit <= 32 hits per query into out[q * k + done ..] --
// between rounds the rows just returned leave the chunk's per-query masks, so round r + 1 ranks what is left (same certification, same
// exact path); the rounds re-rank the SAME score plane, so they end before the next group's scan overwrites it.
int knn_search_chunk(astts_knn* h, const KnnPlan& p, const float* queries, int nq, int k, int64_t* out_idx, float* out_score,
                     double* out_score64, const uint8_t* row_mask, int64_t mask_stride, char* ws, int flags, bool clear_flag,
                     hipStream_t st) {
    const bool direct = p.route.scan == ASTTS_KNN_SCAN_DIRECT, multi = p.passes > 1;
    int* nflag = (int*)(ws + p.off_nflag);
    float *qf = (float*)(ws + p.off_qf), *qscale = (float*)(ws + p.off_qscale);
    double* qn = (double*)(ws + p.off_qn);
    uint8_t* own_mask = (uint8_t*)(ws + p.off_mask);
    // The mask the kernels see.  k > 32: per-query masks in the workspace.  A bank with tombstones: its live mask, ANDed into the
    // workspace with the caller's when there is one (one row for a shared mask, else one per query).  Otherwise the caller's, as is.
    const bool own = multi || (h->live && row_mask);
    const int own_rows = multi || mask_stride ? nq : 1;
    const uint8_t* const mask = own ? own_mask : h->live ? h->live : row_mask;
    const int64_t mstride = own ? (own_rows > 1 || multi ? h->n : 0) : h->live ? 0 : mask_stride;
    const KnnChunk c{h, p, st, queries, nq, (_Float16*)(ws + p.off_qh), p.gemm ? (_Float16*)(ws + p.off_qrow) : nullptr,
                     (float*)(ws + p.off_spart), (int*)(ws + p.off_cidx), (float*)(ws + p.off_cs), (int*)(ws + p.off_sidx),
                     (float*)(ws + p.off_ss), (float*)(ws + p.off_bmax), mask, mstride,
                     // (direct: no preparation launch -- the finish reads the caller's queries and forms their norms itself)
                     KnnRescoreArgs{direct ? queries : qf, qn, qscale, h->norm64, h->n, h->dp, p.c, k, h->err_bound,
                                    (flags & ASTTS_KNN_FORCE_EXACT) ? 1 : 0, out_idx, out_score, out_score64, nflag, h->metric, h->bmax}};
    if (own) {
        hipLaunchKernelGGL(knn_mask_init, dim3((unsigned)(cdiv(h->n, 256 * 16) < 1024 ? cdiv(h->n, 256 * 16) : 1024), own_rows), dim3(256), 0,
                           st, own_mask, row_mask, mask_stride, h->n, (const uint8_t*)h->live);
        ASTTS_CHECK_LAUNCH();
    }
    if (!direct) {
        hipLaunchKernelGGL(knn_prep_queries, dim3((unsigned)align_up((size_t)nq, 32)), dim3(256), 0, st, queries, nq, h->d, h->dp, c.qh, qf, qn,
                           qscale, clear_flag ? nflag : nullptr, c.qrow);
        ASTTS_CHECK_LAUNCH();
    }
    int finished = 0;           // leading queries whose hits a BLOCKS launch has written (groups come in order; only the last can differ)
    for (int q0 = 0; q0 < nq; q0 += p.gstep) {
        const int qg = (nq - q0) < p.gstep ? (nq - q0) : p.gstep;
        const KnnRoute r = p.of(qg);
        int rc = c.scan(r, q0, qg);
        if (rc != ASTTS_OK) return rc;
        if (r.finish == ASTTS_KNN_FINISH_FUSED) return c.finish_fused(r);
        if (r.finish == ASTTS_KNN_FINISH_BLOCKS) {
            if ((rc = c.finish_blocks(q0, qg)) != ASTTS_OK) return rc;
            finished = q0 + qg;
            continue;
        }
        for (int done = 0; done < k; done += kPassK) {
            if ((rc = c.select(r, q0, qg)) != ASTTS_OK) return rc;
            if (!multi) break;          // (one pass: the candidate lists of every group wait for the one re-score launch below)
            const int kp = (k - done) < kPassK ? (k - done) : kPassK;
            if ((rc = c.rescore(q0, qg, kp, done)) != ASTTS_OK) return rc;
            if (done + kPassK < k) {
                hipLaunchKernelGGL(knn_mask_out, dim3(qg), dim3(64), 0, st, out_idx + (size_t)q0 * k, k, done, kp, own_mask + (int64_t)q0 * h->n,
                                   h->n);
                ASTTS_CHECK_LAUNCH();
            }
        }
    }
    if (multi || finished == nq) return ASTTS_OK;
    return c.rescore(finished, nq - finished, k, 0);      // the queries no fused launch has finished: all of them, or the tail group
}

}  // namespace

extern "C" {

int astts_knn_search(astts_knn_t* h, const float* queries, int32_t nq, int32_t k, int64_t* out_idx,
                     float* out_score, double* out_score64, const uint8_t* row_mask, int64_t mask_stride,
                     void* workspace, size_t workspace_bytes, int32_t flags, astts_stream_t stream) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_search: handle is null");
    ASTTS_REQUIRE(queries && out_idx && out_score, ASTTS_ERR_INVALID, "astts_knn_search: null pointer argument");
    ASTTS_REQUIRE(nq >= 1, ASTTS_ERR_INVALID, "astts_knn_search: nq=%d", nq);
    ASTTS_REQUIRE(k >= 1 && k <= ASTTS_KNN_MAX_K, ASTTS_ERR_INVALID,
                  "astts_knn_search: k=%d (1..%d)", k, ASTTS_KNN_MAX_K);
    ASTTS_REQUIRE(row_mask == nullptr || mask_stride == 0 || mask_stride >= h->n, ASTTS_ERR_INVALID,
                  "astts_knn_search: mask_stride %lld (0 = one mask for every query, else >= n = %lld)", (long long)mask_stride, (long long)h->n);
    ASTTS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 255) == 0, ASTTS_ERR_WORKSPACE,
                  "astts_knn_search: workspace must be 256-byte aligned");
    const KnnPlan p = plan_search(h->n, h->d, nq, k, row_mask != nullptr, ((uintptr_t)queries & 15) == 0, workspace, h->live != nullptr);
    ASTTS_REQUIRE(workspace_bytes >= p.total, ASTTS_ERR_WORKSPACE,
                  "astts_knn_search: workspace %zu < required %zu", workspace_bytes, p.total);
    const int chunk = p.passes == 1 ? nq : kMaxQPerPass;      // k > 32: chunks of <= 256 queries share the workspace, in stream order
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int qc = (nq - q0) < chunk ? (nq - q0) : chunk;
        const int rc = knn_search_chunk(h, p, queries + (size_t)q0 * h->d, qc, k, out_idx + (size_t)q0 * k, out_score + (size_t)q0 * k,
                                        out_score64 ? out_score64 + (size_t)q0 * k : nullptr,
                                        row_mask ? row_mask + (int64_t)q0 * mask_stride : nullptr, mask_stride, (char*)workspace, flags,
                                        q0 == 0, (hipStream_t)stream);
        if (rc != ASTTS_OK) return rc;
    }
    return ASTTS_OK;
}

int astts_knn_route(int64_t n, int32_t d, int32_t nq, int32_t k, int32_t masked, int32_t queries_aligned, int32_t group, int32_t* rows,
                    int32_t* scan, int32_t* finish, int32_t* passes) {
    ASTTS_REQUIRE(n >= 1 && n <= (int64_t)1024 * kSelSeg && d >= 1 && d <= (1 << 20) && nq >= 1 && k >= 1 && k <= ASTTS_KNN_MAX_K,
                  ASTTS_ERR_INVALID, "astts_knn_route: bad shape n=%lld d=%d nq=%d k=%d", (long long)n, d, nq, k);
    const KnnPlan p = plan_search(n, d, nq, k, masked != 0, queries_aligned != 0, nullptr);
    ASTTS_REQUIRE(group >= 0 && (int64_t)group * p.gstep < nq, ASTTS_ERR_INVALID, "astts_knn_route: group %d of %lld", group,
                  (long long)cdiv(nq, p.gstep));
    const int left = nq - group * p.gstep, qg = left < p.gstep ? left : p.gstep;
    const KnnRoute r = p.of(qg);
    if (rows) *rows = qg;
    if (scan) *scan = r.scan;
    if (finish) *finish = r.finish;
    if (passes) *passes = p.passes;
    return ASTTS_OK;
}

int astts_knn_profile_enable(astts_knn_t* h, int32_t on) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_profile_enable: handle is null");
    if (on && h->ev.empty()) {
        h->ev.resize(2 * 8192);
        for (auto& e : h->ev) ASTTS_CHECK_HIP(hipEventCreate(&e));
    }
    h->profile = on != 0;
    h->ev_used = 0;
    return ASTTS_OK;
}

int astts_knn_profile_read(astts_knn_t* h, double* scan_ms_sum, int64_t* scan_launches) {
    ASTTS_REQUIRE(h && scan_ms_sum && scan_launches, ASTTS_ERR_INVALID, "astts_knn_profile_read: null argument");
    double sum = 0.0;
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        ASTTS_CHECK_HIP(hipEventSynchronize(h->ev[i + 1]));
        float ms = 0.f;
        ASTTS_CHECK_HIP(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        sum += ms;
    }
    *scan_ms_sum = sum;
    *scan_launches = (int64_t)(h->ev_used / 2);
    h->ev_used = 0;
    return ASTTS_OK;
}

int astts_knn_last_fallbacks(const astts_knn_t* h, const void* workspace, astts_stream_t stream,
                             int32_t* n_fallback_host) {
    ASTTS_REQUIRE(h && workspace && n_fallback_host, ASTTS_ERR_INVALID,
                  "astts_knn_last_fallbacks: null argument");
    hipStream_t st = (hipStream_t)stream;
    ASTTS_CHECK_HIP(hipMemcpyAsync(n_fallback_host, workspace, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ASTTS_CHECK_HIP(hipStreamSynchronize(st));
    return ASTTS_OK;
}

}  // extern "C"
