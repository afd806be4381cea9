// ops_gemm.hip -- fp16-MFMA implicit GEMM with fp32 activations / fp32 accumulate (gfx950).
//
// One kernel family serves every dense contraction of the synthesis path (the arithmetic the
// reference runs inside cosyvoice: nn.Linear, nn.Conv1d incl. dilation/stride, nn.ConvTranspose1d
// after phase decomposition):
//
//   out[m, n] = epilogue( sum_{tap, c} X[src_row(m, tap), c] * W[n, tap*cin_pad + c] )
//   m = b*t_out + t,   src_row = b*t_in + t*stride + tap*dil - pad   (zero outside [0, t_in))
//
// X: fp32 [B*t_in, lda] channels-last, W: fp16 [n_pad, taps*cin_pad] (K contiguous, zero padded:
// cin_pad multiple of 64, n_pad multiple of 128), out: fp32 [B*t_out, ldc].
// epilogue: (+bias[n]) -> activation -> *alpha -> *row_scale[m] -> +residual[m, n]
//
// Three files, one path per call:
//   gemm_kernels.h  the device code (argument block, epilogues, gemm_tile, the ring kernels, gemm_skinny16, gemm_rows);
//   gemm_plan.h     WHAT runs for a shape -- kernel family, ring tile, split-K and row passes of the skinny kernel, the tile of
//                   gemm_rows: pure host functions, no HIP, tested on the CPU against recorded plans (tests/test_gemm_plan_cpu.py);
//   this file       a C entry fills a GemmArgs by name -> launch_gemm asks gemm_plan() -> one typed launcher per kernel family
//                   (launch_tile, launch_ring, launch_skinny, launch_rows), each of which derives grid, block and LDS bytes from its
//                   template arguments or the plan, and sets the dynamic-LDS attribute once under a std::once_flag.
#include "gemm_kernels.h"
#include "gemm_plan.h"
#include "flow_share.h"
#include "../../include/session/astts_flow_share.h"

#include <cstdlib>
#include <mutex>

namespace astts {

static_assert(kSkinnyWaves == SK_WAVES, "gemm_plan.h sizes the skinny kernel's LDS image for the kernel's wave count");

template <int RT, int CT, int PL, bool A32>
static void launch_rows(const GemmArgs& a, hipStream_t st) {
    static std::once_flag attr;
    const size_t lds = (size_t)8 * RT * CT * 4 * 64 * sizeof(float);
    std::call_once(attr, [&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_rows<RT, CT, PL, A32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    const unsigned grid = (unsigned)(cdiv(a.m, 16 * RT) * cdiv(a.n, 16 * CT));
    hipLaunchKernelGGL((gemm_rows<RT, CT, PL, A32>), dim3(grid), dim3(512), lds, st, a);
}

// the workgroup tile gemm_rows_plan picked, among the ones instantiated for this PL (the plan applies the same PL guards);
// false: the plan names a tile that is not instantiated here, i.e. the two tables have drifted apart -- nothing is launched
template <int PL, bool A32>
static bool launch_rows_pl(const RowsPlan& p, const GemmArgs& a, hipStream_t st) {
    if constexpr (PL <= 2) {
        if (p.rt == 4 && p.ct == 2) return launch_rows<4, 2, PL, A32>(a, st), true;
    }
    if constexpr (PL <= 4) {
        if (p.rt == 2 && p.ct == 2) return launch_rows<2, 2, PL, A32>(a, st), true;
    }
    if (p.rt == 2 && p.ct == 1) return launch_rows<2, 1, PL, A32>(a, st), true;
    return false;
}

// the plain case: out[m, n] = x[m, k] . w[n, k]^T, one tap, every row a sequence position of one batch row
static GemmArgs gemm_args(const void* x, const void* w_f16, void* out, int64_t m, int n, int k, int lda, int ldc) {
    GemmArgs a;
    a.x = (const float*)x;
    a.w = (const _Float16*)w_f16;
    a.out = (float*)out;
    a.m = m;
    a.n = n;
    a.cin = a.cin_pad = k;
    a.lda = lda;
    a.ldc = ldc;
    a.t_in = a.t_out = (int)m;
    return a;
}

template <int WM, int WN, int TM, int TN, int BKT>
static void launch_tile(const GemmArgs& a, hipStream_t st) {
    constexpr int BM = WM * TM * 32, BN = WN * TN * 32;
    const dim3 grid((unsigned)cdiv(a.m, BM), (unsigned)cdiv(a.n, BN));
    if (a.x_f16)
        hipLaunchKernelGGL((gemm_tile<WM, WN, TM, TN, true, BKT>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((gemm_tile<WM, WN, TM, TN, false, BKT>), grid, dim3(256), 0, st, a);
}

// The launch geometry of a ring kernel (gemm_ring.inc under either of its names) follows from its template arguments: NW waves as
// (NW / WN) x WN, wave tile (32 TM) x (32 TN), a stage of the ring = (BM + BN) rows of 128 B.
template <int TM, int TN, int STAGES, int WN = 2, int NW = 4>
struct RingGeom {
    static constexpr int BM = (NW / WN) * TM * 32, BN = WN * TN * 32;
    static constexpr int threads = NW * 64;
    static constexpr int lds = STAGES * (BM + BN) * 128;
};
// what the launches used to spell out beside each kernel name
static_assert(RingGeom<2, 2, 2>::lds == 2 * 256 * 128, "128 x 128, two stages");
static_assert(RingGeom<2, 1, 2>::lds == 2 * 192 * 128, "128 x 64, two stages");
static_assert(RingGeom<1, 1, 4>::lds == 4 * 128 * 128, "64 x 64, four stages");
static_assert(RingGeom<4, 2, 2, 4, 8>::lds == 2 * 512 * 128, "256 x 256, two stages (also gemm_ring8 / head_lse_ring8)");
static_assert(RingGeom<1, 2, 3, 4>::lds == 3 * 288 * 128, "32 x 256, three stages (astts_op_gemm_ln)");
static_assert(RingGeom<2, 2, 2, 4, 4>::lds == 2 * 320 * 128, "64 x 256, two stages (head_lse_ring)");

// one launch: one workgroup per BM x BN tile (1-D: the kernel orders the tiles itself), the dynamic-LDS attribute set once
template <typename G, typename Args>
static void launch_ring_kernel(void (*kern)(Args), std::once_flag& attr, const Args& a, hipStream_t st) {
    std::call_once(attr, [&] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, G::lds); });
    hipLaunchKernelGGL(kern, dim3((unsigned)(cdiv(a.m, G::BM) * cdiv(a.n, G::BN))), dim3(G::threads), G::lds, st, a);
}

template <int TM, int TN, int STAGES, int WN = 2, int NW = 4>
static void launch_ring(const GemmArgs& a, hipStream_t st) {
    static std::once_flag attr;
    launch_ring_kernel<RingGeom<TM, TN, STAGES, WN, NW>>(&gemm_ring<TM, TN, STAGES, WN, NW>, attr, a, st);
}

// 256 x 256 on the eight-phase schedule: the tile of gemm_ring<4, 2, 2, 4, 8>
static void launch_ring8(const GemmArgs& a, hipStream_t st) {
    static std::once_flag attr;
    launch_ring_kernel<RingGeom<4, 2, 2, 4, 8>>(&gemm_ring8, attr, a, st);
}

// the LM head's twins of the two launchers above
template <int TM, int TN, int STAGES, int WN, int NW>
static void launch_head_lse_ring(const HeadLseArgs& a, hipStream_t st) {
    static std::once_flag attr;
    launch_ring_kernel<RingGeom<TM, TN, STAGES, WN, NW>>(&head_lse_ring<TM, TN, STAGES, WN, NW>, attr, a, st);
}

static void launch_head_lse_ring8(const HeadLseArgs& a, hipStream_t st) {
    static std::once_flag attr;
    launch_ring_kernel<RingGeom<4, 2, 2, 4, 8>>(&head_lse_ring8, attr, a, st);
}

// The skinny kernel over the plan's row passes: the block keeps its rows of x as an fp16 image in LDS, so rows are taken in chunks
// that fit (GemmPlan::rows).  Every pass is a launch of its own for the launch profiler.
static void launch_skinny(const GemmPlan& p, const GemmArgs& a, hipStream_t st) {
    static std::once_flag attr;
    std::call_once(attr, [] {  // allow > 64 KiB of dynamic LDS (one-off, outside any captured region in practice)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_skinny16<1, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkinnyLdsMax);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_skinny16<2, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkinnyLdsMax);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_skinny16<1, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkinnyLdsMax);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_skinny16<2, 16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkinnyLdsMax);
    });
    const dim3 grid((a.n + 15) / 16, p.ksplit);
    for (int r0 = 0; r0 < (int)a.m; r0 += p.rows) {
        GemmArgs c = a;
        c.ksplit = p.ksplit;
        c.m = (int)a.m - r0 < p.rows ? (int)a.m - r0 : p.rows;
        if (c.gather) c.gather += r0; else c.x += (int64_t)r0 * a.lda;
        if (c.residual) c.residual += (int64_t)r0 * a.ldr;
        if (c.row_scale) c.row_scale += r0;
        c.out += (int64_t)r0 * a.ldc;
        if (c.out2) c.out2 = a.out2_f16 ? (float*)((_Float16*)a.out2 + (int64_t)r0 * a.ldc2) : a.out2 + (int64_t)r0 * a.ldc2;
        const int mt = skinny_mt((int)c.m);
        const size_t lds = skinny_lds_bytes((int)c.m, p.kslice, mt);
        const bool prof = prof_begin(ASTTS_PROF_GEMM_SKINNY, st, (double)a.n * a.cin_pad * 2.0);
        if (mt == 1 && p.xv == 4)
            hipLaunchKernelGGL((gemm_skinny16<1, 4>), grid, dim3(512), lds, st, c);
        else if (mt == 1)
            hipLaunchKernelGGL((gemm_skinny16<1, 16>), grid, dim3(512), lds, st, c);
        else if (p.xv == 4)
            hipLaunchKernelGGL((gemm_skinny16<2, 4>), grid, dim3(512), lds, st, c);
        else
            hipLaunchKernelGGL((gemm_skinny16<2, 16>), grid, dim3(512), lds, st, c);
        if (prof) prof_end(ASTTS_PROF_GEMM_SKINNY, st);
    }
}

static int g_ring_mode_override = kRingModeAuto;   // astts_op_gemm_set_ring_mode: auto = the rule / ASTTS_GEMM_RING, else that switch

// the ring switch in force: astts_op_gemm_set_ring_mode (tests) over the environment's ASTTS_GEMM_RING over the rule
static int ring_mode_in_force() {
    static const int ring_env0 = [] { const char* e = getenv("ASTTS_GEMM_RING"); return e ? atoi(e) : kRingModeAuto; }();
    return g_ring_mode_override >= kRingModeOff ? g_ring_mode_override : ring_env0;
}

// what gemm_plan reads of a call (plain: row lengths are masked by the tile kernel only)
static GemmShape gemm_shape(const GemmArgs& a) {
    static const bool nosplit_env = getenv("ASTTS_NO_SPLITK") != nullptr;
    GemmShape s;
    s.m = a.m;
    s.n = a.n;
    s.cin = a.cin;
    s.cin_pad = a.cin_pad;
    s.taps = a.taps;
    s.plain = a.taps == 1 && a.stride == 1 && a.pad == 0 && a.t_in == a.t_out && !a.in_lens;
    s.x_f16 = a.x_f16 != 0;
    s.out_f16 = a.out_f16 != 0;
    s.x_aligned = (a.lda & 7) == 0 && ((uintptr_t)a.x & 15) == 0;
    s.blockmax = a.blockmax != nullptr;
    s.gather = a.gather != nullptr;
    s.ln = a.ln_gamma != nullptr;
    s.splitk_ws = a.sk_part != nullptr;
    s.ring_mode = ring_mode_in_force();
    s.no_splitk = nosplit_env;
    return s;
}

// what gemm_plan reads of an astts_op_gemm call, m aside (flow_engine.hip groups the batches of a joined pass by their plans)
GemmShape gemm_shape_of_call(const void* x, int x_f16, int out_f16, int n, int cin, int cin_pad, int taps, int lda, int t_in, int t_out,
                             int stride, int pad) {
    GemmArgs a;
    a.x = (const float*)x;
    a.n = n;
    a.cin = cin;
    a.cin_pad = cin_pad;
    a.taps = taps;
    a.lda = lda;
    a.t_in = t_in;
    a.t_out = t_out;
    a.stride = stride;
    a.pad = pad;
    a.x_f16 = x_f16 ? 1 : 0;
    a.out_f16 = out_f16 ? 1 : 0;
    return gemm_shape(a);
}

// Every GEMM call: shape -> plan -> the launcher of the planned kernel.  What runs is decided in gemm_plan.h and nowhere else.
// plan_m > 0: the plan is the one gemm_plan() gives plan_m rows, the kernel runs over all a.m rows (grid, bounds and the skinny
// kernel's passes follow a.m): the rows of several batches in the launch each batch gets alone (flow_share.h).
static int launch_gemm(const GemmArgs& a, hipStream_t st, int64_t plan_m = 0) {
    GemmShape shape = gemm_shape(a);
    if (plan_m > 0) shape.m = plan_m;
    const GemmPlan p = gemm_plan(shape);
    const bool skinny = p.kind == ASTTS_GEMM_KIND_SKINNY;
    ASTTS_REQUIRE(gemm_plan_serves(p, a.m), ASTTS_ERR_UNSUPPORTED,
                  "astts_op_gemm_planned: the plan of %lld rows is the m <= 32 family, which does not serve m=%lld", (long long)plan_m, (long long)a.m);
    ASTTS_REQUIRE(!skinny || p.fits, ASTTS_ERR_INVALID, "astts_op_gemm: cin_pad=%d does not fit the skinny kernel's LDS image", a.cin_pad);
    ASTTS_REQUIRE(skinny || (!a.gather && !a.ln_gamma && !a.out2), ASTTS_ERR_INVALID,
                  "astts_op_gemm_fused: gather / LayerNorm / split output need m <= 32 and a plain (non-conv) GEMM");
    // (launch_skinny brackets each of its passes itself, under its own profiler kind)
    const bool prof = !skinny && prof_begin(ASTTS_PROF_GEMM_TILE, st, 2.0 * (double)a.m * a.n * a.cin * a.taps);
    switch (p.kind) {
        case ASTTS_GEMM_KIND_SKINNY: launch_skinny(p, a, st); break;
        case ASTTS_GEMM_KIND_RING:
            switch (p.tile) {
                case RingTile::T128x128_S2: launch_ring<2, 2, 2>(a, st); break;
                case RingTile::T128x64_S2: launch_ring<2, 1, 2>(a, st); break;
                case RingTile::T64x64_S4: launch_ring<1, 1, 4>(a, st); break;
                case RingTile::T256x256_1B: launch_ring<4, 2, 2, 4, 8>(a, st); break;
                case RingTile::T256x256_8P: launch_ring8(a, st); break;
            }
            break;
        case ASTTS_GEMM_KIND_T32: launch_tile<4, 1, 1, 1, 64>(a, st); break;
        case ASTTS_GEMM_KIND_T128: launch_tile<2, 2, 2, 2, 32>(a, st); break;
        case ASTTS_GEMM_KIND_T128X64: launch_tile<2, 2, 2, 1, 32>(a, st); break;
        case ASTTS_GEMM_KIND_T64K128: launch_tile<2, 2, 1, 1, 128>(a, st); break;
        default: launch_tile<2, 2, 1, 1, 64>(a, st); break;
    }
    if (prof) prof_end(ASTTS_PROF_GEMM_TILE, st);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

// Will the ring kernels serve the kNN scan of `qg` fp16 query rows [qg][dp] with its block-maximum epilogue?  The kNN route (knn.hip) asks
// before it plans that scan and gemm_scan checks its arguments with the same answer: the plan of the GEMM gemm_scan builds, under
// the ring switch in force.  (n > 64: the maxima are per 64 columns of a wave, i.e. the tiles with TN = 2, and a narrower output gets the
// 128 x 64 tile.)  queries: null stands for a 16-byte aligned pointer (a host query has none).
bool gemm_scan_blockmax_ok(int32_t qg, int64_t n, int32_t dp, const void* queries) {
    GemmShape s;
    s.m = qg;
    s.n = (int)n;
    s.cin = dp;
    s.cin_pad = (int)align_up((size_t)dp, 64);
    s.x_f16 = true;
    s.x_aligned = ((uintptr_t)queries & 15) == 0;
    s.blockmax = true;
    s.ring_mode = ring_mode_in_force();
    return n > 64 && gemm_plan(s).kind == ASTTS_GEMM_KIND_RING;
}

// the kNN scan as one GEMM (knn.hip): scores[q][n] = <query q, bank row n>, fp16 operands, fp32 out [qg][ldc]; row panels of one bank
// tile first (GemmArgs::m_first), so that the bank is fetched from HBM once however many 128-query panels there are
int gemm_scan(const _Float16* queries, const _Float16* bank, float* out, int32_t qg, int64_t n, int32_t dp, int32_t ldc, hipStream_t st,
              const float* col_scale, const float* col_bias, const float* row_qs, float* blockmax, int32_t bm_ld) {
    GemmArgs a = gemm_args(queries, bank, out, qg, (int)n, dp, dp, ldc);
    a.x_f16 = 1;
    a.m_first = 1;
    if (blockmax) {
        // (only the ring kernels carry that epilogue -- the caller takes the plain scan otherwise)
        if (!(gemm_scan_blockmax_ok(qg, n, dp, queries) && col_scale && (!col_bias || row_qs))) {
            set_error("gemm_scan: the block-maximum epilogue needs the ring kernels (qg=%d n=%lld dp=%d, ring mode %d)", qg, (long long)n, dp,
                      ring_mode_in_force());
            return ASTTS_ERR_INVALID;
        }
        a.col_scale = col_scale;
        a.col_bias = col_bias;
        a.row_qs = row_qs;
        a.blockmax = blockmax;
        a.bm_ld = bm_ld;
    }
    return launch_gemm(a, st);
}

// The LM head with the log-sum-exp epilogue (ops_score.hip): partials of logits[m][0 .. vocab) = <h[m], head row> (+ bias), never the
// logits.  rows >= 64: the eight-phase 256 x 256 tile; below: 64 x 256 (a decode-width call does not pay for a 256-row tile's staging and
// LDS).  Preconditions (checked by the caller): h 16-byte aligned, ldh % 8 == 0, k % 64 == 0, nblk == ceil(vocab / 256).
int gemm_head_lse(const _Float16* h, int32_t ldh, const _Float16* w, const float* bias, const int32_t* targets, int64_t rows, int32_t vocab,
                  int32_t k, float* tgt, float* part, int32_t* idx, int32_t nblk, hipStream_t st) {
    // the launchers size the grid from (rows, vocab) and the tile, ceil(rows / BM) x ceil(vocab / 256) workgroups, and the kernels index
    // part / idx by nblk: the two must be the same number
    ASTTS_REQUIRE(nblk == (int32_t)cdiv(vocab, 256), ASTTS_ERR_INVALID, "gemm_head_lse: nblk=%d is not ceil(vocab=%d / 256)", nblk, vocab);
    HeadLseArgs a{};
    static_cast<GemmArgs&>(a) = gemm_args(h, w, nullptr, rows, vocab, k, ldh, 0);
    a.bias = bias;
    a.x_f16 = 1;
    a.targets = targets;
    a.tgt = tgt;
    a.part = reinterpret_cast<float2*>(part);
    a.idx = idx;
    a.nblk = nblk;
    const bool prof = prof_begin(ASTTS_PROF_GEMM_TILE, st, 2.0 * (double)rows * vocab * k);
    if (rows >= 64) launch_head_lse_ring8(a, st);                // grid: ceil(rows / 256) x nblk tiles
    else launch_head_lse_ring<2, 2, 2, 4, 4>(a, st);             // grid: nblk tiles (rows < 64 = one 64-row panel)
    if (prof) prof_end(ASTTS_PROF_GEMM_TILE, st);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // namespace astts

using namespace astts;

static int check_gemm_args(const char* who, const float* x, const void* w, float* out, int64_t m, int32_t n, int32_t cin,
                           int32_t cin_pad, int32_t taps, int32_t t_in, int32_t t_out, int32_t stride, int32_t dil, int32_t act) {
    ASTTS_REQUIRE(x && w && out, ASTTS_ERR_INVALID, "%s: null pointer", who);
    ASTTS_REQUIRE((const void*)x != (const void*)out, ASTTS_ERR_INVALID,
                  "%s: out aliases x (every workgroup reads whole input rows: an in-place GEMM races)", who);
    ASTTS_REQUIRE(m >= 1 && n >= 1 && cin >= 1 && taps >= 1, ASTTS_ERR_INVALID, "%s: bad shape m=%lld n=%d cin=%d taps=%d",
                  who, (long long)m, n, cin, taps);
    ASTTS_REQUIRE(cin_pad >= cin && cin_pad % 64 == 0, ASTTS_ERR_INVALID,
                  "%s: cin_pad=%d must be a multiple of 64 and >= cin=%d", who, cin_pad, cin);
    ASTTS_REQUIRE(t_in >= 1 && t_out >= 1 && m % t_out == 0 && stride >= 1 && dil >= 1, ASTTS_ERR_INVALID,
                  "%s: bad conv geometry t_in=%d t_out=%d stride=%d dil=%d", who, t_in, t_out, stride, dil);
    ASTTS_REQUIRE(act >= ACT_NONE && act <= ACT_LEAKY, ASTTS_ERR_INVALID, "%s: act=%d", who, act);
    return ASTTS_OK;
}

extern "C" {

int astts_op_gemm_set_ring_mode(int32_t mode) {
    ASTTS_REQUIRE(mode >= kRingModeAuto && mode <= kRingModeMax, ASTTS_ERR_INVALID,
                  "astts_op_gemm_set_ring_mode: mode=%d (-1 auto, 0 off, 1..5 tile)", mode);
    g_ring_mode_override = mode;
    return ASTTS_OK;
}

int astts_op_gemm_kernel_kind(int64_t m, int32_t n, int32_t cin, int32_t cin_pad, int32_t taps, int32_t plain, int32_t x_f16,
                              int32_t out_f16, int32_t x_aligned) {
    ASTTS_REQUIRE(m >= 1 && n >= 1 && cin >= 1 && taps >= 1 && cin_pad >= cin && cin_pad % 64 == 0, ASTTS_ERR_INVALID,
                  "astts_op_gemm_kernel_kind: bad shape m=%lld n=%d cin=%d cin_pad=%d taps=%d", (long long)m, n, cin, cin_pad, taps);
    GemmShape s;
    s.m = m;
    s.n = n;
    s.cin = cin;
    s.cin_pad = cin_pad;
    s.taps = taps;
    s.plain = plain != 0;
    s.x_f16 = x_f16 != 0;
    s.out_f16 = out_f16 != 0;
    s.x_aligned = x_aligned != 0;
    s.ring_mode = ring_mode_in_force();
    return gemm_plan(s).kind;
}

int astts_op_pack_weight(const float* src, void* dst_f16, int32_t n, int32_t taps, int32_t cin,
                         int32_t n_pad, int32_t cin_pad, astts_stream_t stream) {
    ASTTS_REQUIRE(src && dst_f16, ASTTS_ERR_INVALID, "astts_op_pack_weight: null pointer");
    ASTTS_REQUIRE(n >= 1 && taps >= 1 && cin >= 1 && n_pad >= n && cin_pad >= cin, ASTTS_ERR_INVALID,
                  "astts_op_pack_weight: bad shape n=%d taps=%d cin=%d n_pad=%d cin_pad=%d", n, taps, cin, n_pad, cin_pad);
    const int64_t total = (int64_t)n_pad * taps * cin_pad;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_weight_f16, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src,
                       (_Float16*)dst_f16, n, taps, cin, n_pad, cin_pad);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

static int op_gemm(const char* who, const void* x, int32_t x_f16, const void* w_f16, const float* bias, const float* residual,
                   const float* row_scale, void* out, int32_t out_f16, int64_t m, int32_t n, int32_t cin, int32_t cin_pad,
                   int32_t taps, int32_t lda, int32_t ldc, int32_t ldr, int32_t t_in, int32_t t_out,
                   int32_t stride, int32_t dil, int32_t pad, int32_t act, float alpha, float slope, const int32_t* in_lens,
                   int64_t plan_m, astts_stream_t stream) {
    const int rc = check_gemm_args(who, (const float*)x, w_f16, (float*)out, m, n, cin, cin_pad, taps, t_in, t_out, stride, dil, act);
    if (rc != ASTTS_OK) return rc;
    GemmArgs a = gemm_args(x, w_f16, out, m, n, cin, lda, ldc);
    a.bias = bias;
    a.residual = residual;
    a.row_scale = row_scale;
    a.cin_pad = cin_pad;
    a.taps = taps;
    a.ldr = ldr;
    a.t_in = t_in;
    a.t_out = t_out;
    a.stride = stride;
    a.dil = dil;
    a.pad = pad;
    a.act = act;
    a.alpha = alpha;
    a.slope = slope;
    a.x_f16 = x_f16 ? 1 : 0;
    a.out_f16 = out_f16 ? 1 : 0;
    a.in_lens = in_lens;
    return launch_gemm(a, (hipStream_t)stream, plan_m);
}

int astts_op_gemm(const void* x, int32_t x_f16, const void* w_f16, const float* bias, const float* residual,
                  const float* row_scale, void* out, int32_t out_f16, int64_t m, int32_t n, int32_t cin, int32_t cin_pad,
                  int32_t taps, int32_t lda, int32_t ldc, int32_t ldr, int32_t t_in, int32_t t_out,
                  int32_t stride, int32_t dil, int32_t pad, int32_t act, float alpha, float slope, const int32_t* in_lens,
                  astts_stream_t stream) {
    return op_gemm("astts_op_gemm", x, x_f16, w_f16, bias, residual, row_scale, out, out_f16, m, n, cin, cin_pad, taps, lda, ldc, ldr, t_in,
                   t_out, stride, dil, pad, act, alpha, slope, in_lens, 0, stream);
}

int astts_op_gemm_planned(const void* x, int32_t x_f16, const void* w_f16, const float* bias, const float* residual,
                          const float* row_scale, void* out, int32_t out_f16, int64_t m, int32_t n, int32_t cin, int32_t cin_pad,
                          int32_t taps, int32_t lda, int32_t ldc, int32_t ldr, int32_t t_in, int32_t t_out,
                          int32_t stride, int32_t dil, int32_t pad, int32_t act, float alpha, float slope, const int32_t* in_lens,
                          int64_t plan_m, astts_stream_t stream) {
    ASTTS_REQUIRE(plan_m >= 1 && plan_m <= m, ASTTS_ERR_INVALID, "astts_op_gemm_planned: plan_m=%lld (1 .. m=%lld)", (long long)plan_m,
                  (long long)m);
    return op_gemm("astts_op_gemm_planned", x, x_f16, w_f16, bias, residual, row_scale, out, out_f16, m, n, cin, cin_pad, taps, lda, ldc, ldr,
                   t_in, t_out, stride, dil, pad, act, alpha, slope, in_lens, plan_m, stream);
}

int astts_op_gemm_rows(const void* x, int32_t x_f16, const void* w_f16,
                       const float* bias, const float* residual, void* out, int32_t out_f16, void* out2, int32_t out2_f16, int32_t m, int32_t n,
                       int32_t n_split, int32_t k, int32_t lda, int32_t ldc, int32_t ldc2, int32_t ldr, int32_t act, astts_stream_t stream) {
    ASTTS_REQUIRE(x && w_f16 && out, ASTTS_ERR_INVALID, "astts_op_gemm_rows: null pointer");
    ASTTS_REQUIRE(m >= 1 && m <= 4096 && n >= 1 && k >= 64 && (k % 64) == 0, ASTTS_ERR_UNSUPPORTED,
                  "astts_op_gemm_rows: m=%d n=%d k=%d (1 <= m <= 4096 rows, k a multiple of 64)", m, n, k);
    ASTTS_REQUIRE((lda % (x_f16 ? 8 : 4)) == 0 && (((uintptr_t)x | (uintptr_t)w_f16) & 15) == 0 && lda >= k && ldc >= (out2 ? n_split : n) &&
                      (!residual || ldr >= n),
                  ASTTS_ERR_INVALID, "astts_op_gemm_rows: operands must be 16-byte aligned (lda=%d), ld* >= the row's width", lda);
    ASTTS_REQUIRE(!out2 || (n_split >= 1 && n_split < n && ldc2 >= n - n_split), ASTTS_ERR_INVALID,
                  "astts_op_gemm_rows: split output needs 1 <= n_split=%d < n=%d and ldc2=%d >= n - n_split", n_split, n, ldc2);
    ASTTS_REQUIRE(act >= ACT_NONE && act <= ACT_LEAKY, ASTTS_ERR_INVALID, "astts_op_gemm_rows: act=%d", act);
    GemmArgs a = gemm_args(x, w_f16, out, m, n, k, lda, ldc);
    a.bias = bias;
    a.residual = residual;
    a.ldr = ldr;
    a.act = act;
    a.out2 = (float*)out2;
    a.ldc2 = ldc2;
    a.n_split = n_split;
    a.x_f16 = x_f16 ? 1 : 0;
    a.out_f16 = out_f16 ? 1 : 0;
    a.out2_f16 = out2_f16 ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const RowsPlan p = gemm_rows_plan(m, n, k, x_f16 != 0);
    const bool prof = prof_begin(ASTTS_PROF_GEMM_TILE, st, 2.0 * (double)m * n * k);
    bool launched = false;      // (PL = 8 is instantiated for fp16 rows only: fp32 rows hold twice the registers)
    if (x_f16) {
        if (p.pl == 2) launched = launch_rows_pl<2, false>(p, a, st);
        else if (p.pl == 4) launched = launch_rows_pl<4, false>(p, a, st);
        else if (p.pl == 8) launched = launch_rows_pl<8, false>(p, a, st);
    } else {
        if (p.pl == 2) launched = launch_rows_pl<2, true>(p, a, st);
        else if (p.pl == 4) launched = launch_rows_pl<4, true>(p, a, st);
    }
    if (prof) prof_end(ASTTS_PROF_GEMM_TILE, st);
    ASTTS_REQUIRE(launched, ASTTS_ERR_UNSUPPORTED, "astts_op_gemm_rows: no kernel for the plan PL=%d RT=%d CT=%d (x_f16=%d)", p.pl, p.rt, p.ct,
                  x_f16);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_op_gemm_ln(const void* x_f16, const void* w_f16, const float* bias, const float* residual, float* out,
                     const float* ln_gamma, const float* ln_beta, float ln_eps, void* ln_out_f16, int64_t m, int32_t n, int32_t cin,
                     int32_t cin_pad, int32_t lda, int32_t ldc, int32_t ldr, int32_t ld_ln, astts_stream_t stream) {
    const int rc = check_gemm_args("astts_op_gemm_ln", (const float*)x_f16, w_f16, out, m, n, cin, cin_pad, 1, (int32_t)m, (int32_t)m, 1, 1,
                                   ASTTS_ACT_NONE);
    if (rc != ASTTS_OK) return rc;
    ASTTS_REQUIRE(ln_gamma && ln_beta && ln_out_f16, ASTTS_ERR_INVALID, "astts_op_gemm_ln: null pointer");
    ASTTS_REQUIRE(n == 256 && cin == cin_pad, ASTTS_ERR_UNSUPPORTED,
                  "astts_op_gemm_ln: n=%d cin=%d (a workgroup owns whole output rows: n must be 256, cin a multiple of 64)", n, cin);
    ASTTS_REQUIRE((lda & 7) == 0 && (ldc & 3) == 0 && (ld_ln & 3) == 0 && (!residual || (ldr & 3) == 0) &&
                      (((uintptr_t)x_f16 | (uintptr_t)out | (uintptr_t)ln_out_f16 | (uintptr_t)residual | (uintptr_t)bias |
                        (uintptr_t)ln_gamma | (uintptr_t)ln_beta) & 15) == 0,
                  ASTTS_ERR_INVALID, "astts_op_gemm_ln: operands must be 16-byte aligned with 16-byte row strides");
    GemmArgs a = gemm_args(x_f16, w_f16, out, m, n, cin, lda, ldc);
    a.bias = bias;
    a.residual = residual;
    a.cin_pad = cin_pad;
    a.ldr = ldr;
    a.ln_gamma = ln_gamma;
    a.ln_beta = ln_beta;
    a.ln_eps = ln_eps;
    a.out2 = (float*)ln_out_f16;     // LayerNorm(out) as fp16, row stride ld_ln
    a.ldc2 = ld_ln;
    a.x_f16 = 1;
    a.out2_f16 = 1;
    hipStream_t st = (hipStream_t)stream;
    const bool prof = prof_begin(ASTTS_PROF_GEMM_TILE, st, 2.0 * (double)m * n * cin);
    launch_ring<1, 2, 3, 4>(a, st);         // the row-complete tile: 32 rows x all 256 columns per workgroup (n == 256 checked above: ceil(m / 32) workgroups)
    if (prof) prof_end(ASTTS_PROF_GEMM_TILE, st);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

size_t astts_op_gemm_fused_workspace_bytes(void) {
    return 1024 + (size_t)128 * 4 * 512 * sizeof(float);      // arrival counters + [128 column blocks][4 slices][512] partial sums
}

int astts_op_gemm_fused(const float* x, const int32_t* gather, const float* ln_gamma, const float* ln_beta, float ln_eps,
                        const void* w_f16, const float* bias, const float* residual, float* out, void* out2, int32_t out2_f16,
                        int32_t m, int32_t n, int32_t n_split, int32_t cin, int32_t cin_pad, int32_t lda, int32_t ldc,
                        int32_t ldc2, int32_t ldr, int32_t act, float alpha, float slope, void* workspace, size_t workspace_bytes,
                        astts_stream_t stream) {
    const int rc = check_gemm_args("astts_op_gemm_fused", x, w_f16, out, m, n, cin, cin_pad, 1, 1, 1, 1, 1, act);
    if (rc != ASTTS_OK) return rc;
    ASTTS_REQUIRE(m <= 32, ASTTS_ERR_INVALID, "astts_op_gemm_fused: m=%d > 32", m);
    ASTTS_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), ASTTS_ERR_INVALID, "astts_op_gemm_fused: gamma/beta");
    ASTTS_REQUIRE(!out2 || (n_split > 0 && n_split < n), ASTTS_ERR_INVALID, "astts_op_gemm_fused: n_split=%d", n_split);
    ASTTS_REQUIRE(!workspace || (workspace_bytes >= astts_op_gemm_fused_workspace_bytes() && ((uintptr_t)workspace & 255) == 0),
                  ASTTS_ERR_WORKSPACE, "astts_op_gemm_fused: workspace too small or misaligned");
    GemmArgs a = gemm_args(x, w_f16, out, m, n, cin, lda, ldc);
    a.bias = bias;
    a.residual = residual;
    a.cin_pad = cin_pad;
    a.ldr = ldr;
    a.act = act;
    a.alpha = alpha;
    a.slope = slope;
    a.gather = gather;
    a.ln_gamma = ln_gamma;
    a.ln_beta = ln_beta;
    a.ln_eps = ln_eps;
    a.out2 = (float*)out2;
    a.ldc2 = ldc2;
    a.n_split = n_split;
    a.out2_f16 = out2_f16 ? 1 : 0;
    if (workspace) {      // split-K: arrival counters in the first 1024 bytes, the partial sums behind them
        a.sk_cnt = reinterpret_cast<unsigned*>(workspace);
        a.sk_part = reinterpret_cast<float*>((char*)workspace + 1024);
    }
    return launch_gemm(a, (hipStream_t)stream);
}

}  // extern "C"
