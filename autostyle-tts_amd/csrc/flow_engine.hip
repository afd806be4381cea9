// flow_engine.hip -- Euler solver of the flow-matching decoder, host side in C++.
//
// The reference's hot loop #3: ConditionalCFM.solve_euler -> ConditionalDecoder.forward
// (cosyvoice/flow/flow_matching.py, cosyvoice/flow/decoder.py [EXT]; reached from tts_with_rag.py:195).
// One solve = n_steps x (2 down + 12 mid + 2 up) U-Net blocks, each a ResnetBlock1D and 4 transformer
// blocks: ~520 launches per step.  A Python host needs as long to enqueue them (~10 us each) as the GPU
// needs to run them, which both caps the stage and starves the other pipeline threads of the GIL; this
// engine issues the same operator sequence (astts_op_gemm / groupnorm / layernorm /
// attn_mha_ex / elementwise: bit-identical results to the operator-by-operator path) from C++.
//
// Data layout: activations [2b, t, C] row-major (time-major rows, channels contiguous), rows [0, b) the
// guided half, rows [b, 2b) the unguided half (mu / spk / cond read as zero).  The residual stream is
// fp32; tensors consumed only by MFMA operands (GroupNorm-1 / LayerNorm / qkv / attention / GELU
// outputs) are fp16.
#include "common.h"
#include "flow_session.h"
#include "flow_share.h"
#include "../../include/session/astts_flow_session.h"
#include "../../include/session/astts_flow_share.h"

#include <cstdlib>
#include <utility>
#include <vector>

struct astts_flow {
    astts_flow_config_t cfg;
    struct Block {
        astts_flow_resnet_t res;
        std::vector<astts_flow_tfm_t> tfm;
        astts_weight_t resample;
        int kind;
    };
    std::vector<Block> down, mid, up;
};

namespace astts {

// h[r, :] = [x | mu | spk | cond] for the guided half, [x | 0 | 0 | 0] for the unguided half; 0 beyond lens.
__global__ __launch_bounds__(256) void flow_pack_input(const float* __restrict__ x, const float* __restrict__ mu,
                                                      const float* __restrict__ spk, const float* __restrict__ cond,
                                                      const int* __restrict__ lens2, float* __restrict__ out, int b, int t,
                                                      int mel) {
    const int c4 = 4 * mel;
    const int64_t total = (int64_t)2 * b * t * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % c4);
        const int64_t row = i / c4;
        const int bb = (int)(row / t), tt = (int)(row % t);
        const int src_b = bb < b ? bb : bb - b;
        const int part = c / mel, cc = c % mel;
        float v = 0.0f;
        if (tt < lens2[bb]) {
            const int64_t o = ((int64_t)src_b * t + tt) * mel + cc;
            if (part == 0) v = x[o];
            else if (bb < b) v = part == 1 ? mu[o] : (part == 2 ? spk[(int64_t)src_b * mel + cc] : cond[o]);
        }
        out[i] = v;
    }
}

// out[b, t, 0:C] = a[b * a_bs + t * C + c] (first t steps of a longer tensor), out[b, t, C:2C] = skip; 0 beyond lens.
__global__ __launch_bounds__(256) void flow_concat_skip(const float* __restrict__ a, int64_t a_bs, const float* __restrict__ skip,
                                                       const int* __restrict__ lens, float* __restrict__ out, int b2, int t, int c) {
    const int c4 = c / 4;
    const int64_t total = (int64_t)b2 * t * 2 * c4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cc = (int)(i % (2 * c4));
        const int64_t row = i / (2 * c4);
        const int bb = (int)(row / t), tt = (int)(row % t);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tt < lens[bb]) {
            if (cc < c4) v = reinterpret_cast<const float4*>(a + (int64_t)bb * a_bs + (int64_t)tt * c)[cc];
            else v = reinterpret_cast<const float4*>(skip + row * c)[cc - c4];
        }
        reinterpret_cast<float4*>(out)[i] = v;
    }
}

// lens arrays of the 2b batch at both time resolutions (+ the per-step time value broadcast)
__global__ void flow_fill_lens(const int* __restrict__ lens, int* __restrict__ lens_full, int* __restrict__ lens_half, int b, int t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * b) {
        const int l = lens ? lens[i < b ? i : i - b] : t;
        lens_full[i] = l;
        lens_half[i] = (l + 1) / 2;
    }
}

__global__ void flow_fill_time(float* __restrict__ tv, float value, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tv[i] = value;
}

// ops_gemm.hip: what gemm_plan reads of an astts_op_gemm call, m aside
GemmShape gemm_shape_of_call(const void* x, int x_f16, int out_f16, int n, int cin, int cin_pad, int taps, int lda, int t_in, int t_out,
                             int stride, int pad);

static inline int grid_for(int64_t total) {
    int64_t g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : g);
}

}  // namespace astts

using namespace astts;

#define RUN(expr)                          \
    do {                                   \
        const int rc_ = (expr);            \
        if (rc_ != ASTTS_OK) return rc_;   \
    } while (0)

namespace {

constexpr int FLOW_MAX_STEPS = 32;   // Euler steps whose time embeddings / projections are precomputed (the reference runs 10)

// hands out 256-byte aligned pieces of a workspace; base == nullptr only counts (cv.o: the bytes taken so far)
struct Carver {
    char* base;
    size_t o;
    template <class T>
    T* take(size_t n) {
        T* p = base ? (T*)(base + o) : nullptr;
        o = align_up(o + sizeof(T) * n, 256);
        return p;
    }
};

// where the time path of one batch lives: the rows of `steps` Euler steps x its 2 b sequences
struct TimeBufs {
    float *temb0, *temb1, *temb2, *tproj, *tv;
};

// the one carve of a time path, for a lone solve (FLOW_MAX_STEPS steps, inside carve) and for every slot of a session
TimeBufs carve_time(Carver& cv, const astts_flow* h, size_t steps, size_t b2) {
    const astts_flow_config_t& c = h->cfg;
    const size_t n_res = h->down.size() + h->mid.size() + h->up.size(), trows = steps * b2;
    TimeBufs T;
    T.temb0 = cv.take<float>(trows * c.time_in);
    T.temb1 = cv.take<float>(trows * c.time_dim);
    T.temb2 = cv.take<float>(trows * c.time_dim);
    T.tproj = cv.take<float>(n_res * trows * c.channels);
    T.tv = cv.take<float>(trows);
    return T;
}

struct Buffers {
    float *xin, *r1, *r2, *r3, *pool[6], *d, *up;
    TimeBufs T;     // of a lone solve: all Euler steps at once; T.tproj of a joined pass: the projections gathered by flow_join_assemble
    _Float16 *r1h, *n16, *qkv16, *a16, *f16;
    int *lens_full, *lens_half;
    void* gn_ws;
    size_t gn_ws_bytes;
    float *rstat1, *rstat2;   // astts_op_resnet_conv: per-tile GroupNorm statistics of conv 1 / conv 2
};

// one carve-up serves astts_flow_workspace_bytes (a counting Carver) and astts_flow_solve
Buffers carve(Carver& cv, const astts_flow* h, int b, int t) {
    const astts_flow_config_t& c = h->cfg;
    const size_t b2 = 2 * (size_t)b, rows = b2 * t, C = c.channels, hd = (size_t)c.heads * 64;
    const size_t in_ch = 4 * (size_t)c.mel > 2 * C ? 4 * (size_t)c.mel : 2 * C;
    Buffers X;
    X.xin = cv.take<float>(rows * in_ch);
    X.r1 = cv.take<float>(rows * C);
    X.r2 = cv.take<float>(rows * C);
    X.r3 = cv.take<float>(rows * C);
    for (int i = 0; i < 6; ++i) X.pool[i] = cv.take<float>(rows * C);
    X.up = cv.take<float>(b2 * ((size_t)t + 4) * 2 * C);
    X.r1h = cv.take<_Float16>(rows * C);
    X.n16 = cv.take<_Float16>(rows * C);
    X.qkv16 = cv.take<_Float16>(rows * 3 * hd);
    X.a16 = cv.take<_Float16>(rows * hd);
    X.f16 = cv.take<_Float16>(rows * 4 * C);
    // the time path does not depend on x: it is evaluated for ALL Euler steps before the first one (FLOW_MAX_STEPS rows blocks)
    X.T = carve_time(cv, h, FLOW_MAX_STEPS, b2);
    X.d = cv.take<float>(rows * c.mel);
    X.lens_full = cv.take<int>(b2);
    X.lens_half = cv.take<int>(b2);
    X.gn_ws_bytes = astts_op_groupnorm_workspace_bytes((int)b2, t, c.groups);
    X.gn_ws = cv.take<char>(X.gn_ws_bytes > 16 ? X.gn_ws_bytes : 16);
    X.rstat1 = cv.take<float>(astts_op_resnet_conv_stats_floats((int32_t)b2, t));
    X.rstat2 = cv.take<float>(astts_op_resnet_conv_stats_floats((int32_t)b2, t));
    return X;
}

// does this ResNet block take the three-launch path (astts_op_resnet_conv)?  Ctx::resnet and the prefetch hint of the mid loop ask here
bool resnet_fused(const astts_flow_resnet_t& r, int groups) {
    auto served = [&](const astts_weight_t& w) { return astts_op_resnet_conv_supported(w.cin, w.n, groups, w.taps) != 0; };
    return r.c1_frag && r.c2_frag && r.res_frag && served(r.c1) && served(r.c2) && served(r.res);
}

// bytes of a weight's fp16 image (row-major or fragment order: the same count), as a prefetch hint's length
uint32_t weight_bytes(const astts_weight_t& w) { return (uint32_t)((size_t)w.n * w.taps * w.cin_pad * 2); }

// one batch's share of an estimator pass: its own tensors, its sequences [seq0, seq0 + 2 b) of the pass, its Euler step
struct Seg {
    float* x;
    const float *mu, *spk, *cond;
    int seq0, b;
    float dt, cfg_rate;
};

struct Ctx {
    const astts_flow* const h;
    const Buffers B;
    const int b2, T;    // b2: sequences of the pass (all batches')
    const bool full;    // no sequence is shorter than T: the length masks are not launched
    const astts_stream_t st;
    const Seg* const seg;   // the batches of the pass, one after the other without gaps; astts_flow_solve: one
    const int n_seg;
    const bool share;   // a joined pass issues ONE feed-forward launch and one GEMM launch per group of equal plans (flow_share.h)

    Ctx(const astts_flow* h, const Buffers& B, int t, bool full, astts_stream_t st, const Seg* seg, int n_seg, bool share)
        : h(h), B(B), b2(seg[n_seg - 1].seq0 + 2 * seg[n_seg - 1].b), T(t), full(full), st(st), seg(seg), n_seg(n_seg), share(share) {}

    // a plain projection of `rows` rows, one launch whatever the pass carries (the time path)
    int linear(const void* x, int x16, const astts_weight_t& w, const float* residual, void* out, int out16, int64_t rows, int act) const {
        return astts_op_gemm(x, x16, w.w, w.bias, residual, nullptr, out, out16, rows, w.n, w.cin, w.cin_pad, w.taps, w.cin, w.n,
                             residual ? w.n : 0, (int)rows, (int)rows, 1, 1, 0, act, 1.0f, 0.1f, nullptr, st);
    }
    // a convolution over all sequences ([b2, t_in, cin] -> [b2, t_out, n]).  launch_gemm plans kernel family and tile from the row count
    // (gemm_plan.h), and a row's sum depends on the kernel, not on where its tile lies.  A joined pass therefore groups consecutive
    // batches whose plans FOR THEIR OWN ROW COUNTS are equal (gemm_share_groups) and issues one launch per group with that plan
    // (astts_op_gemm_planned): the kernel each of them gets alone, over the rows of all.  Batches whose plans differ, and the m <= 32
    // family, stay separate.  So does every GEMM with an activation: the epilogue of a tile that lies wholly inside the output evaluates
    // GELU with gelu_erf_fast, the epilogue of an edge tile with erff (gemm_kernels.h), so a batch's last rows would change their bits when
    // another batch's rows complete their tile (the unfused feed-forward's W1; found by the tiny-width session tests).
    // A lone batch is one group planned by its own row count: the launch of astts_op_gemm.
    // `rows_as_one`: a projection of rows (proj()), which a launch takes as ONE sequence of all its rows.
    int gemm(const void* x, int x16, const astts_weight_t& w, const float* residual, void* out, int out16, int t_in, int t_out, int stride,
             int pad, int act, bool rows_as_one = false) const {
        int64_t rows[FlowSessionPlan::kSlots];
        for (int i = 0; i < n_seg; ++i) rows[i] = 2 * (int64_t)seg[i].b * t_out;
        const GemmGroups G = gemm_share_groups(gemm_shape_of_call(x, x16, out16, w.n, w.cin, w.cin_pad, w.taps, w.cin, t_in, t_out, stride, pad),
                                               n_seg, rows, share && act == ASTTS_ACT_NONE);
        for (int g = 0; g < G.n; ++g) {
            const int64_t s0 = seg[G.first[g]].seq0;
            int64_t gm = 0;
            for (int i = 0; i < G.count[g]; ++i) gm += rows[G.first[g] + i];
            const int ti = rows_as_one ? (int)gm : t_in, to = rows_as_one ? (int)gm : t_out;
            RUN(astts_op_gemm_planned((const char*)x + s0 * t_in * w.cin * (x16 ? 2 : 4), x16, w.w, w.bias, residual ? residual + s0 * t_out * w.n : nullptr,
                                      nullptr, (char*)out + s0 * t_out * w.n * (out16 ? 2 : 4), out16, gm, w.n, w.cin, w.cin_pad, w.taps, w.cin, w.n,
                                      residual ? w.n : 0, ti, to, stride, 1, pad, act, 1.0f, 0.1f, nullptr, G.plan_m[g], st));
        }
        return ASTTS_OK;
    }
    // a projection of the rows of all sequences ([b2 * t, cin] -> [b2 * t, n]): grouped by plan in a joined pass, as gemm()
    int proj(const void* x, int x16, const astts_weight_t& w, const float* residual, void* out, int out16, int t, int act) const {
        return gemm(x, x16, w, residual, out, out16, t, t, 1, 0, act, true);
    }
    // the rows of every batch of the pass at t frames per sequence, for the segmented feed-forward launch
    void seg_rows(int t, int64_t* row0, int64_t* rows) const {
        for (int i = 0; i < n_seg; ++i) {
            row0[i] = (int64_t)seg[i].seq0 * t;
            rows[i] = 2 * (int64_t)seg[i].b * t;
        }
    }
    // GroupNorm (+ time projection, Mish) of all sequences: astts_op_groupnorm sizes its grid by the sequence count, so per batch too
    int gnorm(const float* x, const int* lens, const float* gw, const float* gb, const float* add_bc, void* y, int y16, int t) const {
        const int C = h->cfg.channels, G = h->cfg.groups;
        for (int i = 0; i < n_seg; ++i) {
            const int64_t s0 = seg[i].seq0;
            RUN(astts_op_groupnorm(x + s0 * t * C, lens + s0, gw, gb, add_bc ? add_bc + s0 * C : nullptr, (char*)y + s0 * t * C * (y16 ? 2 : 4),
                                   y16, 2 * seg[i].b, t, C, G, 1e-5f, 1, B.gn_ws, B.gn_ws_bytes, st));
        }
        return ASTTS_OK;
    }
    int mask(float* x, const int* lens, int t, int c) const {
        if (full) return ASTTS_OK;
        return astts_op_elementwise(ASTTS_EL_MUL_ROWMASK, x, nullptr, nullptr, lens, x, (int64_t)b2 * t * c, t, c, 0.0f, 0.0f, st);
    }

    // the q|k|v image of one transformer block
    uint32_t qkv_bytes() const { return 3u * (uint32_t)h->cfg.heads * 64u * (uint32_t)h->cfg.channels * 2u; }

    // ResnetBlock1D on x [b2, t, cin] (already masked) -> out [b2, t, C]
    // `tproj` [b2, C]: this block's time projection for the current Euler step (precomputed for all steps by astts_flow_solve)
    // `next_w` / `next_bytes`: the weight image the launch after this block reads first (its first transformer block's q|k|v image)
    int resnet(const astts_flow_resnet_t& r, const float* tproj, const float* x, const int* lens, int t, float* out,
               const void* next_w = nullptr, uint32_t next_bytes = 0) const {
        if (resnet_fused(r, h->cfg.groups)) {
            // three launches, GroupNorm + Mish folded into the convolutions (ops_resnet_conv.hip)
            // every launch requests the NEXT one's (cold) weights into L2 while it runs
            RUN(astts_op_resnet_conv(x, r.c1_frag, r.c1.bias, B.r1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     B.rstat1, lens, b2, t, r.c1.cin, r.c1.taps, 1e-5f, r.c2_frag, weight_bytes(r.c2), st));
            RUN(astts_op_resnet_conv(B.r1, r.c2_frag, r.c2.bias, B.r2, B.rstat1, r.g1_w, r.g1_b, tproj, nullptr, nullptr, nullptr, nullptr,
                                     B.rstat2, lens, b2, t, r.c2.cin, r.c2.taps, 1e-5f, r.res_frag, weight_bytes(r.res), st));
            return astts_op_resnet_conv(x, r.res_frag, r.res.bias, out, nullptr, nullptr, nullptr, nullptr, B.r2, B.rstat2, r.g2_w, r.g2_b,
                                        nullptr, lens, b2, t, r.res.cin, r.res.taps, 1e-5f, next_w, next_bytes, st);
        }
        RUN(gemm(x, 0, r.c1, nullptr, B.r1, 0, t, t, 1, 1, ASTTS_ACT_NONE));
        RUN(gnorm(B.r1, lens, r.g1_w, r.g1_b, tproj, B.r1h, 1, t));
        RUN(gemm(B.r1h, 1, r.c2, nullptr, B.r2, 0, t, t, 1, 1, ASTTS_ACT_NONE));
        RUN(gnorm(B.r2, lens, r.g2_w, r.g2_b, nullptr, B.r3, 0, t));
        return gemm(x, 0, r.res, B.r3, out, 0, t, t, 1, 0, ASTTS_ACT_NONE);     // res_conv(x) + h
    }

    // BasicTransformerBlock: x (in p) -> result back in p, q is scratch of the same size
    // `next_w` / `next_bytes`: the weight image the launch AFTER this block reads first (the next block's q|k|v image, or the next
    // ResNet's first convolution): prefetched into L2 by the feed-forward launch
    int tfm(const astts_flow_tfm_t& w, float* p, float* q, const int* lens, int t, const void* next_w = nullptr, uint32_t next_bytes = 0) const {
        const int C = h->cfg.channels, heads = h->cfg.heads, hd = heads * 64;
        const int64_t rows = (int64_t)b2 * t;
        if (w.qkv_frag && astts_op_tfm_attn_fused_supported(C, heads, t)) {      // LayerNorm + q|k|v + attention in one launch (ops_tfm_fused.hip)
            // the feed-forward launch that follows streams 1.25 MB of weights no launch has touched since the last Euler step:
            // requested into L2 from here
            const void* pf[3] = {w.wo_frag, w.w1_frag, w.w2_frag};
            const uint32_t pfb[3] = {(uint32_t)((size_t)C * hd * 2), (uint32_t)((size_t)w.w1.n * C * 2), (uint32_t)((size_t)C * w.w1.n * 2)};
            RUN(astts_op_tfm_attn_fused(p, w.qkv_frag, w.qkv.bias, lens, B.a16, b2, heads, t, C, 1e-5f, 0.125f, pf, pfb,
                                        (w.wo_frag && w.w1_frag && w.w2_frag) ? 3 : 0, st));
        } else {
            RUN(astts_op_layernorm(p, w.n1_w, w.n1_b, B.n16, 1, rows, C, C, C, 1e-5f, 0.0f, st));
            RUN(proj(B.n16, 1, w.qkv, nullptr, B.qkv16, 1, t, ASTTS_ACT_NONE));
            RUN(astts_op_attn_mha(B.qkv16, B.qkv16 + hd, B.qkv16 + 2 * hd, 1, lens, B.a16, 1, b2, heads, t, 3 * hd, 3 * hd, hd,
                                  0.125f, st));
        }
        const bool ffn = w.w1_frag && w.w2_frag && astts_op_tfm_ffn_fused_supported(C, w.w1.n);
        // output projection + residual + LayerNorm + W1 + GELU + W2 + residual in one launch (in place on p); faster than the
        // separate projection at every row count measured (5 504: 20.2 vs 26.8 us, 11 008: 36.6 vs 45.0, 44 032: 116 vs 128)
        // tfm_ffn_fused sums the hidden chunks in an order rotated by the tile's index (a 32-row tile starts at chunk (tile / 8) % chunks):
        // a row's bits depend on where its tile lies.  A joined pass issues ONE launch over a segment table (astts_op_tfm_ffn_fused_seg):
        // every batch's rows are cut into tiles of their own, counted from the batch's first tile, so each row runs what it runs when
        // its batch is launched alone; the launch prefetches next_w.  ASTTS_FLOW_SHARE=0 (share == false) restores one launch per batch.
        // What stays per batch in a joined pass: astts_op_groupnorm (its grid form depends on the sequence count; three launches per
        // pass), flow_pack_input and the CFG-Euler update (each batch's own tensors), and GEMMs whose plans differ (gemm()).
        const bool ffn_wo = ffn && w.wo_frag && (hd == 256 || hd == 512);
        if (!ffn_wo) RUN(proj(B.a16, 1, w.wo, p, q, 0, t, ASTTS_ACT_NONE));
        if (ffn) {    // (output projection + residual +) LayerNorm + W1 + GELU + W2 + residual: one launch, in place on p with the projection
            const float* in = ffn_wo ? p : q;
            const _Float16* attn = ffn_wo ? B.a16 : nullptr;
            const void* wo = ffn_wo ? w.wo_frag : nullptr;
            const float* bo = ffn_wo ? w.wo.bias : nullptr;
            const int k0 = ffn_wo ? hd : 0;
            int64_t row0[FlowSessionPlan::kSlots], nrows[FlowSessionPlan::kSlots];
            seg_rows(t, row0, nrows);
            if (share && n_seg > 1)
                return astts_op_tfm_ffn_fused_seg(in, w.w1_frag, w.w1.bias, w.w2_frag, w.w2.bias, p, n_seg, row0, nrows, C, w.w1.n, 1e-5f, attn, wo,
                                                  bo, k0, ffn_wo ? next_w : nullptr, ffn_wo ? next_bytes : 0u, st);
            for (int i = 0; i < n_seg; ++i) {
                const bool last = ffn_wo && i + 1 == n_seg;
                RUN(astts_op_tfm_ffn_fused(in + row0[i] * C, w.w1_frag, w.w1.bias, w.w2_frag, w.w2.bias, p + row0[i] * C, nrows[i], C, w.w1.n, 1e-5f,
                                           attn ? attn + row0[i] * hd : nullptr, wo, bo, k0, last ? next_w : nullptr, last ? next_bytes : 0u, st));
            }
            return ASTTS_OK;
        }
        RUN(astts_op_layernorm(q, w.n3_w, w.n3_b, B.n16, 1, rows, C, C, C, 1e-5f, 0.0f, st));
        RUN(proj(B.n16, 1, w.w1, nullptr, B.f16, 1, t, ASTTS_ACT_GELU));
        return proj(B.f16, 1, w.w2, q, p, 0, t, ASTTS_ACT_NONE);
    }

    // One U-Net block: ResNet `in` -> `out` (never in place: every GEMM block reads whole input rows), the transformer chain on `out`
    // with `scratch` of the same size, the length mask.  Every launch chain prefetches what follows it: the ResNet the first transformer
    // block's q|k|v image, every transformer block the next one's, the last one `next_w` / `next_bytes` (what the caller runs next).
    int block(const astts_flow::Block& blk, const float* tproj, const float* in, float* out, float* scratch, const int* lens, int t,
              const void* next_w = nullptr, uint32_t next_bytes = 0) const {
        RUN(resnet(blk.res, tproj, in, lens, t, out, blk.tfm.empty() ? nullptr : blk.tfm[0].qkv_frag, qkv_bytes()));
        for (size_t ti = 0; ti < blk.tfm.size(); ++ti) {
            const bool more = ti + 1 < blk.tfm.size();
            RUN(tfm(blk.tfm[ti], out, scratch, lens, t, more ? blk.tfm[ti + 1].qkv_frag : next_w, more ? qkv_bytes() : next_bytes));
        }
        return mask(out, lens, t, h->cfg.channels);
    }
};

}  // namespace

extern "C" {

int astts_flow_create(const astts_flow_config_t* cfg, const astts_flow_block_t* down, const astts_flow_block_t* mid,
                      const astts_flow_block_t* up, astts_flow_t** out) {
    ASTTS_REQUIRE(cfg && down && mid && up && out, ASTTS_ERR_INVALID, "astts_flow_create: null argument");
    ASTTS_REQUIRE(cfg->mel >= 1 && cfg->channels >= 64 && cfg->channels % 64 == 0 && cfg->heads >= 1 && cfg->groups >= 1 &&
                      cfg->channels % cfg->groups == 0, ASTTS_ERR_INVALID, "astts_flow_create: bad sizes");
    ASTTS_REQUIRE(cfg->n_down >= 1 && cfg->n_down <= 4 && cfg->n_up == cfg->n_down && cfg->n_mid >= 0, ASTTS_ERR_INVALID,
                  "astts_flow_create: n_down=%d n_mid=%d n_up=%d", cfg->n_down, cfg->n_mid, cfg->n_up);
    int n_half = 0;
    for (int i = 0; i < cfg->n_down; ++i) n_half += down[i].resample_kind == ASTTS_FLOW_RESAMPLE_DOWN;
    ASTTS_REQUIRE(n_half <= 1, ASTTS_ERR_UNSUPPORTED, "astts_flow_create: more than one stride-2 level is not implemented");
    ASTTS_REQUIRE(down[cfg->n_down - 1].resample_kind == ASTTS_FLOW_RESAMPLE_CONV && up[cfg->n_up - 1].resample_kind == ASTTS_FLOW_RESAMPLE_CONV,
                  ASTTS_ERR_UNSUPPORTED, "astts_flow_create: the last down / up block must end in the k=3 convolution");
    astts_flow* h = new astts_flow();
    h->cfg = *cfg;
    auto copy = [](const astts_flow_block_t* src, int n, std::vector<astts_flow::Block>& dst) {
        for (int i = 0; i < n; ++i) {
            astts_flow::Block blk;
            blk.res = src[i].res;
            blk.tfm.assign(src[i].tfm, src[i].tfm + src[i].n_tfm);
            blk.resample = src[i].resample;
            blk.kind = src[i].resample_kind;
            dst.push_back(blk);
        }
    };
    copy(down, cfg->n_down, h->down);
    copy(mid, cfg->n_mid, h->mid);
    copy(up, cfg->n_up, h->up);
    *out = h;
    return ASTTS_OK;
}

int astts_flow_destroy(astts_flow_t* h) {
    delete h;
    return ASTTS_OK;
}

size_t astts_flow_workspace_bytes(const astts_flow_t* h, int32_t b, int32_t t) {
    if (!h || b < 1 || t < 1) return 0;
    Carver cv{nullptr, 0};
    carve(cv, h, b, t);
    return cv.o;
}

}  // extern "C"

namespace {

// The time path of `steps` Euler steps of the pass's one batch, hoisted out of the dependent chain (it depends on the schedule
// only): time embedding -> MLP -> Mish (every ResnetBlock1D applies Mish before its own projection) for all steps x b2 rows in one
// pass, then ONE projection GEMM per ResNet block over all steps: ~20 launches per solve instead of 21 per step.
// -> T.tproj [ResNet block][steps * b2][C]
int time_path(const Ctx& k, const TimeBufs& T, const float* t_host, int steps) {
    const astts_flow* h = k.h;
    const astts_flow_config_t& c = h->cfg;
    hipStream_t st = (hipStream_t)k.st;
    const int b2 = k.b2;
    const int64_t trows = (int64_t)steps * b2;
    for (int j = 0; j < steps; ++j) {
        hipLaunchKernelGGL(flow_fill_time, dim3((b2 + 63) / 64), dim3(64), 0, st, T.tv + (size_t)j * b2, t_host[j], b2);
        ASTTS_CHECK_LAUNCH();
    }
    RUN(astts_op_time_embedding(T.tv, T.temb0, (int)trows, c.time_in, 1000.0f, k.st));
    RUN(k.linear(T.temb0, 0, c.t1, nullptr, T.temb1, 0, trows, ASTTS_ACT_SILU));
    RUN(k.linear(T.temb1, 0, c.t2, nullptr, T.temb2, 0, trows, ASTTS_ACT_NONE));
    RUN(astts_op_elementwise(ASTTS_EL_MISH, T.temb2, nullptr, nullptr, nullptr, T.temb2, trows * c.time_dim, 1, c.time_dim, 0.0f, 0.0f, k.st));
    size_t rj = 0;
    for (const std::vector<astts_flow::Block>* grp : {&h->down, &h->mid, &h->up})
        for (const astts_flow::Block& blk : *grp)
            RUN(k.linear(T.temb2, 0, blk.res.mlp, nullptr, T.tproj + (rj++) * (size_t)trows * c.channels, 0, trows, ASTTS_ACT_NONE));
    return ASTTS_OK;
}

// One estimator pass over the k.b2 sequences of k.seg[0 .. k.n_seg), then every batch's own guidance + Euler update.
// `tproj` + i * tproj_stride: the [b2, C] time projections of ResNet block i (down, mid, up order) for this pass;
// `lens_full` / `lens_half` [b2]: the sequences' lengths at both time resolutions.
int estimator_pass(const Ctx& k, const float* tproj, size_t tproj_stride, const int* lens_full, const int* lens_half) {
    const astts_flow* h = k.h;
    const astts_flow_config_t& c = h->cfg;
    hipStream_t st = (hipStream_t)k.st;
    const Buffers& B = k.B;
    const int b2 = k.b2, t = k.T, C = c.channels, mel = c.mel;
    const int t_half = (t - 1) / 2 + 1;     // conv k=3, stride 2, pad 1
    size_t ri = 0;      // ResNet block counter of this estimator pass (down, mid, up order: the order of the table above)
    auto tproj_of = [&]() { return tproj + (ri++) * tproj_stride; };
    for (int i = 0; i < k.n_seg; ++i) {
        const Seg& g = k.seg[i];
        hipLaunchKernelGGL(flow_pack_input, dim3(grid_for((int64_t)2 * g.b * t * 4 * mel)), dim3(256), 0, st, g.x, g.mu, g.spk, g.cond,
                           lens_full + g.seq0, B.xin + (size_t)g.seq0 * t * 4 * mel, g.b, t, mel);
        ASTTS_CHECK_LAUNCH();
    }

    // buffer pool: cur / other ping-pong for the residual stream, the rest become skips
    float* pool[6];
    for (int i = 0; i < 6; ++i) pool[i] = B.pool[i];
    int n_free = 6;
    auto grab = [&]() { return pool[--n_free]; };
    float* cur = grab();
    float* other = grab();
    float* skips[4];
    int skip_t[4];
    const int* skip_lens[4];
    int n_skips = 0;
    const float* block_in = B.xin;
    int tt = t;
    const int* L = lens_full;

    for (const astts_flow::Block& blk : h->down) {
        RUN(k.block(blk, tproj_of(), block_in, other, cur, L, tt));
        skips[n_skips] = other;
        skip_t[n_skips] = tt;
        skip_lens[n_skips] = L;
        ++n_skips;
        const float* skip = other;
        other = grab();
        if (blk.kind == ASTTS_FLOW_RESAMPLE_DOWN) {
            RUN(k.gemm(skip, 0, blk.resample, nullptr, cur, 0, tt, t_half, 2, 1, ASTTS_ACT_NONE));
            tt = t_half;
            L = lens_half;
        } else {
            RUN(k.gemm(skip, 0, blk.resample, nullptr, cur, 0, tt, tt, 1, 1, ASTTS_ACT_NONE));
        }
        RUN(k.mask(cur, L, tt, C));
        block_in = cur;
    }
    for (size_t mi = 0; mi < h->mid.size(); ++mi) {
        // after the last transformer block of a mid block comes the next mid block's first convolution
        // (its fragment-order image when that ResNet block takes the three-launch path, else the row-major one)
        const astts_flow_resnet_t* nr = mi + 1 < h->mid.size() ? &h->mid[mi + 1].res : nullptr;
        const void* next_w = !nr ? nullptr : resnet_fused(*nr, c.groups) ? nr->c1_frag : nr->c1.w;
        RUN(k.block(h->mid[mi], tproj_of(), cur, other, cur, L, tt, next_w, nr ? weight_bytes(nr->c1) : 0u));
        std::swap(cur, other);
    }
    const float* up_src = cur;          // [b2, up_t >= skip t, C] with batch stride up_bs
    int64_t up_bs = (int64_t)tt * C;
    for (const astts_flow::Block& blk : h->up) {
        --n_skips;
        tt = skip_t[n_skips];
        L = skip_lens[n_skips];
        hipLaunchKernelGGL(flow_concat_skip, dim3(grid_for((int64_t)b2 * tt * 2 * (C / 4))), dim3(256), 0, st, up_src, up_bs,
                           skips[n_skips], L, B.xin, b2, tt, C);
        ASTTS_CHECK_LAUNCH();
        RUN(k.block(blk, tproj_of(), B.xin, cur, other, L, tt));
        if (blk.kind == ASTTS_FLOW_RESAMPLE_UP) {
            // phase-decomposed ConvTranspose1d: [b2 * (tt + 1), 2C] == [b2, 2 (tt + 1), C]; output step j is row 1 + j
            RUN(k.gemm(cur, 0, blk.resample, nullptr, B.up, 0, tt, tt + 1, 1, 1, ASTTS_ACT_NONE));
            up_src = B.up + C;
            up_bs = (int64_t)(tt + 1) * 2 * C;
        } else {
            RUN(k.gemm(cur, 0, blk.resample, nullptr, other, 0, tt, tt, 1, 1, ASTTS_ACT_NONE));
            std::swap(cur, other);
            up_src = cur;
            up_bs = (int64_t)tt * C;
        }
    }
    // final block at the full resolution (tt == t here: the last up block restores it)
    float* fin = const_cast<float*>(up_src);
    RUN(k.mask(fin, lens_full, t, C));
    RUN(k.gemm(fin, 0, c.fin_c, nullptr, B.r1, 0, t, t, 1, 1, ASTTS_ACT_NONE));
    RUN(k.gnorm(B.r1, lens_full, c.fin_g_w, c.fin_g_b, nullptr, B.r3, 0, t));
    RUN(k.gemm(B.r3, 0, c.fin_p, nullptr, B.d, 0, t, t, 1, 0, ASTTS_ACT_NONE));
    RUN(k.mask(B.d, lens_full, t, mel));
    // x += dt * ((1 + r) d_cond - r d_uncond), every batch with its own dt and rate on its own sequences of d
    for (int i = 0; i < k.n_seg; ++i) {
        const Seg& g = k.seg[i];
        RUN(astts_op_elementwise(ASTTS_EL_CFG_EULER, g.x, B.d + (size_t)g.seq0 * t * mel, nullptr, nullptr, g.x, (int64_t)g.b * t * mel, t, mel,
                                 g.dt, g.cfg_rate, k.st));
    }
    return ASTTS_OK;
}

}  // namespace

// What a joined pass reads of every batch it carries, passed by value: the batch's sequence range, where its time projections of all
// its steps and its lengths live, and the Euler step it is at.
struct FlowJoinTable {
    const float* tproj[astts::FlowSessionPlan::kSlots];
    const int* lens_full[astts::FlowSessionPlan::kSlots];
    const int* lens_half[astts::FlowSessionPlan::kSlots];
    int seq0[astts::FlowSessionPlan::kSlots], b2[astts::FlowSessionPlan::kSlots], trows[astts::FlowSessionPlan::kSlots],
        step[astts::FlowSessionPlan::kSlots];
    int n;
};

// the batch of the pass that sequence `seq` belongs to
__device__ inline int flow_join_batch_of(const FlowJoinTable& T, int seq) {
    int k = 0;
    while (k + 1 < T.n && seq >= T.seq0[k] + T.b2[k]) ++k;
    return k;
}

// tproj_out [n_res][nseq][C]: every sequence's time projection rows of its batch's CURRENT step, gathered into the contiguous block per
// ResNet block that the kernels read; lens_full / lens_half [nseq]: the batches' lengths side by side
__global__ __launch_bounds__(256) void flow_join_assemble(FlowJoinTable T, float* __restrict__ tproj_out, int* __restrict__ lens_full,
                                                         int* __restrict__ lens_half, int nseq, int n_res, int C) {
    const int64_t total = (int64_t)n_res * nseq * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cc = (int)(i % C);
        const int seq = (int)((i / C) % nseq);
        const int ri = (int)(i / ((int64_t)C * nseq));
        const int k = flow_join_batch_of(T, seq);
        const int j = seq - T.seq0[k];
        tproj_out[i] = T.tproj[k][((int64_t)ri * T.trows[k] + (int64_t)T.step[k] * T.b2[k] + j) * C + cc];
        if (ri == 0 && cc == 0) {       // one element per sequence writes its lengths
            lens_full[seq] = T.lens_full[k][j];
            lens_half[seq] = T.lens_half[k][j];
        }
    }
}

struct astts_flow_session {
    astts_flow* h;
    astts::FlowSessionPlan plan;
    astts_stream_t st;
    Buffers B;                      // of a pass over 2 * rows_max sequences
    struct Slot {
        Seg seg;
        TimeBufs T;                 // the batch's time path, all its steps
        int *lens_full, *lens_half; // [2 b]
        bool full;
        float dt[FLOW_MAX_STEPS];
    } slot[astts::FlowSessionPlan::kSlots];
    int passes, carried;            // passes enqueued; batches they carried (summed)
};

namespace {

// one carve-up serves astts_flow_session_bytes (a counting Carver) and astts_flow_session_create: the buffers of a pass over the
// session's maximum (carve), then every slot's time path and lengths
void carve_session(Carver& cv, astts_flow_session& S, int t, int n_slots, int rows_max, int steps_max) {
    S.B = carve(cv, S.h, rows_max, t);
    for (int i = 0; i < n_slots; ++i) {
        S.slot[i].T = carve_time(cv, S.h, steps_max, 2 * (size_t)rows_max);
        S.slot[i].lens_full = cv.take<int>(2 * (size_t)rows_max);
        S.slot[i].lens_half = cv.take<int>(2 * (size_t)rows_max);
    }
}

}  // namespace

extern "C" {

int astts_flow_solve(astts_flow_t* h, float* x, const float* mu, const float* spk, const float* cond, const int32_t* lens,
                     int32_t b, int32_t t, int32_t n_steps, const float* t_host, const float* dt_host, float cfg_rate,
                     void* workspace, size_t workspace_bytes, astts_stream_t stream) {
    ASTTS_REQUIRE(h && x && mu && spk && cond && t_host && dt_host && workspace, ASTTS_ERR_INVALID, "astts_flow_solve: null argument");
    ASTTS_REQUIRE(b >= 1 && t >= 2 && n_steps >= 1, ASTTS_ERR_INVALID, "astts_flow_solve: b=%d t=%d n_steps=%d", b, t, n_steps);
    ASTTS_REQUIRE(workspace_bytes >= astts_flow_workspace_bytes(h, b, t) && ((uintptr_t)workspace & 255) == 0,
                  ASTTS_ERR_WORKSPACE, "astts_flow_solve: workspace too small or misaligned");
    Seg seg{x, mu, spk, cond, 0, b, 0.0f, cfg_rate};
    Carver cv{(char*)workspace, 0};
    const Ctx k(h, carve(cv, h, b, t), t, lens == nullptr, stream, &seg, 1, false);
    const Buffers& B = k.B;
    const int b2 = k.b2, C = h->cfg.channels;

    hipLaunchKernelGGL(flow_fill_lens, dim3((b2 + 63) / 64), dim3(64), 0, (hipStream_t)stream, lens, B.lens_full, B.lens_half, b, t);
    ASTTS_CHECK_LAUNCH();

    // the time path of all steps before the first one (time_path); solves with more than FLOW_MAX_STEPS steps evaluate it chunk by
    // chunk (the workspace holds FLOW_MAX_STEPS steps)
    for (int s = 0; s < n_steps; ++s) {
        const int s0 = s - s % FLOW_MAX_STEPS, sl = s - s0;
        const int steps = n_steps - s0 < FLOW_MAX_STEPS ? n_steps - s0 : FLOW_MAX_STEPS;
        if (sl == 0) RUN(time_path(k, B.T, t_host + s0, steps));
        seg.dt = dt_host[s];
        RUN(estimator_pass(k, B.T.tproj + (size_t)sl * b2 * C, (size_t)steps * b2 * C, B.lens_full, B.lens_half));
    }
    return ASTTS_OK;
}

size_t astts_flow_session_bytes(const astts_flow_t* h, int32_t t, int32_t n_slots, int32_t rows_max, int32_t steps_max) {
    astts::FlowSessionPlan p;
    if (!h || p.init(t, n_slots, rows_max, steps_max) != astts::FLOW_SESSION_OK || steps_max > FLOW_MAX_STEPS) return 0;
    Carver cv{nullptr, 0};
    astts_flow_session counted;
    counted.h = const_cast<astts_flow*>(h);
    carve_session(cv, counted, t, n_slots, rows_max, steps_max);
    return cv.o;
}

int astts_flow_session_create(astts_flow_t* h, int32_t t, int32_t n_slots, int32_t rows_max, int32_t steps_max, void* workspace,
                              size_t workspace_bytes, astts_stream_t stream, astts_flow_session_t** out) {
    ASTTS_REQUIRE(h && workspace && out, ASTTS_ERR_INVALID, "astts_flow_session_create: null argument");
    astts::FlowSessionPlan p;
    ASTTS_REQUIRE(p.init(t, n_slots, rows_max, steps_max) == astts::FLOW_SESSION_OK && steps_max <= FLOW_MAX_STEPS, ASTTS_ERR_INVALID,
                  "astts_flow_session_create: t=%d n_slots=%d rows_max=%d steps_max=%d", t, n_slots, rows_max, steps_max);
    ASTTS_REQUIRE(workspace_bytes >= astts_flow_session_bytes(h, t, n_slots, rows_max, steps_max) && ((uintptr_t)workspace & 255) == 0,
                  ASTTS_ERR_WORKSPACE, "astts_flow_session_create: workspace too small or misaligned");
    astts_flow_session* s = new astts_flow_session();
    s->h = h;
    s->plan = p;
    s->st = stream;
    s->passes = s->carried = 0;
    Carver cv{(char*)workspace, 0};
    carve_session(cv, *s, t, n_slots, rows_max, steps_max);
    *out = s;
    return ASTTS_OK;
}

int astts_flow_session_destroy(astts_flow_session_t* s) {
    delete s;
    return ASTTS_OK;
}

int astts_flow_session_can_admit(const astts_flow_session_t* s, int32_t b, int32_t t, int32_t n_steps) {
    return s ? s->plan.admissible(b, t, n_steps) : astts::FLOW_SESSION_ERR_ARG;
}

int astts_flow_session_admit(astts_flow_session_t* s, float* x, const float* mu, const float* spk, const float* cond, const int32_t* lens,
                             int32_t b, int32_t t, int32_t n_steps, const float* t_host, const float* dt_host, float cfg_rate,
                             int32_t* slot_out) {
    ASTTS_REQUIRE(s && x && mu && spk && cond && t_host && dt_host && slot_out, ASTTS_ERR_INVALID, "astts_flow_session_admit: null argument");
    const int slot = s->plan.admissible(b, t, n_steps);
    ASTTS_REQUIRE(slot >= 0, ASTTS_ERR_INVALID, "astts_flow_session_admit: b=%d t=%d n_steps=%d is not admissible now (%d)", b, t, n_steps, slot);
    astts_flow_session::Slot& X = s->slot[slot];
    X.seg = Seg{x, mu, spk, cond, 0, b, 0.0f, cfg_rate};
    X.full = lens == nullptr;
    for (int i = 0; i < n_steps; ++i) X.dt[i] = dt_host[i];
    hipLaunchKernelGGL(flow_fill_lens, dim3((2 * b + 63) / 64), dim3(64), 0, (hipStream_t)s->st, lens, X.lens_full, X.lens_half, b, t);
    ASTTS_CHECK_LAUNCH();
    RUN(time_path(Ctx(s->h, s->B, t, X.full, s->st, &X.seg, 1, false), X.T, t_host, n_steps));
    s->plan.admit(b, t, n_steps);
    *slot_out = slot;
    return ASTTS_OK;
}

int astts_flow_session_step(astts_flow_session_t* s, int32_t n_passes, uint32_t* finished_mask_out) {
    ASTTS_REQUIRE(s && finished_mask_out && n_passes >= 1, ASTTS_ERR_INVALID, "astts_flow_session_step: bad argument");
    using astts::FlowSessionPlan;
    const int C = s->h->cfg.channels;
    const int n_res = (int)(s->h->down.size() + s->h->mid.size() + s->h->up.size());
    uint32_t done = 0;
    *finished_mask_out = 0;
    // ASTTS_FLOW_SHARE=0: every batch of a joined pass gets its own feed-forward and GEMM launches (tests, A/B).  Read per call: the tests
    // switch inside one process.
    const char* se = getenv("ASTTS_FLOW_SHARE");
    const bool share = !(se && atoi(se) == 0);
    for (int p = 0; p < n_passes && s->plan.n_active() > 0; ++p) {
        const int nseq = s->plan.layout();
        Seg segs[FlowSessionPlan::kSlots];
        FlowJoinTable J{};
        bool full = true;
        for (int i = 0; i < s->plan.n_slots; ++i) {
            const astts::FlowSlot& ps = s->plan.s[i];
            const astts_flow_session::Slot& X = s->slot[i];
            if (!ps.active) continue;
            const int n = J.n++;
            segs[n] = X.seg;
            segs[n].seq0 = ps.seq0;
            segs[n].dt = X.dt[ps.step];
            full = full && X.full;
            J.tproj[n] = X.T.tproj;
            J.lens_full[n] = X.lens_full;
            J.lens_half[n] = X.lens_half;
            J.seq0[n] = ps.seq0;
            J.b2[n] = 2 * ps.b;
            J.trows[n] = ps.n_steps * 2 * ps.b;
            J.step[n] = ps.step;
        }
        const Ctx k(s->h, s->B, s->plan.t, full, s->st, segs, J.n, share);
        if (J.n == 1) {     // a lone batch: the launches of astts_flow_solve, on the batch's own tables
            RUN(estimator_pass(k, J.tproj[0] + (size_t)J.step[0] * nseq * C, (size_t)J.trows[0] * C, J.lens_full[0], J.lens_half[0]));
        } else {
            hipLaunchKernelGGL(flow_join_assemble, dim3(grid_for((int64_t)n_res * nseq * C)), dim3(256), 0, (hipStream_t)s->st, J, s->B.T.tproj,
                               s->B.lens_full, s->B.lens_half, nseq, n_res, C);
            ASTTS_CHECK_LAUNCH();
            RUN(estimator_pass(k, s->B.T.tproj, (size_t)nseq * C, s->B.lens_full, s->B.lens_half));
        }
        s->passes += 1;
        s->carried += J.n;
        done |= s->plan.advance();
    }
    *finished_mask_out = done;
    return ASTTS_OK;
}

int astts_flow_session_state(const astts_flow_session_t* s, int32_t* out8) {
    ASTTS_REQUIRE(s && out8, ASTTS_ERR_INVALID, "astts_flow_session_state: null argument");
    int mask = 0;
    for (int i = 0; i < astts::FlowSessionPlan::kSlots; ++i) {
        const astts::FlowSlot& ps = s->plan.s[i];
        mask |= ps.active << i;
        out8[4 + i] = ps.active ? ps.n_steps - ps.step : 0;
    }
    out8[0] = mask;
    out8[1] = s->plan.rows_active();
    out8[2] = s->passes;
    out8[3] = s->carried;
    return ASTTS_OK;
}

}  // extern "C"
