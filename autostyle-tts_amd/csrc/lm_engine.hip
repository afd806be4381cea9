// lm_engine.hip -- autoregressive decode loop of the acoustic transformer, host side in C++.
//
// The reference's hot loop #2: one speech token per step, ~50 steps per audio second, inside cosyvoice's
// TransformerLM.inference (behind tts_with_rag.py:195).  A Python host pays ~10 us per operator call; this engine issues a decode from
// C++ with no host synchronisation: sampling, repetition check, EOS masking and the token history all stay on the GPU.
//
// ONE step loop (run_steps: logits copy, sampler, last-step break, the logits carried from one range of steps to the next) drives one
// of THREE step bodies, each nothing but the launches that turn the sampled token into the next logits:
//   step_v2    <= 32 rows, the decode-step kernels of lm_step.hip (5 launches per layer): the product path
//   step_v1    <= 32 rows, the operator chain astts_op_gemm_fused / astts_op_attn_relpos (5 per layer): the second implementation the
//              tests compare with, and the path of fp32 caches / position tables (ASTTS_LM_ENGINE=v1 forces it)
//   step_wide  33 .. ASTTS_LM_MAX_ROWS rows, plain GEMMs over all rows (7 per layer)
// The workspace has two layouts, each written ONCE as a carve function that counts the bytes (astts_lm_workspace_bytes) and hands out
// the pointers (astts_lm_decode): carve_narrow, shared by v1 and v2, and carve_wide.
// A decode SESSION (astts_lm_session_*, include/session/astts_lm_session.h) is the same loop and step_v2 over a WINDOW of rows of a
// cache arena that up to two batches share: a batch admitted while another is decoding joins its chain (bookkeeping: lm_session.h).
#include "common.h"
#include "lm_session.h"
#include "../../include/session/astts_lm_session.h"
#include "lm_step.h"

#include <cstdlib>
#include <cstring>
#include <vector>

struct astts_lm {
    astts_lm_config_t cfg;
    std::vector<astts_lm_layer_t> layers;
    astts_lm_globals_t g;
};

using namespace astts;

#define RUN(expr)                          \
    do {                                   \
        const int rc_ = (expr);            \
        if (rc_ != ASTTS_OK) return rc_;   \
    } while (0)

namespace {

// the rows of one decode inside a call: what the sampler and the logits copy need.  astts_lm_decode has one group, all rows of the call;
// a session step (astts_lm_session_step) has one or two, each at its own step index
struct RowGroup {
    int32_t row0, b;             // rows [row0, row0 + b) of the call
    int32_t n_steps, s_off;      // steps of its decode; its step index is the loop's s + s_off
    const float* uniforms;
    const int32_t* forced_tokens;
    int32_t eos_min_steps;
    const int32_t* eos_min_rows;
    int32_t* tokens_out;
    float* logits_out;
};

// what astts_lm_decode received (include/astts.h), after validation -- or one range of steps of a session
struct DecodeCall {
    const float* logits0;
    void* const* kv_cache;
    const int32_t* key_start;
    int32_t t_max, b, pos0, s_begin, s_end;
    int32_t kv_rows;             // rows of the time-major cache the pointers lead into (== b unless the call is a row window of a session's arena)
    RowGroup g[2];
    int32_t n_groups;
    hipStream_t st;
};

// hands out 256-byte aligned pieces of a workspace; with base == nullptr it only counts them
struct Carver {
    char* base;
    size_t o = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + o) : nullptr;
        o = align_up(o + sizeof(T) * count, 256);
        return p;
    }
};

// ---- workspace of <= 32 rows: ONE layout.  The members carry v1's names; v2 uses the same slots through the view V2.
struct NarrowWs {
    float *h0, *h1, *q, *ao;   // four float[b*d] slots.  v1: residual stream ping / pong (h1 first holds the embedding projection), q, attention output
    float* ff;                 // float[b*ffn]: fp32 FFN hidden
    float* lg;                 // float[b*vocab_out]: the logits the next step samples from -- what one range of steps hands to the next
    int32_t* tok;              // int32[b]: the sampled tokens (a second int32[b] slot behind it is reserved)
    void* skw;                 // astts_op_gemm_fused_workspace_bytes(): split-K counters + partial sums
    size_t skw_bytes;
    // v2: embedding projection (before its LayerNorm), residual stream ping / pong, q; fp16 FFN hidden (half of the fp32 slot); the
    // attention's split-key partials live in the split-K area: [b][heads][2][64] + [b][heads][2][2] floats must fit it
    struct V2 { float *h1, *xa, *xb, *q; _Float16* ff; float *part_o, *part_ml, *lg; int32_t* tok; };
    V2 v2(int b, int heads) const { return {h0, h1, q, ao, (_Float16*)ff, (float*)skw, (float*)skw + (size_t)b * heads * 2 * 64, lg, tok}; }
    static size_t v2_partial_bytes(int b, int heads) { return (size_t)b * heads * (2 * 64 + 2 * 2) * sizeof(float); }
};

// one carve-up serves astts_lm_workspace_bytes (base == nullptr) and astts_lm_decode
size_t carve_narrow(const astts_lm* h, int b, char* base, NarrowWs* W) {
    const size_t rows = b;
    Carver c{base};
    NarrowWs tmp;
    NarrowWs& X = W ? *W : tmp;
    for (float** slot : {&X.h0, &X.h1, &X.q, &X.ao}) *slot = c.take<float>(rows * h->cfg.d);
    X.ff = c.take<float>(rows * h->cfg.ffn);
    X.lg = c.take<float>(rows * h->cfg.vocab_out);
    X.tok = c.take<int32_t>(rows);
    (void)c.take<int32_t>(rows);      // reserved
    X.skw_bytes = astts_op_gemm_fused_workspace_bytes();
    X.skw = c.take<char>(X.skw_bytes);
    return c.o;
}

// ---- workspace of 33 .. ASTTS_LM_MAX_ROWS rows
struct WideWs {
    float *h1, *xa, *xb;      // embedding rows; residual stream ping / pong
    _Float16* n16;            // LayerNorm output
    float *q, *ao;            // q; attention output
    _Float16* ff;             // FFN hidden
    float* lg;                // logits (the hand-over between ranges, as NarrowWs::lg)
    int32_t* tok;
};

size_t carve_wide(const astts_lm* h, int b, char* base, WideWs* W) {
    const size_t rows = b, d = h->cfg.d;
    Carver c{base};
    WideWs tmp;
    WideWs& X = W ? *W : tmp;
    X.h1 = c.take<float>(rows * d);
    X.xa = c.take<float>(rows * d);
    X.xb = c.take<float>(rows * d);
    X.n16 = c.take<_Float16>(rows * d);
    X.q = c.take<float>(rows * d);
    X.ao = c.take<float>(rows * d);
    X.ff = c.take<_Float16>(rows * h->cfg.ffn);
    X.lg = c.take<float>(rows * h->cfg.vocab_out);
    X.tok = c.take<int32_t>(rows);
    return c.o;
}

// ---- the step loop of every engine.  Steps [s_begin, s_end) of an n_steps decode: a range that does not start at 0 samples from the
// logits the previous range left in the workspace (`lg`: the caller passes the SAME workspace, token buffer and cache to every range of
// one decode).  advance(pos) issues the forward pass of the tokens in `tok` at position pos and leaves the next logits in `lg`; the last
// step of a decode only samples.  (A template parameter, not a function pointer: the step is launch-rate bound.)
// With two groups (a session) the sampler serves both in ONE launch, and advance() runs while any group has a step left: it is the
// session's advance that narrows the rows to the groups that go on (astts_lm_session_step).
template <class Advance>
int run_steps(const astts_lm_config_t& c, const DecodeCall& k, float* lg, int32_t* tok, Advance advance) {
    const float* cur = k.s_begin == 0 ? k.logits0 : lg;
    for (int s = k.s_begin; s < k.s_end; ++s) {
        SampleGroup sg[2];
        bool last = true;
        for (int i = 0; i < k.n_groups; ++i) {
            const RowGroup& r = k.g[i];
            const int sr = s + r.s_off;
            if (r.logits_out)
                ASTTS_CHECK_HIP(hipMemcpy2DAsync(r.logits_out + (size_t)sr * c.vocab_out, sizeof(float) * (size_t)r.n_steps * c.vocab_out,
                                                 cur + (size_t)r.row0 * c.vocab_out, sizeof(float) * c.vocab_out, sizeof(float) * c.vocab_out,
                                                 r.b, hipMemcpyDeviceToDevice, k.st));
            sg[i] = SampleGroup{r.tokens_out, r.uniforms + (size_t)sr * r.b * 2, r.forced_tokens, r.eos_min_rows, r.b, r.row0, sr, r.n_steps,
                                sr < r.eos_min_steps ? 1 : 0};
            last = last && sr + 1 == r.n_steps;
        }
        RUN(ras_sample_groups_launch(cur, tok, c.vocab_out, c.top_k, c.top_p, c.ras_win, c.ras_tau, c.speech_vocab, c.eos_policy, sg, k.n_groups, k.st));
        if (last) break;
        RUN(advance(k.pos0 + s));
        cur = lg;
    }
    return ASTTS_OK;
}

// ---- v2: the step kernels of lm_step.hip (2 launches fewer per step than v1, one memory round trip per kernel, 8-column workgroups,
// key-split attention merged by its consumer).  A row's arithmetic does not depend on the number of rows (lm_step.hip, FORM 2), so 8-,
// 16- and 32-row chains agree bit for bit.  With the sampler, one decode step = 1 + 14 x (QKV, attention, out-proj, FFN-in, FFN-out)
// + head = 72 launches (73 without the projected embedding table).
int step_v2(const astts_lm* h, const DecodeCall& k, const NarrowWs::V2& w, int pos) {
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    const int d = c.d, b = k.b;
    hipStream_t st = k.st;
    const float scale = 0.125f;
    // ASTTS_LM_KSPLIT=1 (experiments): the decode attention as 128 workgroups with the whole key range each instead of 256 with half of it
    static const int ksplit = exp_env_int("ASTTS_LM_KSPLIT", 2) == 1 ? 1 : 2;
    // ASTTS_LM_SKIP=<bits> (timing experiments only, results are GARBAGE): drops a launch of every layer -- 1 out-projection, 2 FFN-out,
    // 4 QKV, 8 attention, 16 FFN-in.  Compiled in only with -DASTTS_EXPERIMENTS (make EXTRA=-DASTTS_EXPERIMENTS): the product library
    // cannot be talked into wrong tokens by an environment variable.
#ifdef ASTTS_EXPERIMENTS
    static const int skip = exp_env_int("ASTTS_LM_SKIP", 0);
#else
    constexpr int skip = 0;
#endif
    // ASTTS_LM_FFN_SPLIT=0: FFN-out as one workgroup per column block over the whole K (rounds 2-3)
    static const bool ffn_split_env = exp_env_int("ASTTS_LM_FFN_SPLIT", 1) != 0;
    const bool ffn_split = ffn_split_env && (c.ffn & 255) == 0;
    const KvLayout lay = KvLayout::time_major(k.kv_rows, d);
    auto gemv = [&]() {
        GemvArgs a;
        memset(&a, 0, sizeof(a));
        a.m = b;
        a.ln_eps = c.eps;
        return a;
    };
    auto with_ln = [&](GemvArgs& a, const float* gam, const float* bet) {
        if (c.ln_folded) a.ln_plain = 1;
        else { a.ln_g = gam; a.ln_b = bet; }
    };
    // embed projection: speech_embedding[tok] -> Linear.  Its LayerNorm -> ReLU -> * sqrt(d) runs inside layer 0's QKV
    // kernel (pre-transform of the staged rows; workgroup 0 writes the result to xa, the residual stream).
    // With the projected table (globals.embed_table = speech_emb W^T + b, formed at load) the projection is a gather as well.
    GemvArgs a = gemv();
    if (!g.embed_table) {
        a.x = g.speech_emb; a.gather = w.tok; a.ldx = d; a.w = (const _Float16*)g.embed_w; a.bias = g.embed_b; a.out = w.h1; a.ldo = d;
        a.n = d; a.k = d; a.kpad = d;
        RUN(lm_gemv_launch(a, st));
    }
    // the residual stream alternates between two buffers: layer l reads X[l % 2] and its FFN-out projection leaves X[(l + 1) % 2].
    // FFN-out runs as two K slices per column block (lm_step.h, GemvArgs::ksplit: 256 workgroups with 32 KB of weights each instead
    // of 128 with 64 KB) that meet in the output with one fp32 atomic each, so the output must hold zeros: the FFN-in launch of the
    // layer clears it (its last readers, QKV and the out-projection of the layer, are done by then).
    float* X[2] = {w.xa, w.h1};          // (h1 is free once layer 0's QKV has read it)
    float* y = w.xb;
    for (int l = 0; l < c.layers; ++l) {
        const astts_lm_layer_t& L = h->layers[l];
        _Float16* kvc = (_Float16*)k.kv_cache[l];
        float* x = X[l & 1];
        float* xn = X[(l + 1) & 1];
        a = gemv();             // LN1 + QKV: q -> `q`, K|V -> cache row `pos`
        if (l == 0) {
            a.x = g.embed_table ? g.embed_table : w.h1;
            a.gather = g.embed_table ? w.tok : nullptr;
            a.pre_g = g.embed_ln_g; a.pre_b = g.embed_ln_b; a.pre_scale = sqrtf((float)d); a.pre_out = x;
        } else {
            a.x = x;
        }
        a.ldx = d; with_ln(a, L.n1_g, L.n1_b);
        a.w = (const _Float16*)L.wqkv; a.bias = L.bqkv; a.out = w.q; a.ldo = d; a.kv = kvc; a.n_split = d; a.kv_t = lay.t; a.kv_b = lay.b; a.kv_h = lay.h; a.kv_v = lay.v; a.pos = pos;
        a.n = 3 * d; a.k = d; a.kpad = d;
        if (!(skip & 4)) RUN(lm_gemv_launch(a, st));
        AttnArgs t;
        memset(&t, 0, sizeof(t));
        t.q = w.q; t.kv = kvc; t.postab = (const _Float16*)L.pos; t.bias_u = L.bias_u; t.bias_v = L.bias_v; t.kstart = k.key_start;
        t.part_o = w.part_o; t.part_ml = w.part_ml; t.ksplit = ksplit; t.b = b;
        t.h = c.heads; t.ldq = d; t.ldp = c.pos_ld; t.center = c.pos_center;
        if (ksplit == 1) { t.out = w.ff; t.ldo = d; }      // one workgroup per (row, head): the fp16 FFN buffer is free until FFN-in
        t.d = d; t.scale = scale; t.pos = pos; t.kv_t = lay.t; t.kv_b = lay.b; t.kv_h = lay.h; t.kv_v = lay.v;
        if (!(skip & 8)) RUN(lm_attn_launch(t, st));
        a = gemv();             // out-proj on the merged attention partials + residual
        a.x = w.part_o; a.x2 = w.part_ml; a.x_mode = 2;
        if (ksplit == 1) { a.x = w.ff; a.x2 = nullptr; a.x_mode = 1; a.ldx = d; }
        a.w = (const _Float16*)L.wo; a.bias = L.bo; a.res = x; a.ldr = d; a.out = y; a.ldo = d;
        a.n = d; a.k = d; a.kpad = d;
        if (!(skip & 1)) RUN(lm_gemv_launch(a, st));
        a = gemv();             // LN2 + FFN-in + ReLU -> fp16 hidden (its only consumer is an MFMA operand)
        a.x = y; a.ldx = d; with_ln(a, L.n2_g, L.n2_b);
        a.w = (const _Float16*)L.w1; a.bias = L.b1; a.out16 = w.ff; a.ldo16 = c.ffn; a.relu = 1; a.n = c.ffn; a.k = d; a.kpad = d;
        if (ffn_split) { a.zero = xn; a.zero_n = b * d; }
        if (!(skip & 16)) RUN(lm_gemv_launch(a, st));
        a = gemv();             // FFN-out + residual
        a.x = w.ff; a.x_mode = 1; a.ldx = c.ffn; a.w = (const _Float16*)L.w2; a.bias = L.b2; a.res = y; a.ldr = d; a.out = xn; a.ldo = d;
        a.n = d; a.k = c.ffn; a.kpad = c.ffn;
        if (ffn_split) a.ksplit = 2;
        if (!(skip & 2)) RUN(lm_gemv_launch(a, st));
    }
    a = gemv();                 // after_norm + output head
    a.x = X[c.layers & 1]; a.ldx = d; with_ln(a, g.after_g, g.after_b);
    a.w = (const _Float16*)g.head_w; a.bias = g.head_b; a.out = w.lg; a.ldo = c.vocab_out; a.n = c.vocab_out; a.k = d; a.kpad = d;
    return lm_gemv_launch(a, st);
}

// ---- v1: the operator chain (round 1): sampler + embedding projection + its LayerNorm + 14 x 5 + head = 74 launches per step.
// (A "v3" -- two fused launches per layer with a fixed-point residual stream -- was built in round 4, parity-green and 2.4x slower:
// EXPERIMENTS.md F holds the log; the code is gone.)
int step_v1(const astts_lm* h, const DecodeCall& k, const NarrowWs& w, int pos) {
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    const int d = c.d, b = k.b;
    hipStream_t st = k.st;
    const int dpad = (int)align_up((size_t)d, 64), fpad = (int)align_up((size_t)c.ffn, 64);
    const float scale = 0.125f;  // 1/sqrt(64)
    const int64_t kv_row = (int64_t)b * 2 * d;  // one time step of the time-major cache
    const size_t esz = c.kv_f16 ? 2 : 4;
    // embed: speech_embedding[tok] -> Linear -> LayerNorm -> ReLU * sqrt(d)
    RUN(astts_op_gemm_fused(g.speech_emb, w.tok, nullptr, nullptr, 0.f, g.embed_w, g.embed_b, nullptr, w.h1, nullptr, 0, b, d, 0, d, dpad, d, d,
                            0, 0, ASTTS_ACT_NONE, 1.f, 0.f, w.skw, w.skw_bytes, st));
    RUN(astts_op_layernorm(w.h1, g.embed_ln_g, g.embed_ln_b, w.h0, 0, b, d, d, d, c.eps, sqrtf((float)d), st));
    float* x = w.h0;
    float* y = w.h1;
    for (int l = 0; l < c.layers; ++l) {
        const astts_lm_layer_t& L = h->layers[l];
        char* kvc = (char*)k.kv_cache[l];
        // LN1 + QKV; K|V land in cache row `pos`
        RUN(astts_op_gemm_fused(x, nullptr, L.n1_g, L.n1_b, c.eps, L.wqkv, L.bqkv, nullptr, w.q, kvc + (size_t)pos * kv_row * esz, c.kv_f16, b,
                                3 * d, d, d, dpad, d, d, 2 * d, 0, ASTTS_ACT_NONE, 1.f, 0.f, w.skw, w.skw_bytes, st));
        RUN(astts_op_attn_relpos(w.q, kvc, kvc + (size_t)d * esz, c.kv_f16, L.pos, c.pos_f16, L.bias_u, L.bias_v,
                                 /*lens: every row has pos + 1 keys*/ nullptr, k.key_start, w.ao, b, c.heads, 1, pos + 1, /*ldq*/ b * d,
                                 /*ldk*/ (int32_t)kv_row, /*ldo*/ b * d, c.pos_ld, /*q_bs*/ d, /*k_bs*/ 2 * d, /*o_bs*/ d, pos, c.pos_center, 1,
                                 scale, st));
        RUN(astts_op_gemm_fused(w.ao, nullptr, nullptr, nullptr, 0.f, L.wo, L.bo, x, y, nullptr, 0, b, d, 0, d, dpad, d, d, 0, d,
                                ASTTS_ACT_NONE, 1.f, 0.f, w.skw, w.skw_bytes, st));
        RUN(astts_op_gemm_fused(y, nullptr, L.n2_g, L.n2_b, c.eps, L.w1, L.b1, nullptr, w.ff, nullptr, 0, b, c.ffn, 0, d, dpad, d, c.ffn, 0, 0,
                                ASTTS_ACT_RELU, 1.f, 0.f, w.skw, w.skw_bytes, st));
        RUN(astts_op_gemm_fused(w.ff, nullptr, nullptr, nullptr, 0.f, L.w2, L.b2, y, x, nullptr, 0, b, d, 0, c.ffn, fpad, c.ffn, d, 0, d,
                                ASTTS_ACT_NONE, 1.f, 0.f, w.skw, w.skw_bytes, st));
    }
    // after_norm + output head
    return astts_op_gemm_fused(x, nullptr, g.after_g, g.after_b, c.eps, g.head_w, g.head_b, nullptr, w.lg, nullptr, 0, b, c.vocab_out, 0, d, dpad,
                               d, c.vocab_out, 0, 0, ASTTS_ACT_NONE, 1.f, 0.f, w.skw, w.skw_bytes, st);
}

// ---- wide: one decode step over 33 .. 256 rows with PLAIN GEMMs (round 5).  The step kernels of lm_step.hip stage every input row of the
// batch in each workgroup: right for <= 32 rows (a launch is a chain of latencies), wrong beyond -- a 256-row batch as eight 32-row chains
// streams the 352 MB of weights eight times per token and pays 8 x 72 launches.  Here a layer is LayerNorm -> q GEMM, K|V GEMM (straight
// into the cache row) -> per-row decode attention -> out-projection (+ residual) -> LayerNorm -> FFN-in (+ ReLU, fp16) -> FFN-out (+ residual),
// the GEMMs on the LDS-DMA ring kernel wherever the activations are fp16 (LayerNorm output, FFN hidden): the weights are read ONCE per token
// for all rows.  Measured alone at 256 rows x ~190 keys (scripts/bigbatch_probe.py): 3.9 ms per step as eight 32-row chains on two
// streams, 2.5 ms on the operator path from Python (host-bound, fp32-activation tile GEMMs).  The KV reads (B x heads x keys x 256 bytes
// per layer) are the same either way and take over at long contexts.  Arithmetic: the same fp16 products with fp32 accumulation; only the
// summation order differs from the <= 32-row engines (tests hold the logits to the oracle, not to them).
// One step = sampler + embedding gather + its LayerNorm + 14 x 7 + (LayerNorm, head) = 103 launches; 117 with ASTTS_LM_WIDE_GEMM=tile.
int step_wide(const astts_lm* h, const DecodeCall& k, const WideWs& w, int pos) {
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    const int d = c.d, b = k.b;
    astts_stream_t stream = k.st;
    const float scale = 0.125f;
    const int64_t kv_row = (int64_t)b * 2 * d;      // one time step of the time-major cache
    // astts_op_gemm_rows: a latency-sized kernel for these shapes; the K | V columns of the q | k | v projection go straight into the
    // cache (seven launches per layer: two LayerNorms, q | k | v, attention, out-projection, FFN-in, FFN-out).  ASTTS_LM_WIDE_GEMM=tile
    // goes back to the tile / ring family (eight per layer).
    static const bool rows_kernel = !(getenv("ASTTS_LM_WIDE_GEMM") && !strcmp(getenv("ASTTS_LM_WIDE_GEMM"), "tile"));
    auto gemm = [&](const void* x, int x16, int kk, const void* wt, const float* bias, const float* res, void* out, int out16, int n, int ldc, int act) {
        if (rows_kernel)
            return astts_op_gemm_rows(x, x16, wt, bias, res, out, out16, nullptr, 0, b, n, 0, kk, kk, ldc, 0, res ? d : 0, act, stream);
        return astts_op_gemm(x, x16, wt, bias, res, nullptr, out, out16, b, n, kk, kk, 1, kk, ldc, res ? d : 0, b, b, 1, 1, 0, act, 1.0f, 0.1f, nullptr, stream);
    };
    // LayerNorm(x) -> fp16 -> projection (optionally with a second destination for the columns >= n_split)
    auto gemm_ln = [&](const float* x, const float* ga, const float* be, const void* wt, const float* bias, void* out, int out16, int n, int ldc,
                       int act, void* out2, int n_split, int ldc2) {
        RUN(astts_op_layernorm(x, ga, be, w.n16, 1, b, d, d, d, c.eps, 0.0f, stream));
        if (rows_kernel)
            return astts_op_gemm_rows(w.n16, 1, wt, bias, nullptr, out, out16, out2, 1, b, n, n_split, d, d, ldc, ldc2, 0, act, stream);
        if (!out2) return gemm(w.n16, 1, d, wt, bias, nullptr, out, out16, n, ldc, act);
        RUN(gemm(w.n16, 1, d, wt, bias, nullptr, out, out16, n_split, ldc, act));
        return gemm(w.n16, 1, d, (const _Float16*)wt + (size_t)n_split * d, bias + n_split, nullptr, out2, 1, n - n_split, ldc2, act);
    };
    // the token's projected embedding (a row of the load-time table) -> LayerNorm -> ReLU -> * sqrt(d)
    RUN(astts_op_embedding(g.embed_table, w.tok, w.h1, b, d, d, c.speech_vocab, 1.0f, stream));
    RUN(astts_op_layernorm(w.h1, g.embed_ln_g, g.embed_ln_b, w.xa, 0, b, d, d, d, c.eps, sqrtf((float)d), stream));
    float* x = w.xa;
    float* y = w.xb;
    for (int l = 0; l < c.layers; ++l) {
        const astts_lm_layer_t& L = h->layers[l];
        char* kvc = (char*)k.kv_cache[l];
        RUN(gemm_ln(x, L.n1_g, L.n1_b, L.wqkv, L.bqkv, w.q, 0, 3 * d, d, ASTTS_ACT_NONE, kvc + (size_t)pos * kv_row * 2, d, 2 * d));
        RUN(astts_op_attn_relpos(w.q, kvc, kvc + (size_t)d * 2, 1, L.pos, 1, L.bias_u, L.bias_v, nullptr, k.key_start, w.ao, b, c.heads, 1, pos + 1,
                                 b * d, (int32_t)kv_row, b * d, c.pos_ld, d, 2 * d, d, pos, c.pos_center, 1, scale, stream));
        RUN(gemm(w.ao, 0, d, L.wo, L.bo, x, y, 0, d, d, ASTTS_ACT_NONE));
        RUN(gemm_ln(y, L.n2_g, L.n2_b, L.w1, L.b1, w.ff, 1, c.ffn, c.ffn, ASTTS_ACT_RELU, nullptr, 0, 0));
        RUN(gemm(w.ff, 1, c.ffn, L.w2, L.b2, y, x, 0, d, d, ASTTS_ACT_NONE));
    }
    return gemm_ln(x, g.after_g, g.after_b, g.head_w, g.head_b, w.lg, 0, c.vocab_out, c.vocab_out, ASTTS_ACT_NONE, nullptr, 0, 0);
}


// ---- decode session (include/session/astts_lm_session.h): ONE chain that up to two batches share.  The bookkeeping -- rows, arena
// positions, how many steps fit one range, when to rebase -- is lm_session.h (no HIP); here are the two copy kernels and the calls.
constexpr int kSessionMaxLayers = 32;
struct KvPtrs { _Float16* p[kSessionMaxLayers]; };

// Admission: the valid prefix keys [key_start[r], pos0) of every layer move from the prefill's cache [t][rows][2d] to the arena
// [t + shift][arena rows][2d] (dst leads to the group's first row), 16 bytes per thread and iteration; block (0, 0) writes the rows'
// shifted key_start.  grid (pos0, layers).
__global__ __launch_bounds__(256) void lm_kv_admit(KvPtrs src, KvPtrs dst, const int* kstart_src, int* kstart_dst, int rows, int shift,
                                                   int64_t src_t, int64_t dst_t, int row_vec) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const uint4* sp = reinterpret_cast<const uint4*>(src.p[blockIdx.y] + (int64_t)t * src_t);
    uint4* dp = reinterpret_cast<uint4*>(dst.p[blockIdx.y] + (int64_t)(t + shift) * dst_t);
    for (int i = tid; i < rows * row_vec; i += 256) {
        const int r = i / row_vec;
        if (kstart_src && t < kstart_src[r]) continue;
        dp[i] = sp[i];
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < rows) kstart_dst[tid] = (kstart_src ? kstart_src[tid] : 0) + shift;
}

// Rebase: arena positions [src0, src0 + gridDim.x) of rows [0, rows) (kv leads to the first of them) move down by delta -- source and
// destination do not overlap (SessionPlan::rebase) -- and the rows' key_start (kstart leads to the first of them) drops by the same
// amount.  grid (n, layers).
__global__ __launch_bounds__(256) void lm_kv_rebase(KvPtrs kv, int* kstart, int rows, int src0, int delta, int64_t t_stride, int row_vec) {
    const int t = src0 + blockIdx.x, tid = threadIdx.x;
    const uint4* sp = reinterpret_cast<const uint4*>(kv.p[blockIdx.y] + (int64_t)t * t_stride);
    uint4* dp = reinterpret_cast<uint4*>(kv.p[blockIdx.y] + (int64_t)(t - delta) * t_stride);
    for (int i = tid; i < rows * row_vec; i += 256) dp[i] = sp[i];
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < rows) kstart[tid] -= delta;
}

}  // namespace

struct astts_lm_session {
    astts_lm* h;
    hipStream_t st;
    SessionPlan plan;
    char* mem;                 // one allocation: arenas, workspace, key_start
    KvPtrs arena;              // [t_arena][rows_max][2d] fp16 per layer
    NarrowWs ws;               // for rows_max rows
    int32_t* kstart;           // [rows_max] first valid key of every row, in arena positions
    RowGroup rows[SessionPlan::kGroups];   // what each admitted group's sampler needs (row0 / s_off are set per range)
    int64_t rebases;
};

extern "C" {

int astts_lm_create(const astts_lm_config_t* cfg, const astts_lm_globals_t* globals, const astts_lm_layer_t* layers,
                    astts_lm_t** out) {
    ASTTS_REQUIRE(cfg && globals && layers && out, ASTTS_ERR_INVALID, "astts_lm_create: null argument");
    ASTTS_REQUIRE(cfg->d >= 64 && cfg->d % 64 == 0 && cfg->heads * 64 == cfg->d, ASTTS_ERR_INVALID,
                  "astts_lm_create: d=%d heads=%d (head dim must be 64)", cfg->d, cfg->heads);
    ASTTS_REQUIRE(cfg->layers >= 1 && cfg->ffn >= 64 && cfg->vocab_out >= 2 && cfg->speech_vocab >= 1, ASTTS_ERR_INVALID,
                  "astts_lm_create: bad sizes");
    astts_lm* h = new astts_lm();
    h->cfg = *cfg;
    h->g = *globals;
    h->layers.assign(layers, layers + cfg->layers);
    *out = h;
    return ASTTS_OK;
}

int astts_lm_destroy(astts_lm_t* h) {
    delete h;
    return ASTTS_OK;
}

size_t astts_lm_workspace_bytes(const astts_lm_t* h, int32_t b) {
    if (!h || b < 1 || b > ASTTS_LM_MAX_ROWS) return 0;
    return b > 32 ? carve_wide(h, b, nullptr, nullptr) : carve_narrow(h, b, nullptr, nullptr);
}

// Arguments: include/astts.h.  Validate, choose the engine, carve the workspace, run the steps [s_begin, s_end).
int astts_lm_decode(astts_lm_t* h, const float* logits0, void* const* kv_cache, const int32_t* key_start, int32_t t_max,
                    int32_t b, int32_t pos0, int32_t n_steps, int32_t s_begin, int32_t s_end, const float* uniforms,
                    const int32_t* forced_tokens, int32_t eos_min_steps, const int32_t* eos_min_rows, int32_t* tokens_out,
                    float* logits_out, void* workspace, size_t workspace_bytes, astts_stream_t stream) {
    ASTTS_REQUIRE(h && logits0 && kv_cache && uniforms && tokens_out && workspace, ASTTS_ERR_INVALID,
                  "astts_lm_decode: null argument");
    ASTTS_REQUIRE(s_begin >= 0 && s_begin < s_end && s_end <= n_steps, ASTTS_ERR_INVALID, "astts_lm_decode: steps [%d, %d) of %d", s_begin,
                  s_end, n_steps);
    ASTTS_REQUIRE(b >= 1 && b <= ASTTS_LM_MAX_ROWS, ASTTS_ERR_INVALID, "astts_lm_decode: b=%d (1..%d per call)", b, ASTTS_LM_MAX_ROWS);
    ASTTS_REQUIRE(n_steps >= 1 && pos0 >= 1 && pos0 + n_steps - 1 <= t_max, ASTTS_ERR_INVALID,
                  "astts_lm_decode: pos0=%d n_steps=%d t_max=%d", pos0, n_steps, t_max);
    ASTTS_REQUIRE(workspace_bytes >= astts_lm_workspace_bytes(h, b) && ((uintptr_t)workspace & 255) == 0,
                  ASTTS_ERR_WORKSPACE, "astts_lm_decode: workspace too small or misaligned");
    const DecodeCall k = {logits0, kv_cache, key_start, t_max, b, pos0, s_begin, s_end, b,
                          {{0, b, n_steps, 0, uniforms, forced_tokens, eos_min_steps, eos_min_rows, tokens_out, logits_out}, {}}, 1, (hipStream_t)stream};
    const astts_lm_config_t& c = h->cfg;
    const bool f16_64 = c.kv_f16 && c.pos_f16 && (c.d % 64) == 0 && (c.ffn % 64) == 0;
    if (b > 32) {
        ASTTS_REQUIRE(f16_64 && h->g.embed_table, ASTTS_ERR_UNSUPPORTED,
                      "astts_lm_decode: batches of more than 32 rows need the fp16 cache / position tables and the projected embedding table");
        WideWs w;
        carve_wide(h, b, (char*)workspace, &w);
        return run_steps(c, k, w.lg, w.tok, [&](int pos) { return step_wide(h, k, w, pos); });
    }
    NarrowWs w;
    carve_narrow(h, b, (char*)workspace, &w);
    // v2 wherever it is supported, else v1; ASTTS_LM_ENGINE=v1 forces v1
    const char* env = getenv("ASTTS_LM_ENGINE");           // read per call: tests switch engines inside one process
    const bool v2_ok = f16_64 && c.d <= 1024;
    if (v2_ok && !(env && !strcmp(env, "v1"))) {
        ASTTS_REQUIRE(NarrowWs::v2_partial_bytes(b, c.heads) <= w.skw_bytes, ASTTS_ERR_WORKSPACE,
                      "astts_lm_decode: the split-key partials of %d rows x %d heads do not fit the %zu-byte split-K area", b, c.heads,
                      w.skw_bytes);
        const NarrowWs::V2 v = w.v2(b, c.heads);
        return run_steps(c, k, w.lg, w.tok, [&](int pos) { return step_v2(h, k, v, pos); });
    }
    ASTTS_CHECK_HIP(hipMemsetAsync(w.skw, 0, 1024, k.st));      // arrival counters start at zero (once per call; they reset themselves)
    return run_steps(c, k, w.lg, w.tok, [&](int pos) { return step_v1(h, k, w, pos); });
}

// ---- decode session
namespace {

static size_t session_carve(const astts_lm* h, int rows_max, int t_arena, char* base, astts_lm_session* S) {
    Carver c{base};
    for (int l = 0; l < h->cfg.layers; ++l) {
        _Float16* p = c.take<_Float16>((size_t)t_arena * rows_max * 2 * h->cfg.d);
        if (S) S->arena.p[l] = p;
    }
    int32_t* ks = c.take<int32_t>(rows_max);
    if (S) S->kstart = ks;
    const size_t o = align_up(c.o, 256);
    return o + carve_narrow(h, rows_max, base ? base + o : nullptr, S ? &S->ws : nullptr);
}

// the launch set of rows [r0, r0 + rows) of a session: a DecodeCall whose pointers lead to row r0 of the arena, of key_start and of the workspace
struct RowWindow {
    DecodeCall k;
    NarrowWs::V2 v;
    void* kv[kSessionMaxLayers];
    RowWindow(const astts_lm_session* S, int r0, int rows) {
        const astts_lm_config_t& c = S->h->cfg;
        memset(&k, 0, sizeof(k));
        for (int l = 0; l < c.layers; ++l) kv[l] = S->arena.p[l] + (size_t)r0 * 2 * c.d;
        v = S->ws.v2(S->plan.rows_max, c.heads);
        v.h1 += (size_t)r0 * c.d; v.xa += (size_t)r0 * c.d; v.xb += (size_t)r0 * c.d; v.q += (size_t)r0 * c.d;
        v.ff += (size_t)r0 * c.ffn; v.part_o += (size_t)r0 * c.heads * 2 * 64; v.part_ml += (size_t)r0 * c.heads * 2 * 2;
        v.lg += (size_t)r0 * c.vocab_out; v.tok += r0;
        k.logits0 = v.lg; k.kv_cache = kv; k.key_start = S->kstart + r0; k.t_max = S->plan.t_arena; k.b = rows;
        k.kv_rows = S->plan.rows_max; k.st = S->st;
    }
    RowWindow(const RowWindow&) = delete;
};

}  // namespace

size_t astts_lm_session_bytes(const astts_lm_t* h, int32_t rows_max, int32_t t_arena) {
    if (!h || rows_max < 1 || rows_max > 32 || t_arena < 4) return 0;
    return session_carve(h, rows_max, t_arena, nullptr, nullptr);
}

int astts_lm_session_create(astts_lm_t* h, int32_t rows_max, int32_t t_arena, astts_stream_t stream, astts_lm_session_t** out) {
    ASTTS_REQUIRE(h && out, ASTTS_ERR_INVALID, "astts_lm_session_create: null argument");
    const astts_lm_config_t& c = h->cfg;
    ASTTS_REQUIRE(c.kv_f16 && c.pos_f16 && (c.d % 64) == 0 && (c.ffn % 64) == 0 && c.d <= 1024 && c.layers <= kSessionMaxLayers, ASTTS_ERR_UNSUPPORTED,
                  "astts_lm_session_create: a session runs the decode-step kernels only (fp16 cache and position tables, d <= 1024, <= %d layers)",
                  kSessionMaxLayers);
    SessionPlan plan;
    ASTTS_REQUIRE(plan.init(rows_max, t_arena) == SESSION_OK, ASTTS_ERR_INVALID, "astts_lm_session_create: rows_max=%d (1..32) t_arena=%d", rows_max, t_arena);
    ASTTS_REQUIRE(plan.half() <= c.pos_center, ASTTS_ERR_RANGE, "astts_lm_session_create: windows of t_arena / 2 = %d keys pass the position table (%d)",
                  plan.half(), c.pos_center);
    ASTTS_REQUIRE(NarrowWs::v2_partial_bytes(rows_max, c.heads) <= astts_op_gemm_fused_workspace_bytes(), ASTTS_ERR_WORKSPACE,
                  "astts_lm_session_create: the split-key partials of %d rows x %d heads do not fit the split-K area", rows_max, c.heads);
    astts_lm_session* S = new astts_lm_session();
    S->h = h; S->st = (hipStream_t)stream; S->plan = plan; S->rebases = 0;
    const size_t bytes = session_carve(h, rows_max, t_arena, nullptr, nullptr);
    if (hipMalloc((void**)&S->mem, bytes) != hipSuccess) {
        delete S;
        set_error("astts_lm_session_create: hipMalloc of %zu bytes failed", bytes);
        return ASTTS_ERR_HIP;
    }
    session_carve(h, rows_max, t_arena, S->mem, S);
    *out = S;
    return ASTTS_OK;
}

int astts_lm_session_destroy(astts_lm_session_t* S) {
    if (!S) return ASTTS_OK;
    ASTTS_CHECK_HIP(hipStreamSynchronize(S->st));
    ASTTS_CHECK_HIP(hipFree(S->mem));
    delete S;
    return ASTTS_OK;
}

int astts_lm_session_can_admit(const astts_lm_session_t* S, int32_t b, int32_t pos0, int32_t n_steps) {
    return S ? S->plan.admissible(b, pos0, n_steps) : SESSION_ERR_ARG;
}

int astts_lm_session_admit(astts_lm_session_t* S, const float* logits0, void* const* kv_cache, const int32_t* key_start, int32_t t_max,
                           int32_t b, int32_t pos0, int32_t n_steps, const float* uniforms, const int32_t* forced_tokens,
                           int32_t eos_min_steps, const int32_t* eos_min_rows, int32_t* tokens_out, float* logits_out, int32_t* slot_out) {
    ASTTS_REQUIRE(S && logits0 && kv_cache && uniforms && tokens_out && slot_out, ASTTS_ERR_INVALID, "astts_lm_session_admit: null argument");
    ASTTS_REQUIRE(b >= 1 && n_steps >= 1 && pos0 >= 1 && pos0 + n_steps - 1 <= t_max, ASTTS_ERR_INVALID,
                  "astts_lm_session_admit: b=%d pos0=%d n_steps=%d t_max=%d", b, pos0, n_steps, t_max);
    const int slot = S->plan.admit(b, pos0, n_steps);
    ASTTS_REQUIRE(slot >= 0, slot == SESSION_ERR_ARG ? ASTTS_ERR_INVALID : ASTTS_ERR_RANGE,
                  "astts_lm_session_admit: %s (b=%d of %d rows, window %d of %d keys, %d groups active)",
                  slot == SESSION_ERR_FULL ? "both slots are taken" : slot == SESSION_ERR_WINDOW ? "the window is longer than t_arena / 2"
                                                                                                  : "no free rows beside the running group",
                  b, S->plan.rows_max, pos0 + n_steps - 1, S->plan.half(), S->plan.n_active());
    const SessionGroup& G = S->plan.g[slot];
    const astts_lm_config_t& c = S->h->cfg;
    KvPtrs src, dst;
    for (int l = 0; l < kSessionMaxLayers; ++l) {
        src.p[l] = l < c.layers ? (_Float16*)kv_cache[l] : nullptr;
        dst.p[l] = l < c.layers ? S->arena.p[l] + (size_t)G.row0 * 2 * c.d : nullptr;
    }
    hipLaunchKernelGGL(lm_kv_admit, dim3(pos0, c.layers), dim3(256), 0, S->st, src, dst, key_start, S->kstart + G.row0, b, G.win_start,
                       (int64_t)b * 2 * c.d, (int64_t)S->plan.rows_max * 2 * c.d, c.d / 4);
    ASTTS_CHECK_LAUNCH();
    ASTTS_CHECK_HIP(hipMemcpyAsync(S->ws.lg + (size_t)G.row0 * c.vocab_out, logits0, sizeof(float) * (size_t)b * c.vocab_out, hipMemcpyDeviceToDevice, S->st));
    S->rows[slot] = RowGroup{G.row0, b, n_steps, 0, uniforms, forced_tokens, eos_min_steps, eos_min_rows, tokens_out, logits_out};
    *slot_out = slot;
    return ASTTS_OK;
}

int astts_lm_session_step(astts_lm_session_t* S, int32_t k, uint32_t* finished_mask_out) {
    ASTTS_REQUIRE(S && k >= 1, ASTTS_ERR_INVALID, "astts_lm_session_step: null session or k=%d", k);
    const astts_lm* h = S->h;
    const astts_lm_config_t& c = h->cfg;
    SessionPlan& P = S->plan;
    uint32_t done = 0;
    int left = k;
    while (left > 0 && P.n_active() > 0) {
        if (P.needs_rebase()) {
            int r0 = 0, rows = 0;
            P.cover(&r0, &rows);
            const SessionPlan::Rebase rb = P.rebase();
            ASTTS_REQUIRE(rb.n > 0 && rb.delta > 0, ASTTS_ERR_RANGE, "astts_lm_session_step: no legal rebase at position %d of %d", P.pos, P.t_arena);
            KvPtrs kv;
            for (int l = 0; l < kSessionMaxLayers; ++l) kv.p[l] = l < c.layers ? S->arena.p[l] + (size_t)r0 * 2 * c.d : nullptr;
            hipLaunchKernelGGL(lm_kv_rebase, dim3(rb.n, c.layers), dim3(256), 0, S->st, kv, S->kstart + r0, rows, rb.src0, rb.delta,
                               (int64_t)P.rows_max * 2 * c.d, c.d / 4);
            ASTTS_CHECK_LAUNCH();
            ++S->rebases;
        }
        const int q = P.quantum(left);
        ASTTS_REQUIRE(q >= 1, ASTTS_ERR_RANGE, "astts_lm_session_step: no step fits at position %d of %d", P.pos, P.t_arena);
        int r0 = 0, rows = 0;
        P.cover(&r0, &rows);
        RowWindow all(S, r0, rows);
        all.k.pos0 = P.pos; all.k.s_begin = 0; all.k.s_end = q;
        // groups in row order: the sampler's first group starts at the window's row 0
        const int first = (P.g[0].active && (!P.g[1].active || P.g[0].row0 < P.g[1].row0)) ? 0 : 1;
        for (int i = 0; i < SessionPlan::kGroups; ++i) {
            const int gi = i == 0 ? first : 1 - first;
            if (!P.g[gi].active) continue;
            RowGroup r = S->rows[gi];
            r.row0 = P.g[gi].row0 - r0;
            r.s_off = P.g[gi].step;
            all.k.g[all.k.n_groups++] = r;
        }
        // the range's last step: a group that ends there only samples; the forward pass then covers the rows of the groups that go on
        int s0 = 0, srows = 0;
        const bool narrower = P.cover(&s0, &srows, q - 1, true) && (s0 != r0 || srows != rows);
        RowWindow rest(S, narrower ? s0 : r0, narrower ? srows : rows);
        RUN(run_steps(c, all.k, all.v.lg, all.v.tok, [&](int pos) {
            const bool tail = narrower && pos == P.pos + q - 1;
            return step_v2(h, tail ? rest.k : all.k, tail ? rest.v : all.v, pos);
        }));
        done |= P.advance(q);
        left -= q;
    }
    if (finished_mask_out) *finished_mask_out = done;
    return ASTTS_OK;
}

int astts_lm_session_state(const astts_lm_session_t* S, int32_t* out6) {
    ASTTS_REQUIRE(S && out6, ASTTS_ERR_INVALID, "astts_lm_session_state: null argument");
    const SessionPlan& P = S->plan;
    out6[0] = P.g[0].active | P.g[1].active << 1;
    out6[1] = P.pos;
    out6[2] = P.g[0].active ? P.g[0].n_steps - P.g[0].step : 0;
    out6[3] = P.g[1].active ? P.g[1].n_steps - P.g[1].step : 0;
    out6[4] = (int32_t)S->rebases;
    out6[5] = P.half();
    return ASTTS_OK;
}

}  // extern "C"
