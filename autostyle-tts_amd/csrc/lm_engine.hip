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
#include "common.h"
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

// what astts_lm_decode received (include/astts.h), after validation
struct DecodeCall {
    const float* logits0;
    void* const* kv_cache;
    const int32_t* key_start;
    int32_t t_max, b, pos0, n_steps, s_begin, s_end;
    const float* uniforms;
    const int32_t* forced_tokens;
    int32_t eos_min_steps;
    const int32_t* eos_min_rows;
    int32_t* tokens_out;
    float* logits_out;
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
template <class Advance>
int run_steps(const astts_lm_config_t& c, const DecodeCall& k, float* lg, int32_t* tok, Advance advance) {
    const float* cur = k.s_begin == 0 ? k.logits0 : lg;
    for (int s = k.s_begin; s < k.s_end; ++s) {
        if (k.logits_out)
            ASTTS_CHECK_HIP(hipMemcpy2DAsync(k.logits_out + (size_t)s * c.vocab_out, sizeof(float) * (size_t)k.n_steps * c.vocab_out,
                                             cur, sizeof(float) * c.vocab_out, sizeof(float) * c.vocab_out, k.b,
                                             hipMemcpyDeviceToDevice, k.st));
        RUN(astts_op_ras_sample_ex(cur, k.tokens_out, k.uniforms + (size_t)s * k.b * 2, tok, k.b, c.vocab_out, s, k.n_steps, c.top_k,
                                   c.top_p, c.ras_win, c.ras_tau, c.speech_vocab, (s < k.eos_min_steps ? 1 : 0) | (c.eos_policy ? 2 : 0),
                                   k.eos_min_rows, k.forced_tokens, k.st));
        if (s + 1 == k.n_steps) break;
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
    const KvLayout lay = KvLayout::time_major(b, d);
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

}  // namespace

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
    const DecodeCall k = {logits0, kv_cache, key_start, t_max, b, pos0, n_steps, s_begin, s_end, uniforms, forced_tokens,
                          eos_min_steps, eos_min_rows, tokens_out, logits_out, (hipStream_t)stream};
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

}  // extern "C"
