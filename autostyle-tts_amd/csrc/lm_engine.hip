// lm_engine.hip -- autoregressive decode loop of the acoustic transformer, host side in C++.
//
// The reference's hot loop #2: one speech token per step, ~50 steps per audio second,
// inside cosyvoice's TransformerLM.inference (behind tts_with_rag.py:195).  A Python host pays ~10 us
// per operator call; this engine issues the 5-launches-per-layer fused step (astts_op_gemm_fused,
// astts_op_attn_relpos, astts_op_ras_sample) straight from C++ with no host synchronisation:
// sampling, repetition check, EOS masking and the token history all stay on the GPU.
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

// ---- v2: one decode step = sampler + 14 x (QKV, attention, out-proj, FFN-in, FFN-out) + head = 72 launches (73 without
// the projected embedding table)
static int decode_v2(astts_lm* h, const float* logits0, void* const* kv_cache, const int32_t* key_start, int32_t t_max, int32_t b,
                     int32_t pos0, int32_t n_steps, int32_t s_begin, int32_t s_end, const float* uniforms, const int32_t* forced_tokens,
                     int32_t eos_min_steps, const int32_t* eos_min_rows, int32_t* tokens_out, float* logits_out, void* workspace, hipStream_t st) {
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    const int d = c.d;
    char* ws = (char*)workspace;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        void* p = ws + o;
        o = align_up(o + bytes, 256);
        return p;
    };
    // carved from the same workspace as v1 (astts_lm_workspace_bytes covers both layouts)
    float* h1 = (float*)take(sizeof(float) * b * d);                 // embedding projection (before its LayerNorm)
    float* xa = (float*)take(sizeof(float) * b * d);                 // residual stream, ping
    float* xb = (float*)take(sizeof(float) * b * d);                 // residual stream, pong
    float* q = (float*)take(sizeof(float) * b * d);
    _Float16* ff = (_Float16*)take(sizeof(float) * b * c.ffn);      // fp16 FFN hidden (half of the fp32 slot)
    float* lg = (float*)take(sizeof(float) * b * c.vocab_out);
    int32_t* tok = (int32_t*)take(sizeof(int32_t) * b);
    (void)take(sizeof(int32_t) * b);
    // the attention's split-key partials live in v1's split-K area: [b][heads][2][64] + [b][heads][2][2] floats must fit it
    ASTTS_REQUIRE((size_t)b * c.heads * (2 * 64 + 2 * 2) * sizeof(float) <= astts_op_gemm_fused_workspace_bytes(), ASTTS_ERR_WORKSPACE,
                  "astts_lm_decode: the split-key partials of %d rows x %d heads do not fit the %zu-byte split-K area", b, c.heads,
                  astts_op_gemm_fused_workspace_bytes());
    float* part_o = (float*)take(astts_op_gemm_fused_workspace_bytes());
    float* part_ml = part_o + (size_t)b * c.heads * 2 * 64;
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
    // steps [s_begin, s_end) of an n_steps decode: a range that does not start at 0 samples from the logits the previous range left in
    // the workspace (`lg`: the caller passes the SAME workspace, token buffer and cache to every range of one decode)
    const float* cur = s_begin == 0 ? logits0 : lg;
    for (int s = s_begin; s < s_end; ++s) {
        if (logits_out)
            ASTTS_CHECK_HIP(hipMemcpy2DAsync(logits_out + (size_t)s * c.vocab_out, sizeof(float) * (size_t)n_steps * c.vocab_out,
                                             cur, sizeof(float) * c.vocab_out, sizeof(float) * c.vocab_out, b,
                                             hipMemcpyDeviceToDevice, st));
        int rc = astts_op_ras_sample_ex(cur, tokens_out, uniforms + (size_t)s * b * 2, tok, b, c.vocab_out, s, n_steps,
                                        c.top_k, c.top_p, c.ras_win, c.ras_tau, c.speech_vocab, (s < eos_min_steps ? 1 : 0) | (c.eos_policy ? 2 : 0), eos_min_rows, forced_tokens,
                                        st);
        if (rc != ASTTS_OK) return rc;
        if (s + 1 == n_steps) break;
        const int pos = pos0 + s;
        // embed projection: speech_embedding[tok] -> Linear.  Its LayerNorm -> ReLU -> * sqrt(d) runs inside layer 0's QKV
        // kernel (pre-transform of the staged rows; workgroup 0 writes the result to xa, the residual stream).
        // With the projected table (globals.embed_table = speech_emb W^T + b, formed at load) the projection is a gather as well.
        GemvArgs a = gemv();
        if (!g.embed_table) {
            a.x = g.speech_emb; a.gather = tok; a.ldx = d; a.w = (const _Float16*)g.embed_w; a.bias = g.embed_b; a.out = h1; a.ldo = d;
            a.n = d; a.k = d; a.kpad = d;
            if ((rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
        }
        // the residual stream alternates between two buffers: layer l reads X[l % 2] and its FFN-out projection leaves X[(l + 1) % 2].
        // FFN-out runs as two K slices per column block (lm_step.h, GemvArgs::ksplit: 256 workgroups with 32 KB of weights each instead
        // of 128 with 64 KB) that meet in the output with one fp32 atomic each, so the output must hold zeros: the FFN-in launch of the
        // layer clears it (its last readers, QKV and the out-projection of the layer, are done by then).
        float* X[2] = {xa, h1};          // (h1 is free once layer 0's QKV has read it)
        float* y = xb;
        for (int l = 0; l < c.layers; ++l) {
            const astts_lm_layer_t& L = h->layers[l];
            _Float16* kvc = (_Float16*)kv_cache[l];
            float* x = X[l & 1];
            float* xn = X[(l + 1) & 1];
            a = gemv();             // LN1 + QKV: q -> `q`, K|V -> cache row `pos`
            if (l == 0) {
                a.x = g.embed_table ? g.embed_table : h1;
                a.gather = g.embed_table ? tok : nullptr;
                a.pre_g = g.embed_ln_g; a.pre_b = g.embed_ln_b; a.pre_scale = sqrtf((float)d); a.pre_out = x;
            } else {
                a.x = x;
            }
            a.ldx = d; with_ln(a, L.n1_g, L.n1_b);
            a.w = (const _Float16*)L.wqkv; a.bias = L.bqkv; a.out = q; a.ldo = d; a.kv = kvc; a.n_split = d; a.kv_t = lay.t; a.kv_b = lay.b; a.kv_h = lay.h; a.kv_v = lay.v; a.pos = pos;
            a.n = 3 * d; a.k = d; a.kpad = d;
            if (!(skip & 4) && (rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
            AttnArgs t;
            memset(&t, 0, sizeof(t));
            t.q = q; t.kv = kvc; t.postab = (const _Float16*)L.pos; t.bias_u = L.bias_u; t.bias_v = L.bias_v; t.kstart = key_start;
            t.part_o = part_o; t.part_ml = part_ml; t.ksplit = ksplit; t.b = b;
            t.h = c.heads; t.ldq = d; t.ldp = c.pos_ld; t.center = c.pos_center;
            if (ksplit == 1) { t.out = ff; t.ldo = d; }      // one workgroup per (row, head): the fp16 FFN buffer is free until FFN-in
            t.d = d; t.scale = scale; t.pos = pos; t.kv_t = lay.t; t.kv_b = lay.b; t.kv_h = lay.h; t.kv_v = lay.v;
            if (!(skip & 8) && (rc = lm_attn_launch(t, st)) != ASTTS_OK) return rc;
            a = gemv();             // out-proj on the merged attention partials + residual
            a.x = part_o; a.x2 = part_ml; a.x_mode = 2;
            if (ksplit == 1) { a.x = ff; a.x2 = nullptr; a.x_mode = 1; a.ldx = d; }
            a.w = (const _Float16*)L.wo; a.bias = L.bo; a.res = x; a.ldr = d; a.out = y; a.ldo = d;
            a.n = d; a.k = d; a.kpad = d;
            if (!(skip & 1) && (rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
            a = gemv();             // LN2 + FFN-in + ReLU -> fp16 hidden (its only consumer is an MFMA operand)
            a.x = y; a.ldx = d; with_ln(a, L.n2_g, L.n2_b);
            a.w = (const _Float16*)L.w1; a.bias = L.b1; a.out16 = ff; a.ldo16 = c.ffn; a.relu = 1; a.n = c.ffn; a.k = d; a.kpad = d;
            if (ffn_split) { a.zero = xn; a.zero_n = b * d; }
            if (!(skip & 16) && (rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
            a = gemv();             // FFN-out + residual
            a.x = ff; a.x_mode = 1; a.ldx = c.ffn; a.w = (const _Float16*)L.w2; a.bias = L.b2; a.res = y; a.ldr = d; a.out = xn; a.ldo = d;
            a.n = d; a.k = c.ffn; a.kpad = c.ffn;
            if (ffn_split) a.ksplit = 2;
            if (!(skip & 2) && (rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
        }
        float* x = X[c.layers & 1];
        a = gemv();                 // after_norm + output head
        a.x = x; a.ldx = d; with_ln(a, g.after_g, g.after_b);
        a.w = (const _Float16*)g.head_w; a.bias = g.head_b; a.out = lg; a.ldo = c.vocab_out; a.n = c.vocab_out; a.k = d; a.kpad = d;
        if ((rc = lm_gemv_launch(a, st)) != ASTTS_OK) return rc;
        cur = lg;
    }
    return ASTTS_OK;
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
static size_t wide_workspace_bytes(const astts_lm* h, int b) {
    const size_t d = h->cfg.d;
    size_t o = 0;
    auto take = [&](size_t bytes) { o = align_up(o + bytes, 256); };
    take(sizeof(float) * b * d);                      // h1: embedding rows
    take(sizeof(float) * b * d);                      // xa
    take(sizeof(float) * b * d);                      // xb
    take(sizeof(_Float16) * b * d);                   // n16: LayerNorm output
    take(sizeof(float) * b * d);                      // q
    take(sizeof(float) * b * d);                      // attention output
    take(sizeof(_Float16) * b * h->cfg.ffn);          // FFN hidden
    take(sizeof(float) * b * h->cfg.vocab_out);       // logits
    take(sizeof(int32_t) * b);                        // token
    return o;
}

static int decode_wide(astts_lm* h, const float* logits0, void* const* kv_cache, const int32_t* key_start, int32_t t_max, int32_t b,
                       int32_t pos0, int32_t n_steps, int32_t s_begin, int32_t s_end, const float* uniforms, const int32_t* forced_tokens,
                       int32_t eos_min_steps, const int32_t* eos_min_rows, int32_t* tokens_out, float* logits_out, void* workspace,
                       astts_stream_t stream) {
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    hipStream_t st = (hipStream_t)stream;
    const int d = c.d;
    ASTTS_REQUIRE(c.kv_f16 && c.pos_f16 && g.embed_table && (d % 64) == 0 && (c.ffn % 64) == 0, ASTTS_ERR_UNSUPPORTED,
                  "astts_lm_decode: batches of more than 32 rows need the fp16 cache / position tables and the projected embedding table");
    char* ws = (char*)workspace;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        void* p = ws + o;
        o = align_up(o + bytes, 256);
        return p;
    };
    float* h1 = (float*)take(sizeof(float) * b * d);
    float* xa = (float*)take(sizeof(float) * b * d);
    float* xb = (float*)take(sizeof(float) * b * d);
    _Float16* n16 = (_Float16*)take(sizeof(_Float16) * b * d);
    float* q = (float*)take(sizeof(float) * b * d);
    float* ao = (float*)take(sizeof(float) * b * d);
    _Float16* ff = (_Float16*)take(sizeof(_Float16) * b * c.ffn);
    float* lg = (float*)take(sizeof(float) * b * c.vocab_out);
    int32_t* tok = (int32_t*)take(sizeof(int32_t) * b);
    const float scale = 0.125f;
    const int64_t kv_row = (int64_t)b * 2 * d;      // one time step of the time-major cache
    // astts_op_gemm_rows: a latency-sized kernel for these shapes; the K | V columns of the q | k | v projection go straight into the
    // cache (seven launches per layer: two LayerNorms, q | k | v, attention, out-projection, FFN-in, FFN-out).  ASTTS_LM_WIDE_GEMM=tile
    // goes back to the tile / ring family (eight per layer).
    static const bool rows_kernel = !(getenv("ASTTS_LM_WIDE_GEMM") && !strcmp(getenv("ASTTS_LM_WIDE_GEMM"), "tile"));
    auto gemm = [&](const void* x, int x16, int k, const void* w, const float* bias, const float* res, void* out, int out16, int n, int ldc, int act) {
        if (rows_kernel)
            return astts_op_gemm_rows(x, x16, w, bias, res, out, out16, nullptr, 0, b, n, 0, k, k, ldc, 0, res ? d : 0, act, stream);
        return astts_op_gemm(x, x16, w, bias, res, nullptr, out, out16, b, n, k, k, 1, k, ldc, res ? d : 0, b, b, 1, 1, 0, act, 1.0f, 0.1f, nullptr, stream);
    };
    // LayerNorm(x) -> fp16 -> projection (optionally with a second destination for the columns >= n_split)
    auto gemm_ln = [&](const float* x, const float* ga, const float* be, const void* w, const float* bias, void* out, int out16, int n, int ldc,
                       int act, void* out2, int n_split, int ldc2) {
        int rc = astts_op_layernorm(x, ga, be, n16, 1, b, d, d, d, c.eps, 0.0f, stream);
        if (rc != ASTTS_OK) return rc;
        if (rows_kernel)
            return astts_op_gemm_rows(n16, 1, w, bias, nullptr, out, out16, out2, 1, b, n, n_split, d, d, ldc, ldc2, 0, act, stream);
        if (!out2) return gemm(n16, 1, d, w, bias, nullptr, out, out16, n, ldc, act);
        if ((rc = gemm(n16, 1, d, w, bias, nullptr, out, out16, n_split, ldc, act)) != ASTTS_OK) return rc;
        return gemm(n16, 1, d, (const _Float16*)w + (size_t)n_split * d, bias + n_split, nullptr, out2, 1, n - n_split, ldc2, act);
    };
    const float* cur = s_begin == 0 ? logits0 : lg;
    for (int s = s_begin; s < s_end; ++s) {
        if (logits_out)
            ASTTS_CHECK_HIP(hipMemcpy2DAsync(logits_out + (size_t)s * c.vocab_out, sizeof(float) * (size_t)n_steps * c.vocab_out,
                                             cur, sizeof(float) * c.vocab_out, sizeof(float) * c.vocab_out, b,
                                             hipMemcpyDeviceToDevice, st));
        int rc = astts_op_ras_sample_ex(cur, tokens_out, uniforms + (size_t)s * b * 2, tok, b, c.vocab_out, s, n_steps,
                                        c.top_k, c.top_p, c.ras_win, c.ras_tau, c.speech_vocab, (s < eos_min_steps ? 1 : 0) | (c.eos_policy ? 2 : 0), eos_min_rows, forced_tokens,
                                        stream);
        if (rc != ASTTS_OK) return rc;
        if (s + 1 == n_steps) break;
        const int pos = pos0 + s;
        // the token's projected embedding (a row of the load-time table) -> LayerNorm -> ReLU -> * sqrt(d)
        if ((rc = astts_op_embedding(g.embed_table, tok, h1, b, d, d, c.speech_vocab, 1.0f, stream)) != ASTTS_OK) return rc;
        if ((rc = astts_op_layernorm(h1, g.embed_ln_g, g.embed_ln_b, xa, 0, b, d, d, d, c.eps, sqrtf((float)d), stream)) != ASTTS_OK) return rc;
        float* x = xa;
        float* y = xb;
        for (int l = 0; l < c.layers; ++l) {
            const astts_lm_layer_t& L = h->layers[l];
            char* kvc = (char*)kv_cache[l];
            if ((rc = gemm_ln(x, L.n1_g, L.n1_b, L.wqkv, L.bqkv, q, 0, 3 * d, d, ASTTS_ACT_NONE, kvc + (size_t)pos * kv_row * 2, d, 2 * d)) != ASTTS_OK)
                return rc;
            rc = astts_op_attn_relpos(q, kvc, kvc + (size_t)d * 2, 1, L.pos, 1, L.bias_u, L.bias_v, nullptr, key_start, ao, b, c.heads, 1, pos + 1,
                                      b * d, (int32_t)kv_row, b * d, c.pos_ld, d, 2 * d, d, pos, c.pos_center, 1, scale, stream);
            if (rc != ASTTS_OK) return rc;
            if ((rc = gemm(ao, 0, d, L.wo, L.bo, x, y, 0, d, d, ASTTS_ACT_NONE)) != ASTTS_OK) return rc;
            if ((rc = gemm_ln(y, L.n2_g, L.n2_b, L.w1, L.b1, ff, 1, c.ffn, c.ffn, ASTTS_ACT_RELU, nullptr, 0, 0)) != ASTTS_OK) return rc;
            if ((rc = gemm(ff, 1, c.ffn, L.w2, L.b2, y, x, 0, d, d, ASTTS_ACT_NONE)) != ASTTS_OK) return rc;
        }
        if ((rc = gemm_ln(x, g.after_g, g.after_b, g.head_w, g.head_b, lg, 0, c.vocab_out, c.vocab_out, ASTTS_ACT_NONE, nullptr, 0, 0)) != ASTTS_OK) return rc;
        cur = lg;
    }
    return ASTTS_OK;
}

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
    if (h && b > 32 && b <= ASTTS_LM_MAX_ROWS) return wide_workspace_bytes(h, b);      // the wide engine's layout (plain GEMMs)
    if (!h || b < 1 || b > 32) return 0;
    const size_t d = h->cfg.d;
    size_t o = 0;
    auto take = [&](size_t bytes) { o = align_up(o + bytes, 256); };
    take(sizeof(float) * b * d);                  // h0
    take(sizeof(float) * b * d);                  // h1
    take(sizeof(float) * b * d);                  // q
    take(sizeof(float) * b * d);                  // attn out
    take(sizeof(float) * b * h->cfg.ffn);         // ffn hidden
    take(sizeof(float) * b * h->cfg.vocab_out);   // logits
    take(sizeof(int32_t) * b);                    // token
    take(sizeof(int32_t) * b);                    // lens
    take(astts_op_gemm_fused_workspace_bytes());  // split-K counters + partial sums (FFN-out projection)
    return o;
}

// logits0: [B, vocab_out] logits of the last prefix position (from the prefill); kv_cache[l]: fp32 or fp16
// (cfg.kv_f16) [t_max, B, 2d] time-major, rows [0, pos0) filled by the prefill.  tokens_out: int32 [B, n_steps].
// Steps [s_begin, s_end) of an n_steps decode: (0, n_steps) is the whole decode; shorter ranges are streaming synthesis (the chain is
// issued hop by hop, a chunk is rendered while the next hop decodes).  The ranges of one decode are issued in order on ONE stream with
// the same cache, token buffer and workspace: the workspace carries the logits from one range to the next, tokens_out the sampler's
// history.
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
    if (b > 32)
        return decode_wide(h, logits0, kv_cache, key_start, t_max, b, pos0, n_steps, s_begin, s_end, uniforms, forced_tokens, eos_min_steps,
                           eos_min_rows, tokens_out, logits_out, workspace, stream);
    const astts_lm_config_t& c = h->cfg;
    const astts_lm_globals_t& g = h->g;
    hipStream_t st = (hipStream_t)stream;
    const int d = c.d;
    const int dpad = (int)align_up((size_t)d, 64), fpad = (int)align_up((size_t)c.ffn, 64);
    // Which step engine: "v2" = the decode-step kernels of lm_step.hip (4 launches fewer per step, one memory round trip per
    // kernel, 8-column workgroups, key-split attention merged by its consumer) for every batch of <= 32 rows: a row's arithmetic
    // there does not depend on the number of rows (lm_step.hip, FORM 2), so 8-, 16- and 32-row chains agree bit for bit.
    // "v1" = the operator chain below (round 1), kept as the second implementation the tests compare with.
    // (A "v3" -- two fused launches per layer with a fixed-point residual stream -- was built in round 4, parity-green and 2.4x slower:
    // EXPERIMENTS.md F holds the log; the code is gone.)  ASTTS_LM_ENGINE=v1|v2 forces one.
    const char* env = getenv("ASTTS_LM_ENGINE");           // read per call: tests switch engines inside one process
    const int forced = !env ? 0 : (!strcmp(env, "v1") ? 1 : (!strcmp(env, "v2") ? 2 : 0));
    const bool v2_ok = c.kv_f16 && c.pos_f16 && (d % 64) == 0 && (c.ffn % 64) == 0 && d <= 1024;
    if (v2_ok && forced != 1)
        return decode_v2(h, logits0, kv_cache, key_start, t_max, b, pos0, n_steps, s_begin, s_end, uniforms, forced_tokens, eos_min_steps,
                         eos_min_rows, tokens_out, logits_out, workspace, st);
    char* ws = (char*)workspace;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        void* p = ws + o;
        o = align_up(o + bytes, 256);
        return p;
    };
    float* h0 = (float*)take(sizeof(float) * b * d);
    float* h1 = (float*)take(sizeof(float) * b * d);
    float* q = (float*)take(sizeof(float) * b * d);
    float* ao = (float*)take(sizeof(float) * b * d);
    float* ff = (float*)take(sizeof(float) * b * c.ffn);
    float* lg = (float*)take(sizeof(float) * b * c.vocab_out);
    int32_t* tok = (int32_t*)take(sizeof(int32_t) * b);
    (void)take(sizeof(int32_t) * b);  // reserved
    const size_t skw_bytes = astts_op_gemm_fused_workspace_bytes();
    void* skw = take(skw_bytes);
    ASTTS_CHECK_HIP(hipMemsetAsync(skw, 0, 1024, st));      // arrival counters start at zero (once per call; they reset themselves)
    const float scale = 0.125f;  // 1/sqrt(64)
    const int64_t kv_row = (int64_t)b * 2 * d;  // one time step of the time-major cache

    const float* cur = s_begin == 0 ? logits0 : lg;
    for (int s = s_begin; s < s_end; ++s) {
        if (logits_out)
            ASTTS_CHECK_HIP(hipMemcpy2DAsync(logits_out + (size_t)s * c.vocab_out, sizeof(float) * (size_t)n_steps * c.vocab_out,
                                             cur, sizeof(float) * c.vocab_out, sizeof(float) * c.vocab_out, b,
                                             hipMemcpyDeviceToDevice, st));
        int rc = astts_op_ras_sample_ex(cur, tokens_out, uniforms + (size_t)s * b * 2, tok, b, c.vocab_out, s, n_steps,
                                        c.top_k, c.top_p, c.ras_win, c.ras_tau, c.speech_vocab, (s < eos_min_steps ? 1 : 0) | (c.eos_policy ? 2 : 0), eos_min_rows, forced_tokens,
                                        st);
        if (rc != ASTTS_OK) return rc;
        if (s + 1 == n_steps) break;
        const int pos = pos0 + s;
        // embed: speech_embedding[tok] -> Linear -> LayerNorm -> ReLU * sqrt(d)
        rc = astts_op_gemm_fused(g.speech_emb, tok, nullptr, nullptr, 0.f, g.embed_w, g.embed_b, nullptr, h1, nullptr, 0, b, d, 0,
                              d, dpad, d, d, 0, 0, ASTTS_ACT_NONE, 1.f, 0.f, skw, skw_bytes, st);
        if (rc != ASTTS_OK) return rc;
        rc = astts_op_layernorm(h1, g.embed_ln_g, g.embed_ln_b, h0, 0, b, d, d, d, c.eps, sqrtf((float)d), st);
        if (rc != ASTTS_OK) return rc;
        float* x = h0;
        float* y = h1;
        for (int l = 0; l < c.layers; ++l) {
            const astts_lm_layer_t& L = h->layers[l];
            char* kvc = (char*)kv_cache[l];
            const size_t esz = c.kv_f16 ? 2 : 4;
            // LN1 + QKV; K|V land in cache row `pos`
            rc = astts_op_gemm_fused(x, nullptr, L.n1_g, L.n1_b, c.eps, L.wqkv, L.bqkv, nullptr, q,
                                  kvc + (size_t)pos * kv_row * esz, c.kv_f16, b, 3 * d, d, d, dpad, d, d, 2 * d, 0,
                                  ASTTS_ACT_NONE, 1.f, 0.f, skw, skw_bytes, st);
            if (rc != ASTTS_OK) return rc;
            rc = astts_op_attn_relpos(q, kvc, kvc + (size_t)d * esz, c.kv_f16, L.pos, c.pos_f16, L.bias_u, L.bias_v, /*lens: every row has pos + 1 keys*/ nullptr, key_start, ao, b,
                                      c.heads, 1, pos + 1, /*ldq*/ b * d, /*ldk*/ (int32_t)kv_row, /*ldo*/ b * d, c.pos_ld,
                                      /*q_bs*/ d, /*k_bs*/ 2 * d, /*o_bs*/ d, pos, c.pos_center, 1, scale, st);
            if (rc != ASTTS_OK) return rc;
            rc = astts_op_gemm_fused(ao, nullptr, nullptr, nullptr, 0.f, L.wo, L.bo, x, y, nullptr, 0, b, d, 0, d, dpad, d, d, 0, d,
                                  ASTTS_ACT_NONE, 1.f, 0.f, skw, skw_bytes, st);
            if (rc != ASTTS_OK) return rc;
            rc = astts_op_gemm_fused(y, nullptr, L.n2_g, L.n2_b, c.eps, L.w1, L.b1, nullptr, ff, nullptr, 0, b, c.ffn, 0, d, dpad, d,
                                  c.ffn, 0, 0, ASTTS_ACT_RELU, 1.f, 0.f, skw, skw_bytes, st);
            if (rc != ASTTS_OK) return rc;
            rc = astts_op_gemm_fused(ff, nullptr, nullptr, nullptr, 0.f, L.w2, L.b2, y, x, nullptr, 0, b, d, 0, c.ffn, fpad, c.ffn, d,
                                  0, d, ASTTS_ACT_NONE, 1.f, 0.f, skw, skw_bytes, st);
            if (rc != ASTTS_OK) return rc;
        }
        // after_norm + output head
        rc = astts_op_gemm_fused(x, nullptr, g.after_g, g.after_b, c.eps, g.head_w, g.head_b, nullptr, lg, nullptr, 0, b, c.vocab_out,
                              0, d, dpad, d, c.vocab_out, 0, 0, ASTTS_ACT_NONE, 1.f, 0.f, skw, skw_bytes, st);
        if (rc != ASTTS_OK) return rc;
        cur = lg;
    }
    return ASTTS_OK;
}

}  // extern "C"
