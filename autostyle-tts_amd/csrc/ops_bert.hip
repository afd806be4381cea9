// ops_bert.hip -- the two row operators of a post-LayerNorm (BERT-family) encoder (include/llm/astts_bert.h): LayerNorm with an fp32 and
// an fp16 copy of the result (the residual stream and the next GEMM's operand), and the same behind the word + position + type embedding
// sum.  Memory-bound row kernels: a row is read once with 16-byte loads, lives in registers through the three sums (mean, the centred
// values' own mean, variance) and leaves with 16-byte stores.  No LDS and no barrier: a row belongs to LPR lanes of ONE wave, and its sums
// are butterflies over those lanes (xlane.h), so the order is fixed and every lane of the row ends with the same bits.
#include "common.h"
#include "xlane.h"
#include "../../include/llm/astts_bert.h"

namespace astts {

// LPR lanes per row (16: a DPP row, four rows per wave; 64: the wave), NV chunks of 8 floats per lane: lane `sub` owns the chunks
// sub, sub + LPR, ... -- neighbouring lanes read neighbouring 32 bytes.  c <= 8 * LPR * NV; a chunk at or beyond c holds zeros.
template <int LPR>
__device__ __forceinline__ float bert_row_sum(float v) {
    static_assert(LPR == 16 || LPR == 64, "a DPP row or the wave");
    if constexpr (LPR == 64) { v = xadd<32>(v); v = xadd<16>(v); }
    v = xadd<8>(v); v = xadd<4>(v); v = xadd<2>(v);
    return xadd<1>(v);
}

__device__ __forceinline__ void bert_load8(const float* p, float (&o)[8]) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
    o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w; o[4] = hi.x; o[5] = hi.y; o[6] = hi.z; o[7] = hi.w;
}

// v (zeros beyond c) -> LayerNorm(v) * gamma + beta, stored as fp32 and / or fp16 when `store`; `zero`: the row is padding and is written as zeros.
// Called by every lane of the wave (the butterflies need them all), whatever `store` says.
template <int LPR, int NV>
__device__ __forceinline__ void bert_ln_store(float (&v)[NV][8], int sub, int c, float eps, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, float* y32, _Float16* y16, bool store, bool zero) {
    const float fc = (float)c;
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
    const float m0 = bert_row_sum<LPR>(s) / fc;               // a true division: c equal values v give (c v) / c = v when c v is exact
    s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool in = (sub + i * LPR) * 8 < c;
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = in ? v[i][e] - m0 : 0.0f; s += v[i][e]; }
    }
    const float m1 = bert_row_sum<LPR>(s) / fc;               // what rounding left in m0: |m1| <= ulp(m0) / 2 + the sum's own error
    s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool in = (sub + i * LPR) * 8 < c;
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = in ? v[i][e] - m1 : 0.0f; s = fmaf(v[i][e], v[i][e], s); }
    }
    const float var = bert_row_sum<LPR>(s) / fc + eps;
    const float rstd = var > 0.0f ? rsqrtf(var) : 0.0f;
    if (!store) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = (sub + i * LPR) * 8;
        if (col >= c) continue;
        float g[8], b[8], y[8];
        bert_load8(gamma + col, g);
        bert_load8(beta + col, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = zero ? 0.0f : fmaf(v[i][e] * rstd, g[e], b[e]);
        if (y32) {
            *reinterpret_cast<float4*>(y32 + col) = make_float4(y[0], y[1], y[2], y[3]);
            *reinterpret_cast<float4*>(y32 + col + 4) = make_float4(y[4], y[5], y[6], y[7]);
        }
        if (y16) {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (_Float16)y[e];                 // the fp32 value above, rounded once
            *reinterpret_cast<half8*>(y16 + col) = h;
        }
    }
}

// The rows of a launch: a wave takes 64 / LPR neighbouring rows per round and strides by the grid.  `base` (the wave's first row of a
// round) is the same in every lane, so a wave runs its rounds with all lanes; a lane group whose row does not exist works on the last
// row again and stores nothing.  x may be y32 (in place): a group reads its whole row before it stores any of it, and a group without a
// row shares its wave -- and so its load instructions -- with the group that owns the last row.
template <int LPR, int NV>
__global__ __launch_bounds__(256) void layernorm_dual(const float* x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* y32, _Float16* __restrict__ y16, int64_t rows, int c, int ldx, int ldy32,
                                                      int ldy16, float eps) {
    constexpr int RPW = 64 / LPR;
    const int sub = threadIdx.x & (LPR - 1), grp = (threadIdx.x & 63) / LPR;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4 * RPW;
    for (int64_t base = wave * RPW; base < rows; base += step) {
        const bool live = base + grp < rows;
        const int64_t r = live ? base + grp : rows - 1;
        float v[NV][8];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = (sub + i * LPR) * 8;
            if (col < c) bert_load8(x + r * ldx + col, v[i]);
            else
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = 0.0f;
        }
        bert_ln_store<LPR, NV>(v, sub, c, eps, gamma, beta, y32 ? y32 + r * ldy32 : nullptr, y16 ? y16 + r * ldy16 : nullptr, live, false);
    }
}

// row = (sequence, token): the three table rows are summed in the order word + pos + type, then the LayerNorm of layernorm_dual.
template <int LPR, int NV>
__global__ __launch_bounds__(256) void bert_embed_ln(const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                                                     const int* __restrict__ ids, const int* __restrict__ type_ids, const int* __restrict__ lens,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ y32,
                                                     _Float16* __restrict__ y16, int64_t rows, int t, int c, int vocab, int max_pos, int n_types,
                                                     int pos_offset, float eps) {
    constexpr int RPW = 64 / LPR;
    const int sub = threadIdx.x & (LPR - 1), grp = (threadIdx.x & 63) / LPR;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), step = (int64_t)gridDim.x * 4 * RPW;
    for (int64_t base = wave * RPW; base < rows; base += step) {
        const bool live = base + grp < rows;
        const int64_t r = live ? base + grp : rows - 1;
        const int bi = (int)(r / t), j = (int)(r - (int64_t)bi * t);
        const bool pad = lens && j >= lens[bi];
        // clamped into the tables: whatever ids, type_ids and pos_offset hold, every address read lies inside its table
        const int64_t wi = min(max(ids[r], 0), vocab - 1), pi = min(max((int64_t)pos_offset + j, (int64_t)0), (int64_t)max_pos - 1);   // the sum in 64 bits: any pos_offset
        const int64_t ti = type_ids ? min(max(type_ids[r], 0), n_types - 1) : 0;
        float v[NV][8];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = (sub + i * LPR) * 8;
            if (col < c) {
                float p[8], q[8];
                bert_load8(word + wi * c + col, v[i]);
                bert_load8(pos + pi * c + col, p);
                bert_load8(type + ti * c + col, q);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = (v[i][e] + p[e]) + q[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i][e] = 0.0f;
            }
        }
        bert_ln_store<LPR, NV>(v, sub, c, eps, gamma, beta, y32 ? y32 + r * c : nullptr, y16 ? y16 + r * c : nullptr, live, pad);
    }
}

// memory-bound: at most 2048 workgroups (eight per CU), the rows beyond that by the grid stride
static inline unsigned bert_grid(int64_t rows, int lpr) { const int64_t g = cdiv(rows * lpr, 256); return (unsigned)(g < 2048 ? g : 2048); }

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the kernel's width for c (8 <= c <= 4096, c % 8 == 0): 16 lanes x 1 chunk up to 128, then the wave with 1, 2, 4 or 8 chunks per lane
#define BERT_DISPATCH(KERNEL, c, rows, stream, ...)                                                                                      \
    do {                                                                                                                                 \
        if ((c) <= 128) hipLaunchKernelGGL((KERNEL<16, 1>), dim3(bert_grid(rows, 16)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);   \
        else if ((c) <= 512) hipLaunchKernelGGL((KERNEL<64, 1>), dim3(bert_grid(rows, 64)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);  \
        else if ((c) <= 1024) hipLaunchKernelGGL((KERNEL<64, 2>), dim3(bert_grid(rows, 64)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
        else if ((c) <= 2048) hipLaunchKernelGGL((KERNEL<64, 4>), dim3(bert_grid(rows, 64)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<64, 8>), dim3(bert_grid(rows, 64)), dim3(256), 0, (hipStream_t)(stream), __VA_ARGS__);             \
    } while (0)

}  // namespace astts

using namespace astts;

extern "C" {

int astts_op_layernorm_dual(const float* x, const float* gamma, const float* beta, float* y32, void* y16, int64_t rows, int32_t c,
                            int32_t ldx, int32_t ldy32, int32_t ldy16, float eps, astts_stream_t stream) {
    ASTTS_REQUIRE(x && gamma && beta && (y32 || y16), ASTTS_ERR_INVALID, "astts_op_layernorm_dual: null pointer (x, gamma, beta; one of y32 / y16)");
    ASTTS_REQUIRE(c >= 8 && c <= 4096 && (c & 7) == 0, ASTTS_ERR_UNSUPPORTED, "astts_op_layernorm_dual: c=%d (built for multiples of 8 from 8 to 4096)", c);
    ASTTS_REQUIRE(rows >= 1 && ldx >= c && (!y32 || ldy32 >= c) && (!y16 || ldy16 >= c) && eps >= 0.0f, ASTTS_ERR_INVALID,
                  "astts_op_layernorm_dual: bad shape rows=%lld c=%d ldx=%d ldy32=%d ldy16=%d eps=%g", (long long)rows, c, ldx, ldy32, ldy16, (double)eps);
    ASTTS_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y32) && aligned16(y16) && (ldx & 3) == 0 &&
                      (!y32 || (ldy32 & 3) == 0) && (!y16 || (ldy16 & 7) == 0),
                  ASTTS_ERR_INVALID, "astts_op_layernorm_dual: pointers and row strides must be 16-byte aligned");
    ASTTS_REQUIRE((const float*)y32 != x || ldy32 == ldx, ASTTS_ERR_INVALID, "astts_op_layernorm_dual: in place needs ldy32 == ldx");
    BERT_DISPATCH(layernorm_dual, c, rows, stream, x, gamma, beta, y32, (_Float16*)y16, rows, c, ldx, ldy32, ldy16, eps);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_op_bert_embed_ln(const float* word, const float* pos, const float* type, const int32_t* ids, const int32_t* type_ids,
                           const int32_t* lens, const float* gamma, const float* beta, float* out32, void* out16, int32_t b, int32_t t,
                           int32_t c, int32_t vocab, int32_t max_pos, int32_t n_types, int32_t pos_offset, float eps, astts_stream_t stream) {
    ASTTS_REQUIRE(word && pos && type && ids && gamma && beta && (out32 || out16), ASTTS_ERR_INVALID,
                  "astts_op_bert_embed_ln: null pointer (the tables, ids, gamma, beta; one of out32 / out16)");
    ASTTS_REQUIRE(c >= 8 && c <= 4096 && (c & 7) == 0, ASTTS_ERR_UNSUPPORTED, "astts_op_bert_embed_ln: c=%d (built for multiples of 8 from 8 to 4096)", c);
    ASTTS_REQUIRE(b >= 1 && t >= 1 && vocab >= 1 && max_pos >= 1 && n_types >= 1 && pos_offset >= 0 && eps >= 0.0f, ASTTS_ERR_INVALID,
                  "astts_op_bert_embed_ln: bad shape b=%d t=%d vocab=%d max_pos=%d n_types=%d pos_offset=%d eps=%g", b, t, vocab, max_pos, n_types,
                  pos_offset, (double)eps);
    ASTTS_REQUIRE(aligned16(word) && aligned16(pos) && aligned16(type) && aligned16(gamma) && aligned16(beta) && aligned16(out32) && aligned16(out16),
                  ASTTS_ERR_INVALID, "astts_op_bert_embed_ln: the tables, gamma, beta and the outputs must be 16-byte aligned");
    const int64_t rows = (int64_t)b * t;
    BERT_DISPATCH(bert_embed_ln, c, rows, stream, word, pos, type, ids, type_ids, lens, gamma, beta, out32, (_Float16*)out16, rows, t, c, vocab,
                  max_pos, n_types, pos_offset, eps);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
