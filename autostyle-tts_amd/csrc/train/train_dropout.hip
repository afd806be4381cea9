// train_dropout.hip -- libastts_train.so: the regularisers of the reference's fine-tuning recipe.  LoRA dropout whose masks are never
// stored (philox.h: regenerated in the operand load of the down GEMM and in the epilogue of the dX product; the dA product is in
// train_ops.hip beside the kernel it extends) and NEFTune's embedding noise.  peft gives every LoRA module its own nn.Dropout, so the
// projections that share an input (q | k | v, gate | up) mask it independently: part j of a call uses stream rng_stream + j.
#include "philox.h"
#include "train_common.h"

namespace astts_train {

// ---- the keep mask itself, uint8 [rows, cin]: one thread per group of 8 columns (the test hook that pins the generator)
__global__ __launch_bounds__(256) void dropout_mask_groups(uint8_t* __restrict__ mask, int64_t groups, uint32_t stream, drop_key key) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const uint32_t m = dropout_keep_bits(key, (uint64_t)g, stream);
    uint2 o;
    o.x = (m & 1u) | ((m >> 1 & 1u) << 8) | ((m >> 2 & 1u) << 16) | ((m >> 3 & 1u) << 24);
    o.y = (m >> 4 & 1u) | ((m >> 5 & 1u) << 8) | ((m >> 6 & 1u) << 16) | ((m >> 7 & 1u) << 24);
    reinterpret_cast<uint2*>(mask)[g] = o;
}

// ---- NEFTune, in place on fp32: x += mag (2u - 1), u = ((bits >> 8) + 0.5) 2^-24.  2u - 1 = (2 (bits >> 8) + 1 - 2^24) 2^-24 is an odd
// integer below 2^24 in magnitude times a power of two: exact in fp32, never 0 and never +-1; the fma rounds once
__global__ __launch_bounds__(256) void neftune_groups(float* __restrict__ x, int64_t groups, float mag, drop_key key) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const philox_out o = philox_group(key, (uint64_t)g, NEFTUNE_STREAM);
    float4 v = reinterpret_cast<float4*>(x)[g];
    float* pv = &v.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int s = (int)(2u * (o.w[i] >> 8) + 1u) - (1 << 24);
        pv[i] = fmaf(mag, (float)s * 0x1p-24f, pv[i]);
    }
    reinterpret_cast<float4*>(x)[g] = v;
}

// ---- t[rows, parts * r] = sum_j (mask_j o x) A_j^T / (1 - p), fp16.  One workgroup per 32 rows, its four waves on interleaved
// 64-column chunks of cin; a wave's tile is D[M = row][N = rank column]: x is the A operand (the lane's row, 8 consecutive columns:
// one 16-byte load = one dropout group, read once and masked per part in registers), the stacked A the B operand.  A 32-column tile
// of t may span several parts (r < 32): part j's product takes the B operand with the other parts' columns zeroed.  The four
// partial tiles meet in LDS and are added in wave order; the sum is scaled in fp32 and rounded to fp16 once.
static constexpr int LD_WAVES = 4;

template <int NT>
__global__ __launch_bounds__(256) void lora_down_rows(const _Float16* __restrict__ x, int64_t ldx, const _Float16* __restrict__ a, int64_t lda,
                                                      _Float16* __restrict__ t, int64_t ldt, int64_t rows, int cin, int parts, int r,
                                                      uint32_t stream, drop_key key, float scale) {
    __shared__ float red[LD_WAVES][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, hh = lane >> 5;
    const int64_t row = (int64_t)blockIdx.x * 32 + c;
    const bool row_ok = row < rows;
    const int n_all = parts * r;
    float16v acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.0f;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    for (int kc = wave * 64; kc < cin; kc += LD_WAVES * 64) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int k = kc + ks * 16 + hh * 8;
            if (kc + ks * 16 >= cin) continue;                                // wave-uniform
            const bool k_ok = k < cin;
            uint4 xf = zero4;
            if (row_ok && k_ok) xf = *reinterpret_cast<const uint4*>(x + row * ldx + k);
            uint4 bf[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = nt * 32 + c;
                bf[nt] = (n < n_all && k_ok) ? *reinterpret_cast<const uint4*>(a + (int64_t)n * lda + k) : zero4;
            }
            const uint64_t group = ((uint64_t)row * (uint64_t)cin + (uint64_t)k) >> 3;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j >= parts) continue;
                uint4 xm = xf;
                if (key.thr) {
                    const keep_words m = dropout_keep_words(key, group, stream + j);
                    xm.x &= m.w[0], xm.y &= m.w[1], xm.z &= m.w[2], xm.w &= m.w[3];
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    if (j * r >= (nt + 1) * 32 || (j + 1) * r <= nt * 32) continue;          // part j has no column in this tile
                    const int n = nt * 32 + c;
                    const uint4 bm = (n >= j * r && n < (j + 1) * r) ? bf[nt] : zero4;
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, xm), __builtin_bit_cast(half8, bm), acc[nt], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        __syncthreads();                                                      // the previous tile's readers are done
#pragma unroll
        for (int e = 0; e < 16; ++e) red[wave][e][lane] = acc[nt][e];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = threadIdx.x + 256 * q, e = idx >> 6, l = idx & 63;
            const float s = ((red[0][e][l] + red[1][e][l]) + red[2][e][l]) + red[3][e][l];
            const int64_t orow = (int64_t)blockIdx.x * 32 + mfma_row(e, l >> 5);
            const int n = nt * 32 + (l & 31);
            if (orow < rows && n < n_all) t[orow * ldt + n] = (_Float16)(s * scale);
        }
    }
}

// ---- dx[rows, cin] = residual + scale * sum_j mask_j o (dt_j A_j).  One wave per (32 columns, 32 rows) tile, D[M = column][N = row]:
// the transposed stack A^T [cin, parts * r] is the A operand, dt the B operand (16-byte loads both), so a lane holds one row and, in
// registers 4g .. 4g + 3, columns 8g + 4 (lane >> 5) + 0..3.  The two lane halves trade one quad per pair of g: every lane then
// holds two whole dropout groups of 8 consecutive columns -- one Philox call per part masks one group in the epilogue, and residual
// and dx move in 16-byte accesses, in one pass.  In place (dx = residual) is allowed.
template <bool OUT_F16>
__global__ __launch_bounds__(256) void lora_dx_dropout_tiles(const _Float16* __restrict__ dt, int64_t lddt, const _Float16* __restrict__ at,
                                                             int64_t ldat, const float* residual, void* dx_, int64_t rows, int cin, int parts,
                                                             int r, uint32_t stream, drop_key key, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, hh = lane >> 5;
    const int col0 = (blockIdx.x * 4 + wave) * 32;
    if (col0 >= cin) return;
    const int64_t row = (int64_t)blockIdx.y * 32 + c;
    const bool row_ok = row < rows, col_ok = col0 + c < cin;
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    float tot[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) tot[e] = 0.0f;
    for (int j = 0; j < parts; ++j) {
        float16v acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int k0 = 0; k0 < r; k0 += 16) {
            const int k = k0 + hh * 8;
            uint4 af = zero4, bf = zero4;
            if (k < r) {
                if (col_ok) af = *reinterpret_cast<const uint4*>(at + (int64_t)(col0 + c) * ldat + j * r + k);
                if (row_ok) bf = *reinterpret_cast<const uint4*>(dt + row * lddt + j * r + k);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, af), __builtin_bit_cast(half8, bf), acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            // registers 8q .. 8q + 3 (X) and 8q + 4 .. 8q + 7 (Y): the low half keeps X and takes the high half's X (columns 16q .. 16q + 7),
            // the high half keeps Y and takes the low half's Y (columns 16q + 8 .. 16q + 15)
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float xq = acc[8 * q + i], yq = acc[8 * q + 4 + i];
                const float got = __shfl_xor(hh ? xq : yq, 32, 64);
                v[i] = hh ? got : xq;
                v[4 + i] = hh ? yq : got;
            }
            uint32_t keep = 0xFFu;
            if (key.thr) {
                const int col = col0 + 16 * q + 8 * hh;
                keep = dropout_keep_bits(key, ((uint64_t)row * (uint64_t)cin + (uint64_t)col) >> 3, stream + j);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) tot[8 * q + i] += (keep >> i & 1u) ? v[i] : 0.0f;
        }
    }
    if (!row_ok) return;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = col0 + 16 * q + 8 * hh;
        if (col >= cin) continue;                                             // cin is a multiple of 8: a group is inside or outside
        const int64_t o = row * (int64_t)cin + col;
        const float4 r0 = *reinterpret_cast<const float4*>(residual + o), r1 = *reinterpret_cast<const float4*>(residual + o + 4);
        const float res[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
        float out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = fmaf(scale, tot[8 * q + i], res[i]);
        if (OUT_F16) {
            half8 h;
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = (_Float16)out[i];
            *reinterpret_cast<half8*>(reinterpret_cast<_Float16*>(dx_) + o) = h;
        } else {
            float* d = reinterpret_cast<float*>(dx_) + o;
            *reinterpret_cast<float4*>(d) = make_float4(out[0], out[1], out[2], out[3]);
            *reinterpret_cast<float4*>(d + 4) = make_float4(out[4], out[5], out[6], out[7]);
        }
    }
}

}  // namespace astts_train

using namespace astts_train;

static bool drop_key_from(int64_t seed, uint32_t draw, double p, drop_key* key, float* scale) {
    if (!(p >= 0.0 && p < 1.0)) return false;
    key->seed_lo = (uint32_t)(uint64_t)seed;
    key->seed_hi = (uint32_t)((uint64_t)seed >> 32);
    key->draw = draw;
    key->thr = (uint32_t)(p * 65536.0);                                       // floor: p >= 0
    if (scale) *scale = (float)(1.0 / (1.0 - p));
    return true;
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" {

int astts_train_dropout_mask(void* mask_u8, int64_t rows, int32_t cin, double p, int64_t seed, uint32_t rng_stream, uint32_t draw,
                             astts_stream_t stream) {
    drop_key key;
    TRAIN_REQUIRE(mask_u8 && rows > 0 && cin > 0 && cin % 8 == 0 && ((uintptr_t)mask_u8 & 7) == 0, ASTTS_ERR_INVALID,
                  "dropout_mask: bad arguments (rows %lld cin %d: a multiple of 8; mask 8-byte aligned)", (long long)rows, cin);
    TRAIN_REQUIRE(drop_key_from(seed, draw, p, &key, nullptr), ASTTS_ERR_INVALID, "dropout_mask: p = %g is outside [0, 1)", p);
    const int64_t groups = rows * (cin / 8), blocks = cdiv(groups, 256);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "dropout_mask: %lld groups exceed the grid", (long long)groups);
    hipLaunchKernelGGL(dropout_mask_groups, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint8_t*)mask_u8, groups, rng_stream, key);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_neftune(float* x, int64_t rows, int32_t hidden, float mag, int64_t seed, uint32_t draw, astts_stream_t stream) {
    drop_key key;
    TRAIN_REQUIRE(x && rows > 0 && hidden > 0 && hidden % 4 == 0 && aligned16(x) && mag >= 0.0f, ASTTS_ERR_INVALID,
                  "neftune: bad arguments (rows %lld hidden %d: a multiple of 4; x 16-byte aligned; mag %g >= 0)", (long long)rows, hidden, (double)mag);
    drop_key_from(seed, draw, 0.0, &key, nullptr);
    const int64_t groups = rows * (hidden / 4), blocks = cdiv(groups, 256);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "neftune: %lld groups exceed the grid", (long long)groups);
    hipLaunchKernelGGL(neftune_groups, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, groups, mag, key);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_lora_down(const void* x_f16, int64_t ldx, const void* a_f16, int64_t lda, void* t_f16, int64_t ldt, int64_t rows,
                          int32_t cin, int32_t parts, int32_t r, double p, int64_t seed, uint32_t rng_stream, uint32_t draw,
                          astts_stream_t stream) {
    drop_key key;
    float scale;
    TRAIN_REQUIRE(x_f16 && a_f16 && t_f16 && rows > 0 && cin > 0 && cin % 8 == 0 && parts >= 1 && parts <= 3 && r >= 8 && r <= 64 && r % 8 == 0,
                  ASTTS_ERR_INVALID, "lora_down: bad arguments (rows %lld cin %d: a multiple of 8; parts %d in 1..3; r %d: a multiple of 8 up to 64)",
                  (long long)rows, cin, parts, r);
    TRAIN_REQUIRE(ldx >= cin && lda >= cin && ldt >= parts * r && ldx % 8 == 0 && lda % 8 == 0 && aligned16(x_f16) && aligned16(a_f16),
                  ASTTS_ERR_INVALID, "lora_down: row strides (ldx %lld lda %lld ldt %lld) must cover the rows, and x and A must allow 16-byte loads",
                  (long long)ldx, (long long)lda, (long long)ldt);
    TRAIN_REQUIRE(drop_key_from(seed, draw, p, &key, &scale), ASTTS_ERR_INVALID, "lora_down: p = %g is outside [0, 1)", p);
    const int64_t blocks = cdiv(rows, 32);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "lora_down: %lld rows exceed the grid", (long long)rows);
    const int nt = (int)cdiv(parts * r, 32);
#define LORA_DOWN_LAUNCH(NT)                                                                                                              \
    hipLaunchKernelGGL(lora_down_rows<NT>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x_f16, ldx,        \
                       (const _Float16*)a_f16, lda, (_Float16*)t_f16, ldt, rows, cin, parts, r, rng_stream, key, scale)
    switch (nt) {
        case 1: LORA_DOWN_LAUNCH(1); break;
        case 2: LORA_DOWN_LAUNCH(2); break;
        case 3: LORA_DOWN_LAUNCH(3); break;
        case 4: LORA_DOWN_LAUNCH(4); break;
        case 5: LORA_DOWN_LAUNCH(5); break;
        default: LORA_DOWN_LAUNCH(6); break;
    }
#undef LORA_DOWN_LAUNCH
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_lora_dx_dropout(const void* dt_f16, int64_t lddt, const void* at_f16, int64_t ldat, const float* residual, void* dx,
                                int32_t dx_f16, int64_t rows, int32_t cin, int32_t parts, int32_t r, double p, int64_t seed,
                                uint32_t rng_stream, uint32_t draw, astts_stream_t stream) {
    drop_key key;
    float scale;
    TRAIN_REQUIRE(dt_f16 && at_f16 && residual && dx && rows > 0 && cin > 0 && cin % 8 == 0 && parts >= 1 && parts <= 3 && r >= 8 && r <= 64 && r % 8 == 0,
                  ASTTS_ERR_INVALID, "lora_dx_dropout: bad arguments (rows %lld cin %d: a multiple of 8; parts %d in 1..3; r %d: a multiple of 8 up to 64)",
                  (long long)rows, cin, parts, r);
    TRAIN_REQUIRE(lddt >= parts * r && ldat >= parts * r && lddt % 8 == 0 && ldat % 8 == 0 && aligned16(dt_f16) && aligned16(at_f16) &&
                      aligned16(residual) && aligned16(dx),
                  ASTTS_ERR_INVALID, "lora_dx_dropout: row strides (lddt %lld ldat %lld) must cover parts * r, and every plane must allow 16-byte accesses",
                  (long long)lddt, (long long)ldat);
    TRAIN_REQUIRE(dx_f16 == 0 || dx != (const void*)residual, ASTTS_ERR_INVALID, "lora_dx_dropout: an fp16 dx cannot overwrite the fp32 residual");
    TRAIN_REQUIRE(drop_key_from(seed, draw, p, &key, &scale), ASTTS_ERR_INVALID, "lora_dx_dropout: p = %g is outside [0, 1)", p);
    const int64_t by = cdiv(rows, 32);
    TRAIN_REQUIRE(by <= 65535, ASTTS_ERR_INVALID, "lora_dx_dropout: %lld rows exceed the grid", (long long)rows);
    const dim3 grid((unsigned)cdiv(cin, 128), (unsigned)by);
    if (dx_f16)
        hipLaunchKernelGGL(lora_dx_dropout_tiles<true>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)dt_f16, lddt, (const _Float16*)at_f16,
                           ldat, residual, dx, rows, cin, parts, r, rng_stream, key, scale);
    else
        hipLaunchKernelGGL(lora_dx_dropout_tiles<false>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)dt_f16, lddt, (const _Float16*)at_f16,
                           ldat, residual, dx, rows, cin, parts, r, rng_stream, key, scale);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
