// train_attn.hip -- libastts_train.so: causal grouped-query attention backward at head_dim 128 or 64 on the matrix cores.
//
// Forward (csrc/ops_llm.hip attn_gqa_mfma): S = scale Q K^T (causal, keys < len), P = softmax(S), O = P V.  Backward, per (row, head):
//   dV = P^T dO      dP = dO V^T      D_i = sum_j P_ij dP_ij      dS = P o (dP - D)      dQ = scale dS K      dK = scale dS^T Q
// Two kernels, as flash-attention's backward splits them, so that neither needs an atomic:
//   attn_bwd_dq   one workgroup per (row, head, 128 queries), a wave per 32 queries.  Pass 1 over the key tiles recomputes the softmax
//                 statistics (online max / sum in the log2 domain, as the forward) and D; both go to the workspace.  Pass 2 forms dS and
//                 accumulates dQ^T += K^T dS^T.
//   attn_bwd_dkdv one workgroup per (row, kv head, 128 keys), a wave per 32 keys, looping over the group's query heads and the query
//                 tiles from the diagonal on: dV^T += dO^T P, dK^T += Q^T dS, summed over the group in head order.
// Every product is v_mfma_f32_32x32x16_f16.  The tile that becomes the next product's B operand (P, dS) is taken straight from the
// accumulator registers, whose element order fixes the K order of that product (train_common.h); the matching A operand is read from a
// transposed LDS image.  The kernels are templates on the head dimension D: S and dP take D / 16 k-steps, the dQ^T / dK^T / dV^T
// accumulators are D / 32 dimension tiles, a row-major LDS row is D + 8 halfs.  q is scaled by scale * log2(e) and rounded to fp16
// before S, exactly as the forward does, so P is the forward's.
#include "train_common.h"

namespace astts_train {

// halfs per row of a row-major LDS tile are D + 8 (136 / 72: 16-byte reads of 32 rows spread over the banks)
static constexpr int TS = 40;       // halfs per row of a transposed LDS tile (32 + 8)
static constexpr float LOG2E = 1.44269504088896341f;

struct AttnBwdArgs {
    const _Float16* qkv;
    const _Float16* dout;
    const int* lens;
    _Float16* dqkv;
    float* lse;       // [b, heads, t], log2 domain
    float* dsum;      // [b, heads, t]
    int64_t ldq, ldo, ldg;
    int t, heads, kv_heads;
    float scale;
};

__device__ __forceinline__ float16v zero16() {
    float16v z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

// A operand of a product whose K order follows an accumulator: row `c` of a transposed image, K step s
__device__ __forceinline__ half8 frag_t(const _Float16* img, int row, int s, int hh) {
    const _Float16* p = img + row * TS + 16 * s + 4 * hh;
    const half4 lo = *reinterpret_cast<const half4*>(p);
    const half4 hi = *reinterpret_cast<const half4*>(p + 8);
    half8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
}

// 32 rows x D halfs from global memory (row index clamped to t - 1) into a row-major image (scaled by `mul` when SCALE) and / or a
// transposed one.  256 threads: thread -> (row = tid >> 3, D / 8 dims from (tid & 7) * (D / 8))
template <int D, bool SCALE>
__device__ __forceinline__ void stage_tile(const _Float16* src, int64_t ld, int row0, int t, _Float16* rowimg, _Float16* timg, float mul) {
    constexpr int RS = D + 8, NH = D / 64;
    const int r = threadIdx.x >> 3, d0 = (threadIdx.x & 7) * (D / 8);
    const _Float16* p = src + (int64_t)min(row0 + r, t - 1) * ld + d0;
    half8 x[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) x[h] = *reinterpret_cast<const half8*>(p + 8 * h);
    if (timg) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int h = 0; h < NH; ++h) timg[(d0 + 8 * h + i) * TS + r] = x[h][i];
        }
    }
    if (rowimg) {
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            half8 x2 = x[h];
            if (SCALE) {
#pragma unroll
                for (int i = 0; i < 8; ++i) x2[i] = (_Float16)((float)x[h][i] * mul);
            }
            *reinterpret_cast<half8*>(&rowimg[r * RS + d0 + 8 * h]) = x2;
        }
    }
}

template <int AD>
__global__ __launch_bounds__(256) void attn_bwd_dq(AttnBwdArgs a) {
    constexpr int RS = AD + 8, NS = AD / 16, NDT = AD / 32;
    __shared__ __attribute__((aligned(16))) _Float16 ks[32 * RS];
    __shared__ __attribute__((aligned(16))) _Float16 vs[32 * RS];
    __shared__ __attribute__((aligned(16))) _Float16 kt[AD * TS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int c = lane & 31, hh = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int kvh = head / (a.heads / a.kv_heads);
    const int hq = a.heads * AD, hk = a.kv_heads * AD;
    const int qblk = blockIdx.x * 128, q0 = qblk + wid * 32;
    const int len = a.lens ? min(max(a.lens[b], 0), a.t) : a.t;
    const int kend = min(len, min(qblk + 128, a.t));                  // causal: no key beyond the block's last query
    const _Float16* base = a.qkv + (int64_t)b * a.t * a.ldq;
    const _Float16* kp = base + hq + kvh * AD;
    const _Float16* vp = base + hq + hk + kvh * AD;
    const int qi = q0 + c;
    const bool wave_on = q0 < a.t;                                    // wave-uniform

    // B operands with the QUERY on the lane: Q (scaled as the forward scales it) and dO
    half8 qf[NS], dof[NS];
    {
        const int qr = min(qi, a.t - 1);
        const _Float16* qrow = base + (int64_t)qr * a.ldq + head * AD;
        const _Float16* drow = a.dout + ((int64_t)b * a.t + qr) * a.ldo + head * AD;
        const float sc = a.scale * LOG2E;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const half8 x = *reinterpret_cast<const half8*>(qrow + 16 * s + 8 * hh);
#pragma unroll
            for (int i = 0; i < 8; ++i) qf[s][i] = (_Float16)((float)x[i] * sc);
            dof[s] = *reinterpret_cast<const half8*>(drow + 16 * s + 8 * hh);
        }
    }

    // S^T and dP^T of one staged key tile: element e of lane (c, hh) = (key j0 + mfma_row(e, hh), query q0 + c)
    auto scores = [&](float16v& st, float16v& dp) {
        st = zero16();
        dp = zero16();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const half8 kf = *reinterpret_cast<const half8*>(&ks[c * RS + 16 * s + 8 * hh]);
            const half8 vf = *reinterpret_cast<const half8*>(&vs[c * RS + 16 * s + 8 * hh]);
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, dof[s], dp, 0, 0, 0);
        }
    };

    // ---- pass 1: the softmax statistics and D
    float m_run = -INFINITY, l_run = 0.0f, acc = 0.0f;
    for (int j0 = 0; j0 < kend; j0 += 32) {
        __syncthreads();
        stage_tile<AD, false>(kp, a.ldq, j0, a.t, ks, nullptr, 1.0f);
        stage_tile<AD, false>(vp, a.ldq, j0, a.t, vs, nullptr, 1.0f);
        __syncthreads();
        if (!wave_on || j0 > q0 + 31) continue;                       // wave-uniform: beyond this wave's last query
        float16v st, dp;
        scores(st, dp);
        float mloc = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = j0 + mfma_row(e, hh);
            st[e] = (key < len && key <= qi) ? st[e] : -INFINITY;
            mloc = fmaxf(mloc, st[e]);
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = m_run == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
        acc *= alpha;
        m_run = m_new;
        const float m_use = m_run == -INFINITY ? 0.0f : m_run;        // no valid key yet: every p is exp2(-inf) = 0
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = __builtin_amdgcn_exp2f(st[e] - m_use);
            l_run += p;
            acc += p * dp[e];
        }
    }
    l_run += __shfl_xor(l_run, 32, 64);
    acc += __shfl_xor(acc, 32, 64);
    const bool qvalid = qi < len && l_run > 0.0f;
    const float lse2 = qvalid ? m_run + __log2f(l_run) : 0.0f;
    const float dq_sum = qvalid ? acc / l_run : 0.0f;
    if (hh == 0 && qi < a.t) {
        const int64_t o = ((int64_t)b * a.heads + head) * a.t + qi;
        a.lse[o] = lse2;
        a.dsum[o] = dq_sum;
    }

    // ---- pass 2: dQ^T[dim][query] += K^T[dim][key] dS^T[key][query]
    float16v ot[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) ot[dt] = zero16();
    for (int j0 = 0; j0 < kend; j0 += 32) {
        __syncthreads();
        stage_tile<AD, false>(kp, a.ldq, j0, a.t, ks, kt, 1.0f);
        stage_tile<AD, false>(vp, a.ldq, j0, a.t, vs, nullptr, 1.0f);
        __syncthreads();
        if (!wave_on || j0 > q0 + 31) continue;
        float16v st, dp;
        scores(st, dp);
        half8 dsf[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int key = j0 + mfma_row(e, hh);
            const bool valid = qvalid && key < len && key <= qi;
            const float p = valid ? __builtin_amdgcn_exp2f(st[e] - lse2) : 0.0f;
            dsf[e >> 3][e & 7] = (_Float16)(p * (dp[e] - dq_sum));
        }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int s = 0; s < 2; ++s) ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag_t(kt, dt * 32 + c, s, hh), dsf[s], ot[dt], 0, 0, 0);
    }
    if (qi < a.t) {
        _Float16* orow = a.dqkv + ((int64_t)b * a.t + qi) * a.ldg + head * AD;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 o4;
#pragma unroll
                for (int i = 0; i < 4; ++i) o4[i] = (_Float16)(ot[dt][4 * g + i] * a.scale);
                *reinterpret_cast<half4*>(orow + dt * 32 + 8 * g + 4 * hh) = o4;
            }
    }
}

template <int AD>
__global__ __launch_bounds__(256) void attn_bwd_dkdv(AttnBwdArgs a) {
    constexpr int RS = AD + 8, NS = AD / 16, NDT = AD / 32;
    __shared__ __attribute__((aligned(16))) _Float16 qs[32 * RS];     // Q rows, scaled as the forward scales them
    __shared__ __attribute__((aligned(16))) _Float16 dos[32 * RS];    // dO rows
    __shared__ __attribute__((aligned(16))) _Float16 qt[AD * TS];     // Q^T (unscaled)
    __shared__ __attribute__((aligned(16))) _Float16 dot_t[AD * TS];    // dO^T
    __shared__ float slse[32], sdsum[32];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int c = lane & 31, hh = lane >> 5;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int group = a.heads / a.kv_heads;
    const int hq = a.heads * AD, hk = a.kv_heads * AD;
    const int kblk = blockIdx.x * 128, k0 = kblk + wid * 32;
    const int len = a.lens ? min(max(a.lens[b], 0), a.t) : a.t;
    const _Float16* base = a.qkv + (int64_t)b * a.t * a.ldq;
    const int key = k0 + c;
    const bool wave_on = k0 < len;                                    // wave-uniform: some key of this wave is real

    // B operands with the KEY on the lane: K and V
    half8 kf[NS], vf[NS];
    {
        const _Float16* krow = base + (int64_t)min(key, a.t - 1) * a.ldq + hq + kvh * AD;
        const _Float16* vrow = krow + hk;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            kf[s] = *reinterpret_cast<const half8*>(krow + 16 * s + 8 * hh);
            vf[s] = *reinterpret_cast<const half8*>(vrow + 16 * s + 8 * hh);
        }
    }
    float16v dvt[NDT], dkt[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        dvt[dt] = zero16();
        dkt[dt] = zero16();
    }
    for (int g = 0; g < group; ++g) {                                 // head order: the sum over the group is a fixed sequence
        const int head = kvh * group + g;
        const _Float16* qp = base + head * AD;
        const _Float16* dop = a.dout + (int64_t)b * a.t * a.ldo + head * AD;
        const float* lsep = a.lse + ((int64_t)b * a.heads + head) * a.t;
        const float* dsp = a.dsum + ((int64_t)b * a.heads + head) * a.t;
        for (int t0 = kblk; t0 < len; t0 += 32) {                     // causal: queries from the block's first key on
            __syncthreads();
            stage_tile<AD, true>(qp, a.ldq, t0, a.t, qs, qt, a.scale * LOG2E);
            stage_tile<AD, false>(dop, a.ldo, t0, a.t, dos, dot_t, 1.0f);
            if (tid < 32) {
                const int q = min(t0 + tid, a.t - 1);
                slse[tid] = lsep[q];
                sdsum[tid] = dsp[q];
            }
            __syncthreads();
            if (!wave_on || t0 + 31 < k0) continue;                   // wave-uniform: every query of the tile is before this wave's keys
            // S and dP: element e of lane (c, hh) = (query t0 + mfma_row(e, hh), key k0 + c)
            float16v st = zero16(), dp = zero16();
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const half8 qa = *reinterpret_cast<const half8*>(&qs[c * RS + 16 * s + 8 * hh]);
                const half8 da = *reinterpret_cast<const half8*>(&dos[c * RS + 16 * s + 8 * hh]);
                st = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa, kf[s], st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_f16(da, vf[s], dp, 0, 0, 0);
            }
            half8 pf[2], dsf[2];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = mfma_row(e, hh), q = t0 + r;
                const bool valid = key < len && key <= q && q < len;
                const float p = valid ? __builtin_amdgcn_exp2f(st[e] - slse[r]) : 0.0f;
                pf[e >> 3][e & 7] = (_Float16)p;
                dsf[e >> 3][e & 7] = (_Float16)(p * (dp[e] - sdsum[r]));
            }
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    dvt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag_t(dot_t, dt * 32 + c, s, hh), pf[s], dvt[dt], 0, 0, 0);
                    dkt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag_t(qt, dt * 32 + c, s, hh), dsf[s], dkt[dt], 0, 0, 0);
                }
        }
    }
    if (key < a.t) {
        _Float16* krow = a.dqkv + ((int64_t)b * a.t + key) * a.ldg + hq + kvh * AD;
        _Float16* vrow = krow + hk;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                half4 k4, v4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    k4[i] = (_Float16)(dkt[dt][4 * g + i] * a.scale);
                    v4[i] = (_Float16)dvt[dt][4 * g + i];
                }
                *reinterpret_cast<half4*>(krow + dt * 32 + 8 * g + 4 * hh) = k4;
                *reinterpret_cast<half4*>(vrow + dt * 32 + 8 * g + 4 * hh) = v4;
            }
    }
}

}  // namespace astts_train

using namespace astts_train;

extern "C" {

size_t astts_train_attn_gqa_bwd_workspace_bytes(int32_t b, int32_t t, int32_t heads) {
    if (b <= 0 || t <= 0 || heads <= 0) return 0;
    return 2 * align_up((size_t)b * t * heads * sizeof(float), 256);
}

int astts_train_attn_gqa_bwd(const void* qkv_f16, const void* dout_f16, const int32_t* lens, void* dqkv_f16, int32_t b, int32_t t,
                             int32_t heads, int32_t kv_heads, int32_t head_dim, int64_t ld_qkv, int64_t ld_dout, int64_t ld_dqkv,
                             float scale, void* workspace, size_t workspace_bytes, astts_stream_t stream) {
    TRAIN_REQUIRE(qkv_f16 && dout_f16 && dqkv_f16 && b > 0 && t > 0, ASTTS_ERR_INVALID, "attn_gqa_bwd: null pointer or empty batch");
    TRAIN_REQUIRE(head_dim == 64 || head_dim == 128, ASTTS_ERR_UNSUPPORTED, "attn_gqa_bwd: head_dim %d (built for 64 and 128)", head_dim);
    const int AD = head_dim;
    TRAIN_REQUIRE(heads > 0 && kv_heads > 0 && heads % kv_heads == 0, ASTTS_ERR_INVALID, "attn_gqa_bwd: %d heads over %d kv heads", heads, kv_heads);
    const int64_t width = (int64_t)(heads + 2 * kv_heads) * AD;
    TRAIN_REQUIRE(ld_qkv >= width && ld_dqkv >= width && ld_dout >= (int64_t)heads * AD && ld_qkv % 8 == 0 && ld_dqkv % 8 == 0 && ld_dout % 8 == 0,
                  ASTTS_ERR_INVALID, "attn_gqa_bwd: row strides %lld / %lld / %lld (multiples of 8, at least the plane's width)",
                  (long long)ld_qkv, (long long)ld_dout, (long long)ld_dqkv);
    TRAIN_REQUIRE((((uintptr_t)qkv_f16 | (uintptr_t)dout_f16 | (uintptr_t)dqkv_f16) & 15) == 0, ASTTS_ERR_INVALID, "attn_gqa_bwd: planes must be 16-byte aligned");
    TRAIN_REQUIRE(b <= 65535 && heads <= 65535, ASTTS_ERR_INVALID, "attn_gqa_bwd: batch %d / heads %d exceed the grid", b, heads);
    const size_t plane = align_up((size_t)b * t * heads * sizeof(float), 256);
    TRAIN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= 2 * plane, ASTTS_ERR_WORKSPACE,
                  "attn_gqa_bwd: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes, 2 * plane);
    AttnBwdArgs a;
    a.qkv = (const _Float16*)qkv_f16;
    a.dout = (const _Float16*)dout_f16;
    a.lens = lens;
    a.dqkv = (_Float16*)dqkv_f16;
    a.lse = (float*)workspace;
    a.dsum = (float*)((char*)workspace + plane);
    a.ldq = ld_qkv; a.ldo = ld_dout; a.ldg = ld_dqkv;
    a.t = t; a.heads = heads; a.kv_heads = kv_heads;
    a.scale = scale;
    const unsigned tiles = (unsigned)cdiv(t, 128);
    hipLaunchKernelGGL(head_dim == 64 ? attn_bwd_dq<64> : attn_bwd_dq<128>, dim3(tiles, heads, b), dim3(256), 0, (hipStream_t)stream, a);
    TRAIN_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_dim == 64 ? attn_bwd_dkdv<64> : attn_bwd_dkdv<128>, dim3(tiles, kv_heads, b), dim3(256), 0, (hipStream_t)stream, a);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
