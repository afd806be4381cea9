// ops_int8.hip -- LLM.int8 linear layers of the query embedder (gfx950): bitsandbytes' Linear8bitLt at inference
// (has_fp16_weights=False, outlier threshold tau) with an unmerged LoRA branch on top.  DESIGN.md section "LLM.int8 + LoRA" states
// the arithmetic; tests/llm_int8_ref.py restates it in torch and tests/test_llm_int8_gpu.py holds these kernels to it.
//
//   i8_quant_weight     W [N, K] (fp32 or fp16, cast to fp16 first) -> CB int8 [N_pad, K_pad] (K contiguous, zero padded), SCB [N_pad]
//   i8_outlier_mark     per segment: columns with |X| >= tau in some row of the segment -> mask [segments, K], union [K]
//   i8_outlier_compact  union -> ascending column list + its count, both on the device (no host synchronisation)
//   i8_quant_act        X fp16 [M, K] -> CA int8 [M, K_pad] (outlier columns of the row's segment zeroed), SCA [M] and the
//                       compacted outlier activations XO fp16 [M, count] (zero where the column is not the row's segment's)
//   i8_lora_down        T fp32 [M, R] = X . A^T (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums)
//   i8_gemm             y = acc * SCA * SCB / 127^2 (+ bias) + XO . (CB * SCB / 127)[cols]^T + scaling * T . B^T (+ residual)
//                       main loop v_mfma_i32_32x32x32_i8, int32 accumulation; the LoRA term an fp32 MFMA side loop of the
//                       epilogue on the same 32 x 32 tiles, the (few) outlier columns one fma each
#include "common.h"

namespace astts {
namespace {

typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int16v __attribute__((ext_vector_type(16)));

constexpr int kBM = 128, kBN = 128, kBK = 128;     // block tile; kBK in bytes = int8 elements
constexpr int kLdsRow = kBK + 16;                  // LDS row pitch (bytes): 16 B of padding staggers the fragment reads' banks

__device__ __forceinline__ float block_max256(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}

// one row of W per block: SCB = max |fp16(W)|, CB = rint(fp16(W) * (127 / SCB)) (half to even); rows n .. n_pad - 1 are zero
__global__ __launch_bounds__(256) void i8_quant_weight(const void* __restrict__ w, int w_f16, int8_t* __restrict__ cb,
                                                       float* __restrict__ scb, int n, int k, int k_pad) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    int8_t* dst = cb + (int64_t)row * k_pad;
    if (row >= n) {
        for (int i = threadIdx.x; i < k_pad; i += 256) dst[i] = 0;
        if (threadIdx.x == 0) scb[row] = 0.0f;
        return;
    }
    auto ld = [&](int i) -> float {
        return w_f16 ? (float)((const _Float16*)w)[(int64_t)row * k + i] : (float)(_Float16)((const float*)w)[(int64_t)row * k + i];
    };
    float m = 0.0f;
    for (int i = threadIdx.x; i < k; i += 256) m = fmaxf(m, fabsf(ld(i)));
    m = block_max256(m, red);
    const float s = m > 0.0f ? 127.0f / m : 0.0f;
    for (int i = threadIdx.x; i < k_pad; i += 256) dst[i] = i < k ? (int8_t)rintf(ld(i) * s) : (int8_t)0;
    if (threadIdx.x == 0) scb[row] = m;
}

__global__ __launch_bounds__(256) void i8_outlier_mark(const _Float16* __restrict__ x, int64_t ldx, const int* __restrict__ seg, int k,
                                                       float tau, uint8_t* __restrict__ mask, uint8_t* __restrict__ uni) {
    const int row = blockIdx.x;
    const int s = seg[row];
    if (s < 0) return;                              // pad rows belong to no segment
    const _Float16* xr = x + row * ldx;
    for (int i = threadIdx.x; i < k; i += 256)
        if (fabsf((float)xr[i]) >= tau) {           // equal values from several rows: a benign race
            mask[(int64_t)s * k + i] = 1;
            uni[i] = 1;
        }
}

// one block of 1024: the union's columns in ascending order, padded with column 0 up to a multiple of 8 (i8_quant_act writes
// XO = 0 there)
__global__ __launch_bounds__(1024) void i8_outlier_compact(const uint8_t* __restrict__ uni, int k, int* __restrict__ cols, int* __restrict__ cnt) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int base = 0;
    for (int k0 = 0; k0 < k; k0 += 1024) {
        const int i = k0 + threadIdx.x;
        const bool f = i < k && uni[i] != 0;
        const unsigned long long b = __ballot(f);
        const int pre = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int off = base, tot = 0;
        for (int j = 0; j < 16; ++j) {
            off += j < wv ? wsum[j] : 0;
            tot += wsum[j];
        }
        if (f) cols[off + pre] = i;
        __syncthreads();
        base += tot;
    }
    const int b8 = (base + 7) & ~7;
    if ((int)threadIdx.x < b8 - base) cols[base + threadIdx.x] = 0;
    if (threadIdx.x == 0) *cnt = base;
}

// one row per block: SCA = max |x| over the row's elements below tau; CA = 0 on the outlier columns of the row's segment (a pad row:
// on its own elements >= tau), rint(x * (127 / SCA)) elsewhere; XO[row, j] = x[cols[j]] when cols[j] is its segment's, else 0
__global__ __launch_bounds__(256) void i8_quant_act(const _Float16* __restrict__ x, int64_t ldx, const int* __restrict__ seg, int k, int k_pad,
                                                    float tau, const uint8_t* __restrict__ mask, const int* __restrict__ cols,
                                                    const int* __restrict__ cnt, int8_t* __restrict__ ca, float* __restrict__ sca,
                                                    _Float16* __restrict__ xo, int ldo) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    const int s = seg[row];
    const bool dec = tau > 0.0f;
    const _Float16* xr = x + row * ldx;
    float m = 0.0f;
    for (int i = threadIdx.x; i < k; i += 256) {
        const float a = fabsf((float)xr[i]);
        if (!dec || a < tau) m = fmaxf(m, a);
    }
    m = block_max256(m, red);
    const float sc = m > 0.0f ? 127.0f / m : 0.0f;
    const uint8_t* mk = (dec && s >= 0) ? mask + (int64_t)s * k : nullptr;
    int* dst = (int*)(ca + (int64_t)row * k_pad);                       // k_pad % 128 == 0: four bytes per store
    for (int i4 = threadIdx.x; i4 < k_pad / 4; i4 += 256) {
        unsigned packed = 0;
        for (int e = 0; e < 4; ++e) {
            const int i = 4 * i4 + e;
            int q = 0;
            if (i < k) {
                const float v = (float)xr[i];
                const bool out = dec && (mk ? mk[i] != 0 : fabsf(v) >= tau);
                if (!out) q = (int)rintf(v * sc);
            }
            packed |= (unsigned)(q & 0xff) << (8 * e);
        }
        dst[i4] = (int)packed;
    }
    if (threadIdx.x == 0) sca[row] = m;
    const int n = *cnt, n8 = (n + 7) & ~7;
    _Float16* xor_ = xo + (int64_t)row * ldo;
    for (int j = threadIdx.x; j < n8; j += 256) {
        _Float16 v = (_Float16)0.0f;
        if (j < n && mk) {
            const int c = cols[j];
            if (mk[c]) v = xr[c];
        }
        xor_[j] = v;
    }
}

// T[m, r] = sum_k x[m, k] * a[r, k]: a 32 x 32 tile of T per block, the four waves split K and meet in LDS (fixed order).
// On the f32 MFMA the lane half h carries k = 8q + 4h + s in step s of chunk q, in both operands (any common k order is a sum)
template <bool VEC>
__global__ __launch_bounds__(256) void i8_lora_down(const _Float16* __restrict__ x, int64_t ldx, const float* __restrict__ a, int m, int k,
                                                    float* __restrict__ t, int ldt) {
    __shared__ float red[4][16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, h = lane >> 5;
    const int m0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int row = m0 + (lane & 31), arow = r0 + (lane & 31);
    const int kchunk = ((k + 7) / 8 + 3) / 4 * 8;
    const int kb = wv * kchunk, ke = min(k, kb + kchunk);
    const _Float16* xr = x + (int64_t)min(row, m - 1) * ldx;
    const float* ar = a + (int64_t)arow * k;
    const bool rv = row < m;
    float16v acc = {};
    for (int kk = kb; kk < ke; kk += 8) {
        const int k4 = kk + 4 * h;
        float xv[4], av[4];
        if (VEC && kk + 8 <= ke) {
            const half4 hx = *(const half4*)(xr + k4);
            const float4v fa = *(const float4v*)(ar + k4);
            for (int e = 0; e < 4; ++e) {
                xv[e] = rv ? (float)hx[e] : 0.0f;
                av[e] = fa[e];
            }
        } else {
            for (int e = 0; e < 4; ++e) {
                const bool in = k4 + e < ke;
                xv[e] = (in && rv) ? (float)xr[k4 + e] : 0.0f;
                av[e] = in ? ar[k4 + e] : 0.0f;
            }
        }
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[e], av[e], acc, 0, 0, 0);
    }
    for (int e = 0; e < 16; ++e) red[wv][e][lane] = acc[e];
    __syncthreads();
    if (wv != 0) return;
    for (int e = 0; e < 16; ++e) {
        const float v = ((red[0][e][lane] + red[1][e][lane]) + red[2][e][lane]) + red[3][e][lane];
        const int orow = m0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (orow < m) t[(int64_t)orow * ldt + r0 + (lane & 31)] = v;
    }
}

struct I8GemmArgs {
    const int8_t* a;      // CA [m, k_pad]
    const float* sca;     // [m]
    const int8_t* b;      // CB [n_pad, k_pad]
    const float* scb;     // [n_pad]
    const _Float16* xo;   // outlier activations [m, ldo] or null
    const int* cols;      // [>= count rounded up to 8]
    const int* cnt;       // device count
    const float* t;       // LoRA down-projection [m, ldt] or null
    const float* lb;      // LoRA B [n_pad, r] (r % 8 == 0)
    const float* bias;    // fp32 [n] or null
    const float* res;     // fp32 residual [m, ldr] or null
    void* out;
    int64_t ldr, ldc;
    int m, n, k_pad, ldo, ldt, r, g1, g2, out_kind;   // out_kind 0 fp32, 1 fp16, 2 the raw int32 accumulator
    float scaling;
};

__global__ __launch_bounds__(256) void i8_gemm(I8GemmArgs p) {
    __shared__ __attribute__((aligned(16))) int8_t lds_a[kBM * kLdsRow];
    __shared__ __attribute__((aligned(16))) int8_t lds_b[kBN * kLdsRow];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 5;
    const int wm = wv >> 1, wn = wv & 1;
    const int nbn = (p.n + kBN - 1) / kBN;
    const int m0 = (blockIdx.x / nbn) * kBM, n0 = (blockIdx.x % nbn) * kBN;

    // global -> LDS staging: 1024 chunks of 16 B per operand tile, four per thread (row = c >> 3, byte = 16 (c & 7))
    int4v ra[4], rb[4];
    auto fetch = [&](int kt) {
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, cb = (c & 7) * 16;
            const int gm = m0 + row;
            ra[i] = gm < p.m ? *(const int4v*)(p.a + (int64_t)gm * p.k_pad + kt + cb) : int4v{0, 0, 0, 0};
            rb[i] = *(const int4v*)(p.b + (int64_t)(n0 + row) * p.k_pad + kt + cb);   // n0 + row < n_pad
        }
    };
    int16v acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = int16v{};
    fetch(0);
    for (int kt = 0; kt < p.k_pad; kt += kBK) {
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, cb = (c & 7) * 16;
            *(int4v*)(lds_a + row * kLdsRow + cb) = ra[i];
            *(int4v*)(lds_b + row * kLdsRow + cb) = rb[i];
        }
        __syncthreads();
        if (kt + kBK < p.k_pad) fetch(kt + kBK);
        for (int kk = 0; kk < kBK; kk += 32) {
            int4v fa[2], fb[2];
            for (int i = 0; i < 2; ++i) {
                fa[i] = *(const int4v*)(lds_a + (wm * 64 + i * 32 + (lane & 31)) * kLdsRow + kk + 16 * h);
                fb[i] = *(const int4v*)(lds_b + (wn * 64 + i * 32 + (lane & 31)) * kLdsRow + kk + 16 * h);
            }
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    const int n_out = (p.xo && p.cols && p.cnt) ? *p.cnt : 0;
    for (int i = 0; i < 2; ++i) {
        const int mt = m0 + wm * 64 + i * 32;
        if (mt >= p.m) continue;
        const int arow = mt + (lane & 31);
        const bool arow_ok = arow < p.m;
        for (int j = 0; j < 2; ++j) {
            const int nt = n0 + wn * 64 + j * 32;
            if (nt >= p.n) continue;
            const int col = nt + (lane & 31);                       // < n_pad
            const float sb = p.scb[col];
            const float bv = (p.bias && col < p.n) ? p.bias[col] : 0.0f;      // bias has n entries, col runs to n_pad
            float16v side = {}, lora = {};
            if (n_out > 0) {                                         // outlier columns against the dequantised int8 weight: one fma
                const int8_t* cbr = p.b + (int64_t)col * p.k_pad;    // per column in list order, so a column of another segment
                for (int q = 0; q < n_out; ++q) {                    // (x = 0) leaves a row's sum bit-identical: batch-invariant
                    const float wq = (float)cbr[p.cols[q]] * sb / 127.0f;
                    for (int e = 0; e < 16; ++e) {
                        const int row = mt + (e & 3) + 8 * (e >> 2) + 4 * h;
                        const float xv = row < p.m ? (float)p.xo[(int64_t)row * p.ldo + q] : 0.0f;
                        side[e] = fmaf(xv, wq, side[e]);
                    }
                }
            }
            if (p.r > 0 && p.t) {                                    // LoRA up-projection on the fp32 T of i8_lora_down
                const int toff = ((nt >= p.g1) + (nt >= p.g2)) * p.r;
                const float* tr = p.t + (int64_t)arow * p.ldt + toff;
                const float* br = p.lb + (int64_t)col * p.r;
                for (int q = 0; q < p.r; q += 8) {
                    const float4v tv = arow_ok ? *(const float4v*)(tr + q + 4 * h) : float4v{};
                    const float4v bv = *(const float4v*)(br + q + 4 * h);
                    for (int e = 0; e < 4; ++e) lora = __builtin_amdgcn_mfma_f32_32x32x2f32(tv[e], bv[e], lora, 0, 0, 0);
                }
            }
            if (col >= p.n) continue;
            for (int e = 0; e < 16; ++e) {
                const int row = mt + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (row >= p.m) continue;
                if (p.out_kind == 2) {
                    ((int*)p.out)[row * p.ldc + col] = acc[i][j][e];
                    continue;
                }
                float v = (float)acc[i][j][e] * p.sca[row] * sb / 16129.0f;
                if (p.bias) v = v + bv;                              // fp32, next to the dequantised accumulator
                v = v + side[e];
                v = v + p.scaling * lora[e];
                if (p.res) v += p.res[row * p.ldr + col];
                if (p.out_kind == 1)
                    ((_Float16*)p.out)[row * p.ldc + col] = (_Float16)v;
                else
                    ((float*)p.out)[row * p.ldc + col] = v;
            }
        }
    }
}

}  // namespace
}  // namespace astts

using namespace astts;

extern "C" {

int astts_op_i8_quant_weight(const void* w, int32_t w_f16, int8_t* cb, float* scb, int32_t n, int32_t k, int32_t n_pad, int32_t k_pad,
                             astts_stream_t stream) {
    ASTTS_REQUIRE(w && cb && scb, ASTTS_ERR_INVALID, "astts_op_i8_quant_weight: null pointer");
    ASTTS_REQUIRE(n >= 1 && k >= 1 && n_pad >= n && n_pad % kBN == 0 && k_pad >= k && k_pad % kBK == 0, ASTTS_ERR_INVALID,
                  "astts_op_i8_quant_weight: bad shape n=%d k=%d n_pad=%d k_pad=%d", n, k, n_pad, k_pad);
    hipLaunchKernelGGL(i8_quant_weight, dim3((unsigned)n_pad), dim3(256), 0, (hipStream_t)stream, w, w_f16, cb, scb, n, k, k_pad);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

size_t astts_op_i8_quant_act_workspace_bytes(int32_t segments, int32_t k) {
    return align_up((size_t)(segments > 0 ? segments : 0) * (size_t)k, 256) + align_up((size_t)k, 256);
}

int astts_op_i8_quant_act(const void* x_f16, int64_t ldx, const int32_t* seg, int32_t m, int32_t k, int32_t k_pad, int32_t segments,
                          float tau, int8_t* ca, float* sca, void* xo_f16, int32_t ldo, int32_t* cols, int32_t* cnt, void* workspace,
                          size_t workspace_bytes, astts_stream_t stream) {
    ASTTS_REQUIRE(x_f16 && seg && ca && sca && xo_f16 && cols && cnt, ASTTS_ERR_INVALID, "astts_op_i8_quant_act: null pointer");
    ASTTS_REQUIRE(m >= 1 && k >= 1 && ldx >= k && k_pad >= k && k_pad % kBK == 0 && ldo >= k_pad && ldo % 4 == 0 && segments >= 1,
                  ASTTS_ERR_INVALID, "astts_op_i8_quant_act: bad shape m=%d k=%d k_pad=%d ldo=%d segments=%d", m, k, k_pad, ldo, segments);
    const hipStream_t st = (hipStream_t)stream;
    if (tau > 0.0f) {
        ASTTS_REQUIRE(workspace && workspace_bytes >= astts_op_i8_quant_act_workspace_bytes(segments, k), ASTTS_ERR_INVALID,
                      "astts_op_i8_quant_act: workspace too small");
        uint8_t* mask = (uint8_t*)workspace;
        uint8_t* uni = mask + align_up((size_t)segments * k, 256);
        ASTTS_CHECK_HIP(hipMemsetAsync(workspace, 0, astts_op_i8_quant_act_workspace_bytes(segments, k), st));
        hipLaunchKernelGGL(i8_outlier_mark, dim3((unsigned)m), dim3(256), 0, st, (const _Float16*)x_f16, ldx, seg, k, tau, mask, uni);
        ASTTS_CHECK_LAUNCH();
        hipLaunchKernelGGL(i8_outlier_compact, dim3(1), dim3(1024), 0, st, (const uint8_t*)uni, k, cols, cnt);
        ASTTS_CHECK_LAUNCH();
        hipLaunchKernelGGL(i8_quant_act, dim3((unsigned)m), dim3(256), 0, st, (const _Float16*)x_f16, ldx, seg, k, k_pad, tau,
                           (const uint8_t*)mask, (const int*)cols, (const int*)cnt, ca, sca, (_Float16*)xo_f16, ldo);
    } else {                                                          // no decomposition: an empty outlier list
        ASTTS_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t), st));
        hipLaunchKernelGGL(i8_quant_act, dim3((unsigned)m), dim3(256), 0, st, (const _Float16*)x_f16, ldx, seg, k, k_pad, tau,
                           (const uint8_t*)nullptr, (const int*)cols, (const int*)cnt, ca, sca, (_Float16*)xo_f16, ldo);
    }
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_op_i8_lora_down(const void* x_f16, int64_t ldx, const float* a, int32_t m, int32_t k, int32_t r_tot, float* t, int32_t ldt,
                          astts_stream_t stream) {
    ASTTS_REQUIRE(x_f16 && a && t, ASTTS_ERR_INVALID, "astts_op_i8_lora_down: null pointer");
    ASTTS_REQUIRE(m >= 1 && k >= 1 && ldx >= k && r_tot >= 32 && r_tot % 32 == 0 && ldt >= r_tot, ASTTS_ERR_INVALID,
                  "astts_op_i8_lora_down: bad shape m=%d k=%d r=%d ldt=%d", m, k, r_tot, ldt);
    const dim3 grid((unsigned)cdiv(m, 32), (unsigned)(r_tot / 32));
    const bool vec = ldx % 4 == 0 && k % 4 == 0 && ((uintptr_t)x_f16 & 7) == 0 && ((uintptr_t)a & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(i8_lora_down<true>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)x_f16, ldx, a, m, k, t, ldt);
    else
        hipLaunchKernelGGL(i8_lora_down<false>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)x_f16, ldx, a, m, k, t, ldt);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_op_i8_gemm(const int8_t* ca, const float* sca, const int8_t* cb, const float* scb, int32_t m, int32_t n, int32_t k_pad,
                     const void* xo_f16, int32_t ldo, const int32_t* cols, const int32_t* cnt, const float* t, int32_t ldt,
                     const float* lora_b, int32_t r, int32_t g1, int32_t g2, float scaling, const float* bias, const float* residual,
                     int64_t ldr, void* out, int32_t out_kind, int64_t ldc, astts_stream_t stream) {
    ASTTS_REQUIRE(ca && sca && cb && scb && out, ASTTS_ERR_INVALID, "astts_op_i8_gemm: null pointer");
    ASTTS_REQUIRE(m >= 1 && n >= 1 && k_pad >= kBK && k_pad % kBK == 0 && ldc >= n && out_kind >= 0 && out_kind <= 2 &&
                      (!residual || ldr >= n),
                  ASTTS_ERR_INVALID, "astts_op_i8_gemm: bad shape m=%d n=%d k_pad=%d", m, n, k_pad);
    ASTTS_REQUIRE(!xo_f16 || (cols && cnt && ldo >= 8 && ldo % 4 == 0 && ((uintptr_t)xo_f16 & 7) == 0 && ((uintptr_t)cols & 15) == 0),
                  ASTTS_ERR_INVALID, "astts_op_i8_gemm: bad outlier operands");
    ASTTS_REQUIRE(r == 0 || (t && lora_b && r % 8 == 0 && ldt % 4 == 0 && g1 % 32 == 0 && g2 % 32 == 0 && ((uintptr_t)t & 15) == 0 &&
                             ((uintptr_t)lora_b & 15) == 0),
                  ASTTS_ERR_INVALID, "astts_op_i8_gemm: bad LoRA operands (r=%d, ldt=%d, group bounds %d %d)", r, ldt, g1, g2);
    I8GemmArgs p{ca, sca, cb, scb, (const _Float16*)xo_f16, cols, cnt, t, lora_b, bias, residual, out, ldr, ldc,
                 m, n, k_pad, ldo, ldt, r, g1, g2, out_kind, scaling};
    const int64_t blocks = cdiv(m, kBM) * cdiv(n, kBN);
    ASTTS_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "astts_op_i8_gemm: grid too large");
    hipLaunchKernelGGL(i8_gemm, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
