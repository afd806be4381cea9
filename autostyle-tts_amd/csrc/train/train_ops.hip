// train_ops.hip -- libastts_train.so: the row-wise backward kernels (RMSNorm, SwiGLU, cross-entropy), the LoRA weight gradient
// (a "TN" GEMM on the matrix cores) and the optimizer (sum of squares, AdamW).  No float atomics: see include/train/astts_train.h.
#include <algorithm>
#include <cstdarg>

#include "philox.h"
#include "train_common.h"
#include "../qknorm_lane.h"

namespace astts_train {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// sum over the 256 threads of a block in a fixed order (xor butterfly inside a wave, then the four waves in order); every thread
// gets the result.  `red`: 4 slots of LDS, free to reuse after the call's second barrier
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                 // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- RMSNorm backward: one workgroup per row.  With g = dy * w and r = rsqrt(mean(x^2) + eps):  dx = r g - x r^3 mean(g x)
__global__ __launch_bounds__(256) void rmsnorm_bwd_rows(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                                        float* __restrict__ dres, int c, float eps) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    const float* xr = x + row * c;
    const float* gr = dy + row * c;
    float ss = 0.0f, sg = 0.0f;
    for (int i = threadIdx.x; i < c; i += 256) {
        const float xv = xr[i];
        ss += xv * xv;
        sg += gr[i] * w[i] * xv;
    }
    ss = block_sum(ss, red);
    sg = block_sum(sg, red);
    const float r = 1.0f / sqrtf(ss / (float)c + eps);
    const float k = r * r * r * sg / (float)c;
    float* dr = dres + row * c;
    for (int i = threadIdx.x; i < c; i += 256) dr[i] += r * gr[i] * w[i] - xr[i] * k;
}

// ---- SwiGLU backward: out = silu(g) u  ->  dg = dout u s (1 + g (1 - s)),  du = dout g s,  s = sigmoid(g)
__global__ __launch_bounds__(256) void swiglu_bwd_rows(const _Float16* __restrict__ dout, const _Float16* __restrict__ gu,
                                                       _Float16* __restrict__ dgu, int64_t rows, int f) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * f) return;
    const int64_t row = i / f;
    const int col = (int)(i - row * f);
    const float g = (float)gu[row * 2 * f + col], u = (float)gu[row * 2 * f + f + col], d = (float)dout[i];
    const float s = 1.0f / (1.0f + __expf(-g));
    dgu[row * 2 * f + col] = (_Float16)(d * u * s * (1.0f + g * (1.0f - s)));
    dgu[row * 2 * f + f + col] = (_Float16)(d * g * s);
}

// ---- cross-entropy gradient, in place on the logits: one workgroup per row
__global__ __launch_bounds__(256) void xent_grad_rows(float* __restrict__ logits, int64_t ld, const float* __restrict__ lse,
                                                      const int* __restrict__ targets, int vocab, float scale) {
    const int64_t row = blockIdx.x;
    float* lr = logits + row * ld;
    const int tg = targets[row];
    if (tg < 0) {
        for (int i = threadIdx.x; i < vocab; i += 256) lr[i] = 0.0f;
        return;
    }
    const float l = lse[row];
    for (int i = threadIdx.x; i < vocab; i += 256) lr[i] = (__expf(lr[i] - l) - (i == tg ? 1.0f : 0.0f)) * scale;
}

// ---- LoRA weight gradient: G[n, k] = sum_row U[row, n] X[row, k].  One wave per (32 n, 32 k, row slab): G^T's tile is
// D[M = n][N = k] = U^T (A operand: M = n on the lane, the 16 rows of a step along K) X (B operand: N = k on the lane); both operands
// are read from global memory column-wise (32 consecutive columns per row: 64-byte segments).  One of n, k is the LoRA rank.
static constexpr int LG_ROWS = 256;   // rows per slab

template <bool UF32>
__global__ __launch_bounds__(64) void lora_grad_partial(const void* __restrict__ u_, int64_t ldu, const _Float16* __restrict__ x, int64_t ldx,
                                                        float* __restrict__ part, int64_t rows, int n, int k) {
    const int lane = threadIdx.x, c = lane & 31, hh = lane >> 5;
    const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int64_t r0 = (int64_t)blockIdx.z * LG_ROWS, r1 = min(rows, r0 + (int64_t)LG_ROWS);
    const int nn = n0 + c, kk = k0 + c;
    float16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    for (int64_t r = r0; r < r1; r += 16) {
        half8 af, bf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t row = r + 8 * hh + j;
            const bool ok = row < r1;
            _Float16 a = (_Float16)0.0f, b = (_Float16)0.0f;
            if (ok && nn < n) a = UF32 ? (_Float16) reinterpret_cast<const float*>(u_)[row * ldu + nn] : reinterpret_cast<const _Float16*>(u_)[row * ldu + nn];
            if (ok && kk < k) b = x[row * ldx + kk];
            af[j] = a;
            bf[j] = b;
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
    }
    if (kk < k) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ni = n0 + mfma_row(e, hh);
            if (ni < n) part[((int64_t)blockIdx.z * n + ni) * k + kk] = acc[e];
        }
    }
}

// The same product with LoRA dropout's masks regenerated on X as it is read (philox.h): G row n belongs to part n / r and sees X
// under that part's mask.  A lane holds one column of X over 8 rows, a dropout group is 8 columns of one row: the 8 lanes that share
// a group column each draw one row's group and hand the bits round.  A tile that spans several parts (r < 32) takes one MFMA per
// part, U's other columns zeroed.  Same slabs, same planes, same merge.
template <bool UF32>
__global__ __launch_bounds__(64) void lora_grad_dropout_partial(const void* __restrict__ u_, int64_t ldu, const _Float16* __restrict__ x, int64_t ldx,
                                                                float* __restrict__ part, int64_t rows, int n, int k, int r, uint32_t stream,
                                                                drop_key key) {
    const int lane = threadIdx.x, c = lane & 31, hh = lane >> 5;
    const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    const int64_t r0 = (int64_t)blockIdx.z * LG_ROWS, r1 = min(rows, r0 + (int64_t)LG_ROWS);
    const int nn = n0 + c, kk = k0 + c;
    const int j0 = n0 / r, j1 = (min(n, n0 + 32) - 1) / r;                    // the parts this tile has rows of
    float16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    for (int64_t rr = r0; rr < r1; rr += 16) {
        half8 af, bf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t row = rr + 8 * hh + j;
            const bool ok = row < r1;
            _Float16 a = (_Float16)0.0f, b = (_Float16)0.0f;
            if (ok && nn < n) a = UF32 ? (_Float16) reinterpret_cast<const float*>(u_)[row * ldu + nn] : reinterpret_cast<const _Float16*>(u_)[row * ldu + nn];
            if (ok && kk < k) b = x[row * ldx + kk];
            af[j] = a;
            bf[j] = b;
        }
        const uint64_t group = ((uint64_t)(rr + 8 * hh + (c & 7)) * (uint64_t)k + (uint64_t)(k0 + (c & ~7))) >> 3;
        for (int jp = j0; jp <= j1; ++jp) {
            half8 am, bm;
            const uint32_t mine = key.thr ? dropout_keep_bits(key, group, stream + jp) : 0xFFu;
            const bool in_part = nn >= jp * r && nn < (jp + 1) * r;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t bits = __shfl(mine, (lane & ~7) | j, 64);
                bm[j] = (bits >> (c & 7) & 1u) ? bf[j] : (_Float16)0.0f;
                am[j] = in_part ? af[j] : (_Float16)0.0f;
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(am, bm, acc, 0, 0, 0);
        }
    }
    if (kk < k) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ni = n0 + mfma_row(e, hh);
            if (ni < n) part[((int64_t)blockIdx.z * n + ni) * k + kk] = acc[e];
        }
    }
}

__global__ __launch_bounds__(256) void lora_grad_merge(const float* __restrict__ part, float* __restrict__ g, int64_t ldg, int n, int k, int slabs,
                                                       float alpha, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * k) return;
    float s = 0.0f;
    for (int z = 0; z < slabs; ++z) s += part[(int64_t)z * n * k + i];      // slab order
    const int64_t o = (i / k) * ldg + (i % k);
    g[o] = accumulate ? g[o] + alpha * s : alpha * s;
}

// ---- sum of squares: stage 1, SS_BLOCKS(n) workgroups each over a fixed strided set of elements; stage 2, one workgroup
static inline int ss_blocks(int64_t n) { return (int)std::min<int64_t>(1024, std::max<int64_t>(1, cdiv(n, 4096))); }

__global__ __launch_bounds__(256) void sumsq_stage1(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = (double)x[i];
        s += v * v;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void sumsq_stage2(const double* __restrict__ part, int nblk, float* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = (float)s;
}

__global__ __launch_bounds__(256) void adamw_step(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                  int64_t n, float lr_wd, float omb1, float beta2, float omb2, float eps, float step_size,
                                                  float bc2_sqrt, float grad_mul) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gr = g[i] * grad_mul;
    float pv = p[i] * (1.0f - lr_wd);
    const float mv = m[i] + omb1 * (gr - m[i]);
    const float vv = beta2 * v[i] + omb2 * gr * gr;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    pv -= step_size * (mv / denom);
    p[i] = pv;
    m[i] = mv;
    v[i] = vv;
}

// ---- Qwen3 q / k norm + RoPE backward (forward: ../ops_qknorm.hip, lane layout: ../qknorm_lane.h).  In place on the q | k part of dqkv:
// dy -> the rotation's transpose -> g = w o that; with r and xh = x r recomputed from the kept pre-norm head:  dx = r (g - xh mean(g xh)).
// xh never comes from the saved output divided by w: w has zeros.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rope_bwd(_Float16* __restrict__ dqkv, int64_t ldd, const _Float16* __restrict__ xpre, int64_t ldx,
                                                       const float* __restrict__ cs, const float* __restrict__ sn, const float* __restrict__ qw,
                                                       const float* __restrict__ kw, int64_t units, int t, int heads, int hall, int pos0, float eps) {
    using namespace astts;
    constexpr int HALF = HD / 2, LPH = HD / 16;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int sub = (int)(tid & (LPH - 1));
    const int64_t unit = tid / LPH;
    const bool live = unit < units;
    const int64_t u = live ? unit : units - 1;          // the spare lanes repeat the last head and store nothing: full waves for xlane.h
    const int64_t row = u / hall;
    const int hd = (int)(u - row * hall);
    const int pos = pos0 + (int)(row % t);

    _Float16* dp = dqkv + row * ldd + hd * HD + sub * 8;
    const QknLane d = qkn_load_f16(dp, HALF);
    const QknLane x = qkn_load_f16(xpre + row * ldx + hd * HD + sub * 8, HALF);
    float wa[8], wb[8], c[8], s[8];
    const float* w = (hd < heads ? qw : kw) + sub * 8;
    qkn_load8_f32(w, wa);
    qkn_load8_f32(w + HALF, wb);
    qkn_load8_f32(cs + (int64_t)pos * HALF + sub * 8, c);
    qkn_load8_f32(sn + (int64_t)pos * HALF + sub * 8, s);

    const float r = qkn_rstd<LPH>(x, eps);
    QknLane g, xh;
    float dot = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        g.a[e] = wa[e] * (d.a[e] * c[e] + d.b[e] * s[e]);
        g.b[e] = wb[e] * (d.b[e] * c[e] - d.a[e] * s[e]);
        xh.a[e] = x.a[e] * r;
        xh.b[e] = x.b[e] * r;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(g.a[e], xh.a[e], dot);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot = fmaf(g.b[e], xh.b[e], dot);
    const float m = qkn_group_sum<LPH>(dot) * (1.0f / (float)HD);
    QknLane o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o.a[e] = r * (g.a[e] - xh.a[e] * m);
        o.b[e] = r * (g.b[e] - xh.b[e] * m);
    }
    if (live) qkn_store_f16(dp, HALF, o);
}

}  // namespace astts_train

using namespace astts_train;

extern "C" {

int32_t astts_train_abi_version(void) { return ASTTS_TRAIN_ABI_VERSION; }

const char* astts_train_last_error_string(void) { return astts_train::g_err; }

int astts_train_rmsnorm_bwd(const float* dy, const float* x, const float* w, float* dres, int64_t rows, int32_t c, float eps,
                            astts_stream_t stream) {
    TRAIN_REQUIRE(dy && x && w && dres && rows >= 0 && c > 0, ASTTS_ERR_INVALID, "rmsnorm_bwd: bad arguments");
    TRAIN_REQUIRE(rows < (1ll << 31), ASTTS_ERR_INVALID, "rmsnorm_bwd: %lld rows exceed the grid", (long long)rows);
    if (rows == 0) return ASTTS_OK;
    hipLaunchKernelGGL(rmsnorm_bwd_rows, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, dy, x, w, dres, c, eps);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_swiglu_bwd(const void* dout_f16, const void* gate_up_f16, void* dgate_up_f16, int64_t rows, int32_t f,
                           astts_stream_t stream) {
    TRAIN_REQUIRE(dout_f16 && gate_up_f16 && dgate_up_f16 && rows >= 0 && f > 0, ASTTS_ERR_INVALID, "swiglu_bwd: bad arguments");
    const int64_t blocks = cdiv(rows * f, 256);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "swiglu_bwd: %lld elements exceed the grid", (long long)(rows * f));
    if (blocks == 0) return ASTTS_OK;
    hipLaunchKernelGGL(swiglu_bwd_rows, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16*)dout_f16,
                       (const _Float16*)gate_up_f16, (_Float16*)dgate_up_f16, rows, f);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_xent_grad(float* logits, int64_t ld, const float* lse, const int32_t* targets, int64_t rows, int32_t vocab,
                          float scale, astts_stream_t stream) {
    TRAIN_REQUIRE(logits && lse && targets && rows >= 0 && vocab > 0 && ld >= vocab, ASTTS_ERR_INVALID, "xent_grad: bad arguments");
    TRAIN_REQUIRE(rows < (1ll << 31), ASTTS_ERR_INVALID, "xent_grad: %lld rows exceed the grid", (long long)rows);
    if (rows == 0) return ASTTS_OK;
    hipLaunchKernelGGL(xent_grad_rows, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, ld, lse, targets, vocab, scale);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int32_t astts_train_lora_grad_row_split(void) { return LG_ROWS; }

size_t astts_train_lora_grad_workspace_bytes(int64_t rows, int32_t n, int32_t k) {
    if (rows <= 0 || n <= 0 || k <= 0) return 0;
    return (size_t)cdiv(rows, LG_ROWS) * (size_t)n * (size_t)k * sizeof(float);
}

int astts_train_lora_grad(const void* u, int32_t u_f32, int64_t ldu, const void* x_f16, int64_t ldx, float* g, int64_t ldg,
                          int64_t rows, int32_t n, int32_t k, float alpha, int32_t accumulate, void* workspace,
                          size_t workspace_bytes, astts_stream_t stream) {
    TRAIN_REQUIRE(u && x_f16 && g && rows > 0 && n > 0 && k > 0 && ldu >= n && ldx >= k && ldg >= k, ASTTS_ERR_INVALID,
                  "lora_grad: bad arguments (rows %lld n %d k %d ldu %lld ldx %lld ldg %lld)", (long long)rows, n, k, (long long)ldu,
                  (long long)ldx, (long long)ldg);
    const int64_t slabs = cdiv(rows, LG_ROWS);
    TRAIN_REQUIRE(slabs <= 65535 && cdiv(k, 32) <= 65535, ASTTS_ERR_INVALID, "lora_grad: %lld rows / k %d exceed the grid", (long long)rows, k);
    TRAIN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= astts_train_lora_grad_workspace_bytes(rows, n, k),
                  ASTTS_ERR_WORKSPACE, "lora_grad: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes,
                  astts_train_lora_grad_workspace_bytes(rows, n, k));
    const dim3 grid((unsigned)cdiv(n, 32), (unsigned)cdiv(k, 32), (unsigned)slabs);
    float* part = (float*)workspace;
    if (u_f32)
        hipLaunchKernelGGL(lora_grad_partial<true>, grid, dim3(64), 0, (hipStream_t)stream, u, ldu, (const _Float16*)x_f16, ldx, part, rows, n, k);
    else
        hipLaunchKernelGGL(lora_grad_partial<false>, grid, dim3(64), 0, (hipStream_t)stream, u, ldu, (const _Float16*)x_f16, ldx, part, rows, n, k);
    TRAIN_CHECK_LAUNCH();
    hipLaunchKernelGGL(lora_grad_merge, dim3((unsigned)cdiv((int64_t)n * k, 256)), dim3(256), 0, (hipStream_t)stream, part, g, ldg, n, k,
                       (int)slabs, alpha, accumulate);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_lora_grad_dropout(const void* u, int32_t u_f32, int64_t ldu, const void* x_f16, int64_t ldx, float* g, int64_t ldg,
                                  int64_t rows, int32_t parts, int32_t r, int32_t cin, float alpha, int32_t accumulate, double p,
                                  int64_t seed, uint32_t rng_stream, uint32_t draw, void* workspace, size_t workspace_bytes,
                                  astts_stream_t stream) {
    TRAIN_REQUIRE(u && x_f16 && g && rows > 0 && cin > 0 && cin % 8 == 0 && parts >= 1 && parts <= 3 && r >= 8 && r <= 64 && r % 8 == 0,
                  ASTTS_ERR_INVALID, "lora_grad_dropout: bad arguments (rows %lld cin %d: a multiple of 8; parts %d in 1..3; r %d: a multiple of 8 up to 64)",
                  (long long)rows, cin, parts, r);
    const int n = parts * r, k = cin;
    TRAIN_REQUIRE(ldu >= n && ldx >= k && ldg >= k, ASTTS_ERR_INVALID, "lora_grad_dropout: row strides (ldu %lld ldx %lld ldg %lld) must cover the rows",
                  (long long)ldu, (long long)ldx, (long long)ldg);
    TRAIN_REQUIRE(p >= 0.0 && p < 1.0, ASTTS_ERR_INVALID, "lora_grad_dropout: p = %g is outside [0, 1)", p);
    const int64_t slabs = cdiv(rows, LG_ROWS);
    TRAIN_REQUIRE(slabs <= 65535 && cdiv(k, 32) <= 65535, ASTTS_ERR_INVALID, "lora_grad_dropout: %lld rows / cin %d exceed the grid", (long long)rows, k);
    TRAIN_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= astts_train_lora_grad_workspace_bytes(rows, n, k),
                  ASTTS_ERR_WORKSPACE, "lora_grad_dropout: workspace of %zu bytes, %zu needed (16-byte aligned)", workspace_bytes,
                  astts_train_lora_grad_workspace_bytes(rows, n, k));
    drop_key key;
    key.seed_lo = (uint32_t)(uint64_t)seed, key.seed_hi = (uint32_t)((uint64_t)seed >> 32), key.draw = draw, key.thr = (uint32_t)(p * 65536.0);
    const dim3 grid((unsigned)cdiv(n, 32), (unsigned)cdiv(k, 32), (unsigned)slabs);
    float* part = (float*)workspace;
    if (u_f32)
        hipLaunchKernelGGL(lora_grad_dropout_partial<true>, grid, dim3(64), 0, (hipStream_t)stream, u, ldu, (const _Float16*)x_f16, ldx, part, rows, n, k,
                           r, rng_stream, key);
    else
        hipLaunchKernelGGL(lora_grad_dropout_partial<false>, grid, dim3(64), 0, (hipStream_t)stream, u, ldu, (const _Float16*)x_f16, ldx, part, rows, n, k,
                           r, rng_stream, key);
    TRAIN_CHECK_LAUNCH();
    hipLaunchKernelGGL(lora_grad_merge, dim3((unsigned)cdiv((int64_t)n * k, 256)), dim3(256), 0, (hipStream_t)stream, part, g, ldg, n, k,
                       (int)slabs, (float)((double)alpha / (1.0 - p)), accumulate);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

size_t astts_train_sumsq_workspace_bytes(int64_t n) { return (size_t)ss_blocks(n) * sizeof(double); }

int astts_train_sumsq(const float* x, int64_t n, float* out, void* workspace, size_t workspace_bytes, astts_stream_t stream) {
    TRAIN_REQUIRE(x && out && n > 0, ASTTS_ERR_INVALID, "sumsq: bad arguments");
    TRAIN_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= astts_train_sumsq_workspace_bytes(n), ASTTS_ERR_WORKSPACE,
                  "sumsq: workspace of %zu bytes, %zu needed (8-byte aligned)", workspace_bytes, astts_train_sumsq_workspace_bytes(n));
    const int nblk = ss_blocks(n);
    hipLaunchKernelGGL(sumsq_stage1, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, n, (double*)workspace);
    TRAIN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sumsq_stage2, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, nblk, out);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_adamw(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                      double weight_decay, double bias_corr1, double bias_corr2, double grad_mul, astts_stream_t stream) {
    TRAIN_REQUIRE(p && g && m && v && n > 0, ASTTS_ERR_INVALID, "adamw: bad arguments");
    TRAIN_REQUIRE(bias_corr1 > 0.0 && bias_corr2 > 0.0, ASTTS_ERR_INVALID, "adamw: bias corrections must be positive (step >= 1)");
    const int64_t blocks = cdiv(n, 256);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "adamw: %lld elements exceed the grid", (long long)n);
    hipLaunchKernelGGL(adamw_step, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)(lr * weight_decay), (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(lr / bias_corr1), (float)sqrt(bias_corr2), (float)grad_mul);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

int astts_train_qknorm_rope_bwd(void* dqkv_f16, int64_t ld_dqkv, const void* x_pre_f16, int64_t ld_x, const float* cos_tab,
                                const float* sin_tab, const float* q_norm_w, const float* k_norm_w, int32_t b, int32_t t, int32_t heads,
                                int32_t kv_heads, int32_t head_dim, int32_t pos0, float eps, astts_stream_t stream) {
    TRAIN_REQUIRE(dqkv_f16 && x_pre_f16 && cos_tab && sin_tab && q_norm_w && k_norm_w, ASTTS_ERR_INVALID, "qknorm_rope_bwd: null pointer");
    TRAIN_REQUIRE(head_dim == 64 || head_dim == 128, ASTTS_ERR_UNSUPPORTED, "qknorm_rope_bwd: head_dim=%d (built for 64 and 128)", head_dim);
    const int64_t wqk = (int64_t)(heads + kv_heads) * head_dim;
    TRAIN_REQUIRE(b >= 1 && t >= 1 && heads >= 1 && kv_heads >= 1 && pos0 >= 0 && ld_dqkv >= wqk && ld_x >= wqk && (ld_dqkv & 7) == 0 &&
                      (ld_x & 7) == 0 && eps >= 0.0f,
                  ASTTS_ERR_INVALID, "qknorm_rope_bwd: bad shape b=%d t=%d heads=%d kv_heads=%d head_dim=%d ld_dqkv=%lld ld_x=%lld", b, t, heads,
                  kv_heads, head_dim, (long long)ld_dqkv, (long long)ld_x);
    TRAIN_REQUIRE((((uintptr_t)dqkv_f16 | (uintptr_t)x_pre_f16 | (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)q_norm_w |
                    (uintptr_t)k_norm_w) & 15) == 0,
                  ASTTS_ERR_INVALID, "qknorm_rope_bwd: the planes, the tables and the norm weights must be 16-byte aligned");
    const int64_t units = (int64_t)b * t * (heads + kv_heads);
    const int64_t blocks = cdiv(units * (head_dim / 16), 256);
    TRAIN_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "qknorm_rope_bwd: %lld heads exceed the grid", (long long)units);
    const auto kern = head_dim == 64 ? qknorm_rope_bwd<64> : qknorm_rope_bwd<128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (_Float16*)dqkv_f16, ld_dqkv, (const _Float16*)x_pre_f16,
                       ld_x, cos_tab, sin_tab, q_norm_w, k_norm_w, units, t, heads, heads + kv_heads, pos0, eps);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
