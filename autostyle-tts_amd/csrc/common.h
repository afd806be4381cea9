// common.h -- shared host-side helpers for libastts.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>

#include "../../include/astts.h"

namespace astts {

void set_error(const char* fmt, ...);

// bench-only launch profiler (runtime.hip); prof_begin returns true when the launch is being timed
bool prof_begin(int kind, hipStream_t st, double work);
void prof_end(int kind, hipStream_t st);
// kernel-level variant: a reserved (start, stop) pair for hipExtLaunchKernelGGL; false when the kind is not being profiled
bool prof_events(int kind, double work, hipEvent_t* e0, hipEvent_t* e1);

#define ASTTS_CHECK_HIP(expr)                                                              \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            astts::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                             __FILE__, __LINE__);                                          \
            return ASTTS_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

#define ASTTS_REQUIRE(cond, code, ...)                                                     \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            astts::set_error(__VA_ARGS__);                                                 \
            return (code);                                                                 \
        }                                                                                  \
    } while (0)

// launch-path variant: checks the launch itself, never synchronises
#define ASTTS_CHECK_LAUNCH()                                                               \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess) {                                                            \
            astts::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),    \
                             __FILE__, __LINE__);                                          \
            return ASTTS_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

// the kNN scan as one GEMM on the LDS-DMA ring kernel (ops_gemm.hip), row panels of one bank tile first
// (blockmax given: the scores leave scaled -- out = dot * col_scale (+ row_qs * col_bias) -- with the maximum of every (query, 64-row
// block) beside them; ring kernels only: ASTTS_ERR_INVALID unless gemm_scan_blockmax_ok, which a caller asks BEFORE it plans that scan --
// the shape and the ring switch in force, astts_op_gemm_set_ring_mode / ASTTS_GEMM_RING, decide it; queries: null = an aligned pointer)
bool gemm_scan_blockmax_ok(int32_t qg, int64_t n, int32_t dp, const void* queries);
int gemm_scan(const _Float16* queries, const _Float16* bank, float* out, int32_t qg, int64_t n, int32_t dp, int32_t ldc, hipStream_t st,
              const float* col_scale = nullptr, const float* col_bias = nullptr, const float* row_qs = nullptr, float* blockmax = nullptr,
              int32_t bm_ld = 0);

// the LM head with the log-sum-exp epilogue (ops_gemm.hip; the merge and the C entry: ops_score.hip): per (row, 256-column tile) the
// pair (max, sum exp(y - max)) -> part[(m * nblk + tile) * 2], the column of the max -> idx[m * nblk + tile], logit[targets[m]] -> tgt[m]
int gemm_head_lse(const _Float16* h, int32_t ldh, const _Float16* w, const float* bias, const int32_t* targets, int64_t rows, int32_t vocab,
                  int32_t k, float* tgt, float* part, int32_t* idx, int32_t nblk, hipStream_t st);

// an integer experiment switch from the environment (`dflt` when unset).  A set variable is reported once on stderr: these switches
// change which kernel form runs (same results), and a stray one in a user's environment should not go unnoticed (runtime.hip)
int exp_env_int(const char* name, int dflt);

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));

// erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7): one exp, one reciprocal and five FMAs instead of the
// branchy library erff -- the exact-erf GELU of the transformer FFN is evaluated 5.6M times per projection.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);   // v_rcp_f32 (1 ulp); __frcp_rn is a ten-instruction IEEE division
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float erf_abs = 1.0f - poly * __expf(-z * z);
    return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}

}  // namespace astts
