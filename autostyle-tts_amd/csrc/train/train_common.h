// train_common.h -- shared host-side helpers of libastts_train.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstdio>

#include "../../../include/train/astts_train.h"

namespace astts_train {

void set_error(const char* fmt, ...);

#define TRAIN_REQUIRE(cond, code, ...)                                                     \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            astts_train::set_error(__VA_ARGS__);                                           \
            return (code);                                                                 \
        }                                                                                  \
    } while (0)

// checks the launch itself, never synchronises
#define TRAIN_CHECK_LAUNCH()                                                               \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess) {                                                            \
            astts_train::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return ASTTS_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));

// v_mfma_f32_32x32x16_f16, D[32 x 32] += A[32 x 16] B[16 x 32].  Lane (c = lane & 31, hh = lane >> 5):
//   A operand element j = A[c][8 hh + j];  B operand element j = B[8 hh + j][c];  D element e = D[(e & 3) + 8 (e >> 2) + 4 hh][c]
__device__ __forceinline__ int mfma_row(int e, int hh) { return (e & 3) + 8 * (e >> 2) + 4 * hh; }

}  // namespace astts_train
