// ops_qknorm.hip -- Qwen3's per-head q / k RMSNorm fused with RoPE (include/llm/astts_qknorm.h): the one launch that replaces
// rope_llama / rope_llama_ex of ops_llm.hip for a shape with qk_norm.  One pass over q | k: 16-byte loads, the head's sum of squares
// inside the wave, norm, weight and rotation in fp32, one rounding to fp16, 16-byte stores.  Lane layout: qknorm_lane.h.
#include "common.h"
#include "qknorm_lane.h"
#include "../../include/llm/astts_qknorm.h"

namespace astts {

// unit = (row, head) in row-major order over the heads + kv_heads heads of a row; LPH lanes per unit.  Lanes beyond the last unit
// work on the last unit again and store nothing: every lane of a wave stays active through the cross-lane steps.
template <int HD>
__global__ __launch_bounds__(256) void qknorm_rope(_Float16* __restrict__ x, const float* __restrict__ cs, const float* __restrict__ sn,
                                                   const float* __restrict__ qw, const float* __restrict__ kw, const int* __restrict__ shift,
                                                   int64_t units, int t, int bsz, int time_major, int heads, int hall, int ld, int pos0, float eps) {
    constexpr int HALF = HD / 2, LPH = HD / 16;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int sub = (int)(tid & (LPH - 1));
    const int64_t unit = tid / LPH;
    const bool live = unit < units;
    const int64_t u = live ? unit : units - 1;
    const int64_t row = u / hall;
    const int hd = (int)(u - row * hall);
    const int ti = time_major ? (int)(row / bsz) : (int)(row % t);
    const int bi = time_major ? (int)(row % bsz) : (int)(row / t);
    const int pos = max(pos0 + ti - (shift ? shift[bi] : 0), 0);

    _Float16* p = x + row * ld + hd * HD + sub * 8;
    const QknLane v = qkn_load_f16(p, HALF);
    float wa[8], wb[8], c[8], s[8];
    const float* w = (hd < heads ? qw : kw) + sub * 8;
    qkn_load8_f32(w, wa);
    qkn_load8_f32(w + HALF, wb);
    qkn_load8_f32(cs + (int64_t)pos * HALF + sub * 8, c);
    qkn_load8_f32(sn + (int64_t)pos * HALF + sub * 8, s);

    const float r = qkn_rstd<LPH>(v, eps);
    QknLane o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float ya = (v.a[e] * r) * wa[e], yb = (v.b[e] * r) * wb[e];     // w * (x * rstd): the order transformers uses
        o.a[e] = ya * c[e] - yb * s[e];
        o.b[e] = yb * c[e] + ya * s[e];
    }
    if (live) qkn_store_f16(p, HALF, o);
}

}  // namespace astts

using namespace astts;

extern "C" {

int astts_op_qknorm_rope(void* x_f16, const float* cos_tab, const float* sin_tab, const float* q_norm_w, const float* k_norm_w,
                         const int32_t* shift, int32_t b, int32_t t, int32_t time_major, int32_t heads, int32_t kv_heads, int32_t ld,
                         int32_t head_dim, int32_t pos0, float eps, astts_stream_t stream) {
    ASTTS_REQUIRE(x_f16 && cos_tab && sin_tab && q_norm_w && k_norm_w, ASTTS_ERR_INVALID, "astts_op_qknorm_rope: null pointer");
    ASTTS_REQUIRE(head_dim == 64 || head_dim == 128, ASTTS_ERR_UNSUPPORTED, "astts_op_qknorm_rope: head_dim=%d (built for 64 and 128)", head_dim);
    ASTTS_REQUIRE(b >= 1 && t >= 1 && heads >= 1 && kv_heads >= 1 && pos0 >= 0 && (int64_t)ld >= (int64_t)(heads + kv_heads) * head_dim &&
                      (ld & 7) == 0 && eps >= 0.0f,
                  ASTTS_ERR_INVALID, "astts_op_qknorm_rope: bad shape b=%d t=%d heads=%d kv_heads=%d head_dim=%d ld=%d pos0=%d", b, t, heads,
                  kv_heads, head_dim, ld, pos0);
    ASTTS_REQUIRE((((uintptr_t)x_f16 | (uintptr_t)cos_tab | (uintptr_t)sin_tab | (uintptr_t)q_norm_w | (uintptr_t)k_norm_w) & 15) == 0,
                  ASTTS_ERR_INVALID, "astts_op_qknorm_rope: x, the tables and the norm weights must be 16-byte aligned");
    const int hall = heads + kv_heads;
    const int64_t units = (int64_t)b * t * hall;
    const int64_t blocks = cdiv(units * (head_dim / 16), 256);
    ASTTS_REQUIRE(blocks < (1ll << 31), ASTTS_ERR_INVALID, "astts_op_qknorm_rope: %lld heads exceed the grid", (long long)units);
    const auto kern = head_dim == 64 ? qknorm_rope<64> : qknorm_rope<128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (_Float16*)x_f16, cos_tab, sin_tab, q_norm_w, k_norm_w,
                       shift, units, t, b, time_major, heads, hall, ld, pos0, eps);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
