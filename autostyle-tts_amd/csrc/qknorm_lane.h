// qknorm_lane.h -- how a head of the Qwen3 q / k norm is spread over lanes; shared by the forward kernel (ops_qknorm.hip, libastts.so)
// and its transpose (train/train_ops.hip, libastts_train.so).
//
// A head of HD = 64 or 128 halfs belongs to LPH = HD / 16 neighbouring lanes.  Lane `sub` of the group owns halfs [8 sub, 8 sub + 8) of
// the head's first half AND the 8 at + HD / 2: two 16-byte accesses, and both members of every rotation pair (i, i + HD / 2) sit in the
// same lane, so RoPE needs no exchange.  A wave holds 64 / LPH heads (8 at 128, 16 at 64) and every lane loads.  The sum over the head
// is a butterfly over the group's lanes: DPP moves inside a row of 16 lanes (xlane.h), no LDS round trip and no barrier; both sides of a
// step add the same pair, so every lane of the group ends with the same bits, and the order is fixed.
#pragma once
#include "xlane.h"

namespace astts {

typedef _Float16 qkn_half8 __attribute__((ext_vector_type(8)));

template <int LPH>
__device__ __forceinline__ float qkn_group_sum(float v) {
    static_assert(LPH == 4 || LPH == 8, "head_dim 64 or 128");
    if constexpr (LPH == 8) v = xadd<4>(v);
    v = xadd<2>(v);
    return xadd<1>(v);
}

// the 16 values of one lane: a = the first-half slice, b = the slice HD / 2 further
struct QknLane {
    float a[8], b[8];
};

__device__ __forceinline__ QknLane qkn_load_f16(const _Float16* p, int half) {
    const qkn_half8 va = *reinterpret_cast<const qkn_half8*>(p), vb = *reinterpret_cast<const qkn_half8*>(p + half);
    QknLane o;
#pragma unroll
    for (int e = 0; e < 8; ++e) { o.a[e] = (float)va[e]; o.b[e] = (float)vb[e]; }
    return o;
}

__device__ __forceinline__ void qkn_load8_f32(const float* p, float (&o)[8]) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
    o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w; o[4] = hi.x; o[5] = hi.y; o[6] = hi.z; o[7] = hi.w;
}

__device__ __forceinline__ void qkn_store_f16(_Float16* p, int half, const QknLane& v) {
    qkn_half8 va, vb;
#pragma unroll
    for (int e = 0; e < 8; ++e) { va[e] = (_Float16)v.a[e]; vb[e] = (_Float16)v.b[e]; }
    *reinterpret_cast<qkn_half8*>(p) = va;
    *reinterpret_cast<qkn_half8*>(p + half) = vb;
}

// sum of squares of the lane's 16 values in a fixed order, then over the head
template <int LPH>
__device__ __forceinline__ float qkn_rstd(const QknLane& x, float eps) {
    float ss = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(x.a[e], x.a[e], ss);
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(x.b[e], x.b[e], ss);
    return rsqrtf(qkn_group_sum<LPH>(ss) * (1.0f / (float)(LPH * 16)) + eps);
}

}  // namespace astts
