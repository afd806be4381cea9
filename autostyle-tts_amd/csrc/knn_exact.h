// knn_exact.h -- the exact (fp64) score of a query against a bank row, one wave per (query, row): the arithmetic every path that returns
// a score shares -- the re-score and the exact path of the brute-force search (knn_kernels.h) and the list scan of the IVF index
// (knn_ivf.hip).  Same products in the same order wherever it is used: that is what makes their scores bit-identical.
#pragma once
#include "common.h"

#include <cmath>
#include <type_traits>

namespace astts {

static constexpr int kWave = 64;

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// fp64 dot of a padded fp32 query row with a padded bank row (fp16 or fp32), one wave.
// Lane l accumulates elements 8*(64*s + l) .. +7 for s = 0,1,...; then a symmetric butterfly,
// so every lane returns the same value and identical rows give identical results.
template <typename RowT>
__device__ __forceinline__ double wave_dot64(const float* __restrict__ q, const RowT* __restrict__ row,
                                             int dp, int lane) {
    // (the element pairs of SIX steps are requested before the first FMA: as a rolled loop every step of 512 elements was a
    // dependent global round trip -- twelve in a row for a 6144-wide row, most of the re-score's time; the sums are taken in the same order)
    double acc = 0.0;
    constexpr int U = 6;
    for (int k0 = lane * 8; k0 < dp; k0 += U * kWave * 8) {
        float qv[U][8], b[U][8];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = min(k0 + u * kWave * 8, dp - 8);          // clamped: a valid address, unused past the end
            const float4 q0 = *reinterpret_cast<const float4*>(q + k);
            const float4 q1 = *reinterpret_cast<const float4*>(q + k + 4);
            qv[u][0] = q0.x; qv[u][1] = q0.y; qv[u][2] = q0.z; qv[u][3] = q0.w;
            qv[u][4] = q1.x; qv[u][5] = q1.y; qv[u][6] = q1.z; qv[u][7] = q1.w;
            if constexpr (sizeof(RowT) == 2) {
                const half8 hb = *reinterpret_cast<const half8*>(row + k);
#pragma unroll
                for (int j = 0; j < 8; ++j) b[u][j] = (float)hb[j];
            } else {
                const float4 b0 = *reinterpret_cast<const float4*>(row + k);
                const float4 b1 = *reinterpret_cast<const float4*>(row + k + 4);
                b[u][0] = b0.x; b[u][1] = b0.y; b[u][2] = b0.z; b[u][3] = b0.w;
                b[u][4] = b1.x; b[u][5] = b1.y; b[u][6] = b1.z; b[u][7] = b1.w;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + u * kWave * 8 < dp) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc = fma((double)qv[u][j], (double)b[u][j], acc);
            }
    }
    return wave_sum_f64(acc);
}

__device__ __forceinline__ double cos_from_parts(double dot, double qn, double bn) {
    double c = dot / (qn * bn);
    return isfinite(c) ? c : 0.0;
}

// fp64 squared distance sum_i (q_i - b_i)^2, one wave; the summation tree of wave_dot64 (identical rows give identical results,
// a row equal to the query gives exactly 0)
template <typename RowT>
__device__ __forceinline__ double wave_dist64(const float* __restrict__ q, const RowT* __restrict__ row, int dp, int lane) {
    double acc = 0.0;
    for (int k = lane * 8; k < dp; k += kWave * 8) {
        float4 q0 = *reinterpret_cast<const float4*>(q + k);
        float4 q1 = *reinterpret_cast<const float4*>(q + k + 4);
        const float qq[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        float b[8];
        if constexpr (sizeof(RowT) == 2) {
            half8 hb = *reinterpret_cast<const half8*>(row + k);
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = (float)hb[j];
        } else {
            float4 b0 = *reinterpret_cast<const float4*>(row + k);
            float4 b1 = *reinterpret_cast<const float4*>(row + k + 4);
            b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w;
            b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double df = (double)qq[j] - (double)b[j];
            acc = fma(df, df, acc);
        }
    }
    return wave_sum_f64(acc);
}

// The same two sums with the QUERY in LDS (the small-bank finishing kernel stages it once per workgroup: sixteen waves no longer fetch the
// same 4 dp bytes each) and ALL of the row's pieces requested before the first FMA (dp <= 8192: at most 16 steps; fp32 rows six steps at
// a time).  Same products, same order: bit-identical to wave_dot64 / wave_dist64.
template <typename RowT, bool DIST>
__device__ __forceinline__ double wave_sum64_ldsq(const float* q_lds, const RowT* __restrict__ row, int dp, int lane) {
    double acc = 0.0;
    constexpr int U = sizeof(RowT) == 2 ? 16 : 6;
    typedef typename std::conditional<sizeof(RowT) == 2, half8, float4>::type Piece;      // 8 fp16 values, or 4 of the 8 fp32 values
    for (int k0 = lane * 8; k0 < dp; k0 += U * kWave * 8) {
        Piece pa[U], pb[U];                          // (pb: the second four fp32 values; unused for fp16 rows)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = min(k0 + u * kWave * 8, dp - 8);
            pa[u] = *reinterpret_cast<const Piece*>(row + k);
            if constexpr (sizeof(RowT) != 2) pb[u] = *reinterpret_cast<const Piece*>(row + k + 4);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * kWave * 8;
            if (k < dp) {
                const float4 q0 = *reinterpret_cast<const float4*>(q_lds + k);
                const float4 q1 = *reinterpret_cast<const float4*>(q_lds + k + 4);
                const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                float bv[8];
                if constexpr (sizeof(RowT) == 2) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) bv[j] = (float)pa[u][j];
                } else {
                    bv[0] = pa[u].x; bv[1] = pa[u].y; bv[2] = pa[u].z; bv[3] = pa[u].w;
                    bv[4] = pb[u].x; bv[5] = pb[u].y; bv[6] = pb[u].z; bv[7] = pb[u].w;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if constexpr (DIST) {
                        const double df = (double)qv[j] - (double)bv[j];
                        acc = fma(df, df, acc);
                    } else {
                        acc = fma((double)qv[j], (double)bv[j], acc);
                    }
                }
            }
        }
    }
    return wave_sum_f64(acc);
}

// the exact score S (larger = closer) of query row `q` against bank row `row` under `metric`, in two steps: the wave-wide sum
// (<q, b> or -|q - b|^2), then the part that needs the norms (COSINE)
template <typename RowT>
__device__ __forceinline__ double exact_raw(int metric, const float* __restrict__ q, const RowT* __restrict__ row, int dp, int lane) {
    return metric == ASTTS_METRIC_L2 ? -wave_dist64<RowT>(q, row, dp, lane) : wave_dot64<RowT>(q, row, dp, lane);
}
__device__ __forceinline__ double exact_finish(int metric, double raw, double qn, double bn) {
    return metric == ASTTS_METRIC_COSINE ? cos_from_parts(raw, qn, bn) : raw;
}
template <typename RowT>
__device__ __forceinline__ double exact_score(int metric, const float* __restrict__ q, const RowT* __restrict__ row, int dp, int lane,
                                              double qn, double bn) {
    return exact_finish(metric, exact_raw<RowT>(metric, q, row, dp, lane), qn, bn);
}
// what the caller sees: cosine, inner product, squared distance
__device__ __forceinline__ double user_score(int metric, double s) { return metric == ASTTS_METRIC_L2 ? -s : s; }

}  // namespace astts
