// train_merge.hip -- libastts_train.so: the live LoRA adapter merged into a second packed fp16 weight image, so that the inference
// path (astts_op_gemm on a PackedWeight) runs on the current parameters while training goes on.
//   out[o, i] = fp16_rn(float(w[o, i]) + scaling * sum_{k < r} b[o, k] * a[part(o) * r + k, i])
// 4 bytes moved and 2 r flops per element (16 flop / byte at r = 32): near the VALU / HBM balance, so a plain LDS-tiled VALU kernel.
// The sum runs over k = 0, 1, .. r - 1 in one fp32 fma chain per element, the base joins it in one more fma (one rounding to fp32,
// one to fp16), no atomics: the image is bit-for-bit repeatable.
#include "train_common.h"

namespace astts_train {

// One workgroup per tile of 32 rows x 128 columns; a thread owns rows (ty, ty + 16) x 8 consecutive columns (one 16-byte access
// of w and out per row).  g1 and g2 are multiples of 32 (or n), so a tile's real rows lie in ONE part: its r rows of A are staged
// in LDS, 32 of them at a time, beside the tile's rows of B.
static constexpr int MG_ROWS = 32, MG_COLS = 128, MG_KC = 32;

__global__ __launch_bounds__(256) void lora_merge_tiles(const _Float16* __restrict__ w, const float* __restrict__ a, const float* __restrict__ b,
                                                        _Float16* __restrict__ out, int n, int cin, int cin_pad, int r, int g1, int g2,
                                                        float scaling) {
    __shared__ float As[MG_KC][MG_COLS];
    __shared__ float Bs[MG_ROWS][MG_KC + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * MG_ROWS, col0 = blockIdx.y * MG_COLS;
    float acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.0f;
    if (row0 < n && col0 < cin) {                                            // block-uniform: a tile of padding alone reads no A and no B
        const int part = (row0 >= g1) + (row0 >= g2);
        const float* __restrict__ ap = a + (int64_t)part * r * cin;
        for (int k0 = 0; k0 < r; k0 += MG_KC) {
            const int kc = r - k0 < MG_KC ? r - k0 : MG_KC;
            for (int kk = tid >> 7; kk < kc; kk += 2) {                      // A: a row of 128 columns per half workgroup
                const int col = col0 + (tid & 127);
                As[kk][tid & 127] = col < cin ? ap[(int64_t)(k0 + kk) * cin + col] : 0.0f;
            }
            for (int rr = tid >> 5; rr < MG_ROWS; rr += 8) {                 // B: 32 consecutive k of one row per 32 threads
                const int kk = tid & 31, row = row0 + rr;
                if (kk < kc) Bs[rr][kk] = row < n ? b[(int64_t)row * r + k0 + kk] : 0.0f;
            }
            __syncthreads();
            for (int kk = 0; kk < kc; ++kk) {
                const float4 a0 = *reinterpret_cast<const float4*>(&As[kk][tx * 8]);
                const float4 a1 = *reinterpret_cast<const float4*>(&As[kk][tx * 8 + 4]);
                const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float b0 = Bs[ty][kk], b1 = Bs[ty + 16][kk];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc[0][e] = fmaf(b0, av[e], acc[0][e]);
                    acc[1][e] = fmaf(b1, av[e], acc[1][e]);
                }
            }
            __syncthreads();
        }
    }
    const int col = col0 + tx * 8;
    if (col >= cin_pad) return;                                              // cin_pad is a multiple of 64: a group of 8 is inside or outside
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = row0 + ty + 16 * i;                                  // < n_pad: the grid covers n_pad / 32 tiles exactly
        const int64_t at = (int64_t)row * cin_pad + col;
        const half8 wv = *reinterpret_cast<const half8*>(w + at);
        half8 ov;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            ov[e] = (row < n && col + e < cin) ? (_Float16)fmaf(scaling, acc[i][e], (float)wv[e]) : (_Float16)0.0f;
        *reinterpret_cast<half8*>(out + at) = ov;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace astts_train

using namespace astts_train;

extern "C" {

int astts_train_lora_merge(const void* w_f16, const float* a, const float* b, void* out_f16, int32_t n, int32_t cin, int32_t n_pad,
                           int32_t cin_pad, int32_t r, int32_t g1, int32_t g2, float scaling, astts_stream_t stream) {
    TRAIN_REQUIRE(w_f16 && a && b && out_f16, ASTTS_ERR_INVALID, "lora_merge: NULL pointer (w %p a %p b %p out %p)", w_f16, (const void*)a,
                  (const void*)b, out_f16);
    TRAIN_REQUIRE(n > 0 && cin > 0 && r >= 8 && r % 8 == 0, ASTTS_ERR_INVALID, "lora_merge: bad shape (n %d cin %d; r %d: a multiple of 8)", n, cin, r);
    TRAIN_REQUIRE(n_pad >= n && n_pad % 128 == 0 && cin_pad >= cin && cin_pad % 64 == 0, ASTTS_ERR_INVALID,
                  "lora_merge: the images are [n_pad, cin_pad] in astts_op_pack_weight's layout (n_pad %d: a multiple of 128 >= n %d; cin_pad %d: a "
                  "multiple of 64 >= cin %d)", n_pad, n, cin_pad, cin);
    TRAIN_REQUIRE(0 < g1 && g1 <= g2 && g2 <= n && (g1 < g2 || g2 == n) && (g1 == n || g1 % 32 == 0) && (g2 == n || g2 % 32 == 0), ASTTS_ERR_INVALID,
                  "lora_merge: the part boundaries must be 0 < g1 <= g2 <= n (equal only at n: no empty part), each a multiple of 32 or n "
                  "itself (g1 %d g2 %d n %d)", g1, g2, n);
    TRAIN_REQUIRE(aligned16(w_f16) && aligned16(out_f16) && ((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0, ASTTS_ERR_INVALID,
                  "lora_merge: w and out must allow 16-byte accesses, a and b 4-byte ones");
    const size_t bytes = (size_t)n_pad * (size_t)cin_pad * sizeof(_Float16);
    const uintptr_t w0 = (uintptr_t)w_f16, o0 = (uintptr_t)out_f16;
    TRAIN_REQUIRE(o0 + bytes <= w0 || w0 + bytes <= o0, ASTTS_ERR_INVALID, "lora_merge: out overlaps w (the frozen base must survive the merge)");
    const int64_t by = cdiv(cin_pad, MG_COLS);
    TRAIN_REQUIRE(by <= 65535, ASTTS_ERR_INVALID, "lora_merge: cin_pad %d exceeds the grid", cin_pad);
    const dim3 grid((unsigned)(n_pad / MG_ROWS), (unsigned)by);
    hipLaunchKernelGGL(lora_merge_tiles, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)w_f16, a, b, (_Float16*)out_f16, n, cin, cin_pad, r,
                       g1, g2, scaling);
    TRAIN_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
