// ops_score.hip -- log-probability of given tokens under the LM head, without a logits plane (astts_op_head_logprob).
//
// Teacher-forced scoring wants one float per row: logprob[m] = logit[m][target[m]] - logsumexp(logit[m][0 .. vocab)).  Through the plain
// GEMM that is a [rows, vocab] fp32 plane written and read back (8.4 GB for 16 384 rows of a 128 256-entry vocabulary).  Here the head
// GEMM's epilogue (ops_gemm.hip, tile_epilogue_lse: the kNN scan's block-maximum pattern with a log-sum-exp in place of the maximum)
// reduces every 256-column tile of a row to (max, sum exp(y - max), column of the max) and keeps the target's logit; what reaches
// memory is rows x ceil(vocab / 256) partials (12 bytes each).  head_lse_merge then folds a row's partials: one wave per row, lane l
// takes tiles l, l + 64, ... in ascending order, the 64 lane results meet in a fixed exchange pattern and lane 0 writes.  No
// floating-point atomics anywhere: two launches on the same input give the same bits, and a row's result depends on that row alone.
#include "common.h"

namespace astts {

struct LsePart {
    float mx, sum;
    int idx;
};

// (a then b, b's tiles to the right of a's unless the indices say otherwise: a tie of the maxima keeps the lower column)
__device__ __forceinline__ LsePart lse_combine(const LsePart& a, const LsePart& b) {
    LsePart o;
    if (b.mx > a.mx) {
        o.mx = b.mx;
        o.idx = b.idx;
        o.sum = a.sum * __expf(a.mx - b.mx) + b.sum;       // (a.mx = -inf: a.sum is 0 and exp gives 0)
    } else if (b.mx == a.mx) {
        o.mx = a.mx;
        o.idx = a.idx < b.idx ? a.idx : b.idx;
        o.sum = a.sum + b.sum;
    } else {
        o.mx = a.mx;
        o.idx = a.idx;
        o.sum = a.sum + b.sum * __expf(b.mx - a.mx);
    }
    return o;
}

__global__ __launch_bounds__(256) void head_lse_merge(const float2* __restrict__ part, const int* __restrict__ idx, const float* __restrict__ tgt,
                                                      const int* __restrict__ targets, int64_t rows, int nblk, int vocab,
                                                      float* __restrict__ logprob, float* __restrict__ lse, int* __restrict__ argmax,
                                                      int* __restrict__ ignored) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;                                  // (whole waves: no exchange below is left without its partner)
    LsePart p{-INFINITY, 0.0f, 0x7fffffff};
    for (int b = lane; b < nblk; b += 64) {
        const float2 v = part[m * nblk + b];
        p = lse_combine(p, LsePart{v.x, v.y, idx[m * nblk + b]});
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        LsePart o;
        o.mx = __shfl_xor(p.mx, off, 64);
        o.sum = __shfl_xor(p.sum, off, 64);
        o.idx = __shfl_xor(p.idx, off, 64);
        p = (lane & off) ? lse_combine(o, p) : lse_combine(p, o);      // the lower lane's share first, on both sides of the exchange
    }
    if (lane != 0) return;
    const float l = p.mx + __logf(p.sum);
    const int t = targets[m];
    const bool ign = t < 0 || t >= vocab;
    logprob[m] = ign ? 0.0f : tgt[m] - l;
    if (lse) lse[m] = l;
    if (argmax) argmax[m] = p.idx;
    if (ignored) ignored[m] = ign ? 1 : 0;
}

}  // namespace astts

using namespace astts;

extern "C" {

size_t astts_op_head_logprob_workspace_bytes(int64_t rows, int32_t vocab) {
    if (rows < 1 || vocab < 1) return 0;
    const size_t nblk = (size_t)cdiv(vocab, 256);
    return (size_t)rows * 4 + (size_t)rows * nblk * 12;
}

int astts_op_head_logprob(const void* h_f16, int64_t ldh, const astts_weight_t* head, const int32_t* targets, int64_t rows, int32_t vocab,
                          float* logprob, float* lse, int32_t* argmax, int32_t* ignored, void* workspace, size_t workspace_bytes,
                          astts_stream_t stream) {
    ASTTS_REQUIRE(h_f16 && head && head->w && targets && logprob && workspace, ASTTS_ERR_INVALID, "astts_op_head_logprob: null pointer");
    ASTTS_REQUIRE(rows >= 1 && rows <= (int64_t)1 << 24, ASTTS_ERR_INVALID, "astts_op_head_logprob: rows=%lld", (long long)rows);
    ASTTS_REQUIRE(vocab >= 1 && vocab <= head->n, ASTTS_ERR_INVALID, "astts_op_head_logprob: vocab=%d outside the head's %d rows", vocab, head->n);
    ASTTS_REQUIRE(head->taps == 1 && head->cin == head->cin_pad && head->cin >= 64, ASTTS_ERR_UNSUPPORTED,
                  "astts_op_head_logprob: hidden=%d must be a multiple of 64 (taps=%d)", head->cin, head->taps);
    ASTTS_REQUIRE(ldh >= head->cin && ldh <= 0x7fffffff && (ldh & 7) == 0 && (((uintptr_t)h_f16 | (uintptr_t)head->w) & 15) == 0, ASTTS_ERR_INVALID,
                  "astts_op_head_logprob: h must be 16-byte aligned with a row stride (%lld) that is a multiple of 8 halfs and >= hidden",
                  (long long)ldh);
    ASTTS_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes >= astts_op_head_logprob_workspace_bytes(rows, vocab), ASTTS_ERR_WORKSPACE,
                  "astts_op_head_logprob: workspace of %zu bytes, needs %zu (16-byte aligned)", workspace_bytes,
                  astts_op_head_logprob_workspace_bytes(rows, vocab));
    const int nblk = (int)cdiv(vocab, 256);
    // workspace: partial pairs [rows][nblk] float2 | columns of the maxima [rows][nblk] int32 | target logits [rows]
    float* part = reinterpret_cast<float*>(workspace);
    int32_t* idx = reinterpret_cast<int32_t*>(part + (size_t)rows * nblk * 2);
    float* tgt = reinterpret_cast<float*>(idx + (size_t)rows * nblk);
    hipStream_t st = (hipStream_t)stream;
    const int rc = gemm_head_lse((const _Float16*)h_f16, (int32_t)ldh, (const _Float16*)head->w, head->bias, targets, rows, vocab, head->cin, tgt,
                                 part, idx, nblk, st);
    if (rc != ASTTS_OK) return rc;
    hipLaunchKernelGGL(head_lse_merge, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, st, reinterpret_cast<const float2*>(part), idx, tgt, targets,
                       rows, nblk, vocab, logprob, lse, argmax, ignored);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}

}  // extern "C"
