// ops_sample.hip -- temperature / top-k / top-p sampling of one token per row from a wide logits row (the embedder LLM's
// model.generate(do_sample=True) step: speaker biographies, milvus/search_json.py:113-151 of the reference).  ras_sample
// (ops_audio.hip) keeps its 4 097-entry row in LDS; a Llama row is 128 256 entries = 513 KB, so here only a short list of candidates
// ever reaches LDS.  Definition (include/astts.h, mirrored by tests/llm_sampling_ref.py), per row:
//   candidates = the top_k largest logits under (logit descending, id ascending); s = logit / temperature; p = softmax(s) over the
//   candidates; nucleus = the candidates whose exclusive prefix sum of p is < top_p; token = first nucleus entry whose inclusive
//   prefix sum of p / sum(p over the nucleus) exceeds u.
// One 1024-thread workgroup per row:
//   A  one pass over the row (16-byte loads): every thread's largest key.  A key is the float's bits made order-preserving as an
//      unsigned integer; with the id in the low half it is a 64-bit "entry" and no two entries of a row are equal.
//   B  T0 = the top_k-th largest of the 1024 thread maxima.  Those maxima are distinct elements of the row, so the row's top_k-th
//      largest key is >= T0: a lower bound that, for top_k = 50 on an ordinary row, leaves 50-odd candidates.
//   C  second pass over the row (from L2): the entries with key >= T0 are gathered into LDS (room for 4096).
//   D  <= 1024 candidates: sorted as they are.  More: the exact top_k-th largest entry by a radix select (integer LDS histograms,
//      11 / 11 / 10 bits of the key, then of the id while the threshold bin still holds a tie to break) over the LDS list -- or, when
//      even that overflowed (a row of equal values), over the row itself -- and the top_k survivors are gathered.
//   E  one bitonic sort of <= 1024 entries in LDS (stages that stay inside a wave's 128 entries need no workgroup barrier), then the
//      softmax, the two prefix sums and the draw on one entry per thread.
// Every sum has a fixed order (wave scan, then wave totals in order) and every atomic is an integer one: the same bits on every run.
#include "common.h"

namespace astts {

static constexpr int SP_NT = 1024;      // threads per row
static constexpr int SP_CAP = 4096;     // candidate entries kept in LDS
static constexpr int SP_BINS = 2048;

typedef unsigned long long u64;

__device__ __forceinline__ unsigned sp_key(float v) {
    v += 0.0f;                                                   // -0 -> +0: equal logits get equal keys
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float sp_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ u64 sp_entry(unsigned key, unsigned id) { return ((u64)key << 32) | (u64)(0xffffffffu - id); }

// fn(value, id) for this thread's share of the row; 16-byte loads when the row allows them
template <typename F>
__device__ __forceinline__ void sp_row(const float* __restrict__ xr, int vocab, bool vec, F fn) {
    const int tid = threadIdx.x;
    if (vec) {
        const int nv = vocab >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(xr);
#pragma unroll 4
        for (int i = tid; i < nv; i += SP_NT) {
            const float4 v = x4[i];
            fn(v.x, 4 * i);
            fn(v.y, 4 * i + 1);
            fn(v.z, 4 * i + 2);
            fn(v.w, 4 * i + 3);
        }
        for (int i = (nv << 2) + tid; i < vocab; i += SP_NT) fn(xr[i], i);
    } else {
        for (int i = tid; i < vocab; i += SP_NT) fn(xr[i], i);
    }
}

__device__ __forceinline__ void sp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The k-th largest (k >= 1, at most the number of entries scanned) of the distinct entries `scan` enumerates, or a lower bound of it
// that still leaves exactly k entries at or above it (returned as soon as the threshold bin is taken whole).  hist is zero on entry
// and on exit; the result is uniform over the workgroup.
template <typename Scan>
__device__ u64 sp_select(Scan scan, int k, unsigned* hist, unsigned* wtot, int* sel) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    u64 prefix = 0, known = 0;
    unsigned remaining = (unsigned)k;
#pragma unroll 1
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = pass == 0 ? 53 : pass == 1 ? 42 : pass == 2 ? 32 : pass == 3 ? 21 : pass == 4 ? 10 : 0;
        const unsigned mask = (pass % 3 == 2) ? 1023u : 2047u;
        scan([&](u64 e) {
            if ((e & known) == prefix) atomicAdd(&hist[(unsigned)(e >> shift) & mask], 1u);
        });
        __syncthreads();
        // thread t owns bins 2t and 2t + 1; suffix sums (bins above) inside the wave, then over the waves above
        const uint2 h2 = *reinterpret_cast<const uint2*>(&hist[2 * tid]);
        const unsigned local = h2.x + h2.y;
        unsigned incl = local;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned tv = __shfl_down(incl, off, 64);
            if (lane + off < 64) incl += tv;
        }
        if (lane == 0) wtot[wid] = incl;
        __syncthreads();
        unsigned above = incl - local;
        for (int w = wid + 1; w < SP_NT / 64; ++w) above += wtot[w];
        if (above < remaining && remaining <= above + local) {       // exactly one thread
            if (above + h2.y >= remaining) {
                sel[0] = 2 * tid + 1; sel[1] = (int)(remaining - above); sel[2] = (int)h2.y;
            } else {
                sel[0] = 2 * tid; sel[1] = (int)(remaining - above - h2.y); sel[2] = (int)h2.x;
            }
        }
        *reinterpret_cast<uint2*>(&hist[2 * tid]) = make_uint2(0u, 0u);
        __syncthreads();
        prefix |= (u64)(unsigned)sel[0] << shift;
        known |= (u64)mask << shift;
        remaining = (unsigned)sel[1];
        if (sel[1] == sel[2]) break;                                 // the whole bin is taken: nothing left to split
    }
    return prefix;
}

__global__ __launch_bounds__(SP_NT) void sample_topk_topp(const float* __restrict__ logits, int64_t ld, const float* __restrict__ uniforms,
                                                          int* __restrict__ out, int vocab, float temperature, int top_k, float top_p) {
    __shared__ __attribute__((aligned(16))) u64 cand[SP_CAP];
    __shared__ __attribute__((aligned(16))) u64 sortbuf[SP_NT];
    __shared__ __attribute__((aligned(16))) unsigned hist[SP_BINS];
    __shared__ unsigned wtot[SP_NT / 64];
    __shared__ float wsum[SP_NT / 64];
    __shared__ int sel[3];
    __shared__ int s_cnt, s_cnt2, s_nuc, s_pick;
    __shared__ float s_norm;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* xr = logits + (int64_t)blockIdx.x * ld;
    const bool vec = ((uintptr_t)xr & 15) == 0;                     // uniform: one row
    const float u = uniforms[blockIdx.x];
    const int kk = top_k < vocab ? top_k : vocab;
    *reinterpret_cast<uint2*>(&hist[2 * tid]) = make_uint2(0u, 0u);
    if (tid == 0) { s_cnt = 0; s_cnt2 = 0; s_nuc = kk; s_pick = 0x7fffffff; }

    // A: thread maxima (a thread without elements keeps key 0, below every real key but a negative NaN's)
    unsigned mk = 0u;
    sp_row(xr, vocab, vec, [&](float v, int) { const unsigned k = sp_key(v); mk = k > mk ? k : mk; });
    cand[tid] = sp_entry(mk, (unsigned)tid);
    __syncthreads();
    // B: the kk-th largest thread maximum bounds the kk-th largest element from below
    const unsigned t0 = (unsigned)(sp_select([&](auto fn) { fn(cand[tid]); }, kk, hist, wtot, sel) >> 32);
    // C: gather what can still be among the kk largest
    sp_row(xr, vocab, vec, [&](float v, int id) {
        const unsigned k = sp_key(v);
        // once the list has overflowed only "more than SP_CAP" matters: stop counting (a constant row would otherwise put all its
        // 128 256 entries through this one address)
        if (k >= t0 && *reinterpret_cast<volatile int*>(&s_cnt) <= SP_CAP) {
            const int pos = atomicAdd(&s_cnt, 1);
            if (pos < SP_CAP) cand[pos] = sp_entry(k, (unsigned)id);
        }
    });
    __syncthreads();
    const int cnt = s_cnt;
    u64* sb = cand;
    int n = cnt;
    if (cnt > SP_NT) {
        // D: exact selection, over the LDS list or (overflow) over the row
        u64 thr;
        if (cnt <= SP_CAP) {
            thr = sp_select([&](auto fn) { for (int i = tid; i < cnt; i += SP_NT) fn(cand[i]); }, kk, hist, wtot, sel);
            for (int i = tid; i < cnt; i += SP_NT) {
                const u64 e = cand[i];
                if (e >= thr) {
                    const int pos = atomicAdd(&s_cnt2, 1);
                    if (pos < SP_NT) sortbuf[pos] = e;
                }
            }
        } else {
            thr = sp_select([&](auto fn) {
                sp_row(xr, vocab, vec, [&](float v, int id) { const unsigned k = sp_key(v); if (k >= t0) fn(sp_entry(k, (unsigned)id)); });
            }, kk, hist, wtot, sel);
            sp_row(xr, vocab, vec, [&](float v, int id) {
                const u64 e = sp_entry(sp_key(v), (unsigned)id);
                if (e >= thr) {
                    const int pos = atomicAdd(&s_cnt2, 1);
                    if (pos < SP_NT) sortbuf[pos] = e;
                }
            });
        }
        sb = sortbuf;
        n = kk;
    }
    // E: sort descending (padding entries are 0: below every real entry)
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += SP_NT) sb[i] = 0ull;
    __syncthreads();
#pragma unroll 1
    for (int k2 = 2; k2 <= n2; k2 <<= 1) {
#pragma unroll 1
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            if (j >= 64) __syncthreads(); else sp_wave_sync();       // j <= 64: wave w reads and writes entries [128 w, 128 w + 128) only
            if (tid < (n2 >> 1)) {
                const int i = 2 * tid - (tid & (j - 1)), l = i + j;
                const u64 a = sb[i], b = sb[l];
                if ((a < b) == ((i & k2) == 0)) { sb[i] = b; sb[l] = a; }
            }
        }
    }
    __syncthreads();
    const bool valid = tid < kk;
    const u64 mine = sb[valid ? tid : 0];
    const float smax = sp_unkey((unsigned)(sb[0] >> 32)) / temperature;
    const float e = valid ? expf(sp_unkey((unsigned)(mine >> 32)) / temperature - smax) : 0.0f;
    // inclusive prefix sum over the workgroup in a fixed order: wave scan, then the wave totals in order
    auto scan_incl = [&](float v, float& total) {
        float s = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float tv = __shfl_up(s, off, 64);
            if (lane >= off) s += tv;
        }
        __syncthreads();                                             // wsum may still be read from the previous call
        if (lane == 63) wsum[wid] = s;
        __syncthreads();
        float before = 0.0f, all = 0.0f;
#pragma unroll
        for (int w = 0; w < SP_NT / 64; ++w) {
            if (w == wid) before = all;
            all += wsum[w];
        }
        total = all;
        return before + s;
    };
    float z;
    (void)scan_incl(e, z);
    const float p = e / z;
    float unused;
    const float incl = scan_incl(p, unused);
    const float excl = incl - p;
    // nucleus = [0, first index whose exclusive prefix reaches top_p); entry 0 (exclusive prefix 0) is always inside
    // top_p = 1 cuts nothing (transformers removes nothing there): an fp32 prefix that rounds up to 1.0 in a long tail must not either
    if (valid && tid > 0 && top_p < 1.0f && excl >= top_p) atomicMin(&s_nuc, tid);
    __syncthreads();
    const int nuc = s_nuc;
    if (tid == nuc - 1) s_norm = incl;
    __syncthreads();
    if (tid < nuc && incl / s_norm > u) atomicMin(&s_pick, tid);
    __syncthreads();
    const int pick = s_pick < nuc ? s_pick : nuc - 1;
    if (tid == pick) out[blockIdx.x] = (int)(0xffffffffu - (unsigned)mine);
}

}  // namespace astts

using namespace astts;

extern "C" int astts_op_sample_topk_topp(const float* logits, int64_t ld, const float* uniforms, int32_t* out_tokens, int32_t rows,
                                         int32_t vocab, float temperature, int32_t top_k, float top_p, astts_stream_t stream) {
    ASTTS_REQUIRE(logits && uniforms && out_tokens, ASTTS_ERR_INVALID, "astts_op_sample_topk_topp: null pointer");
    ASTTS_REQUIRE(rows >= 1 && vocab >= 1 && ld >= vocab && ((uintptr_t)logits & 3) == 0, ASTTS_ERR_INVALID,
                  "astts_op_sample_topk_topp: bad shape rows=%d vocab=%d ld=%lld", rows, vocab, (long long)ld);
    ASTTS_REQUIRE(temperature > 0.0f && temperature <= 3.0e38f, ASTTS_ERR_RANGE, "astts_op_sample_topk_topp: temperature=%g must be positive and finite",
                  (double)temperature);
    ASTTS_REQUIRE(top_p > 0.0f && top_p <= 1.0f, ASTTS_ERR_RANGE, "astts_op_sample_topk_topp: top_p=%g outside (0, 1]", (double)top_p);
    ASTTS_REQUIRE(top_k >= 1 && top_k <= SP_NT, ASTTS_ERR_RANGE, "astts_op_sample_topk_topp: top_k=%d outside [1, %d] (0 = off is not supported)",
                  top_k, SP_NT);
    // a row that starts on a 16-byte boundary is read with 16-byte loads; rows of one call agree when ld is a multiple of 4 floats,
    // and the kernel decides per row either way
    hipLaunchKernelGGL(sample_topk_topp, dim3((unsigned)rows), dim3(SP_NT), 0, (hipStream_t)stream, logits, ld, uniforms, out_tokens, vocab,
                       temperature, top_k, top_p);
    ASTTS_CHECK_LAUNCH();
    return ASTTS_OK;
}
