// knn_grouped.hip -- grouped and ranged search of the style bank (include/knn/astts_knn_grouped.h: the result definition and the round
// scheme; DESIGN.md section 3, "Grouped and ranged search").
//
// Nothing here scores a row.  A round is ONE astts_knn_search of a chunk of <= 256 queries under the chunk's per-query row masks, with
// fp64 scores: every scan route, the certification and the exact path of knn.hip run as they are, and a bank with tombstones is ANDed
// in there.  This file keeps what is new: the masks, one int32 per (query, group), and two kernels --
//   knn_group_accept  one wave per query walks the round's hits in order, fills the query's slots and takes the returned rows out of
//                     its mask; counts the chunk's unfinished queries into one word;
//   knn_group_mask    the bandwidth kernel: rewrites the mask row of every query whose group table closed something in this round.
// After each round the host reads that word back (one 4-byte copy and a stream synchronisation): whether another round is needed
// depends on the data.
#include "common.h"
#include "knn_handle.h"
#include "../../include/knn/astts_knn_grouped.h"

#include <initializer_list>

using namespace astts;

namespace {

static constexpr int kChunkQ = 256;            // queries per chunk, as the multi-pass search (kMaxQPerPass of knn_kernels.h)
static constexpr int kFirstRound = 32;         // hits of round 1: the single-pass finish of astts_knn_search
static constexpr int kRoundGrowth = 4;         // 32, 128, 512, then ASTTS_KNN_MAX_K per round
static constexpr int kTableLds = 8192;         // group tables up to this many entries are staged in LDS (32 KB: four blocks share a CU)
static constexpr int kMaskVecPerBlock = 1024;  // 16-byte mask words per block of knn_group_mask: 16384 rows, four per thread
// a group table entry: -1 = not opened, else (slot << kCountBits) | rows accepted so far (<= group_size <= 1024 < 2^11)
static constexpr int kCountBits = 11;
static_assert(ASTTS_KNN_MAX_K < (1 << kCountBits) && ASTTS_KNN_MAX_K <= (1 << (30 - kCountBits)), "slot and count share an int32");
// the state of a query, four ints: [0] groups opened, [1] slots filled, [2] kActive / kFinishedNow / kFinished, [3] the table closed
// something in this round (a group filled, or the limit-th group opened): the mask row has to be rewritten
enum { kActive = 0, kFinishedNow = 1, kFinished = 2 };
// what knn_group_accept stages per hit besides its row: the group code (>= 0), or
enum { kHitDrop = -1, kHitBeyond = -2, kHitNone = -3 };

struct Range {      // the bounds on the fp64 score; near = range_filter, far = radius
    int has_near, has_far, l2;
    double near, far;
};

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// Start of a chunk (blockIdx.y = query): the mask row from the caller's (null: all rows) with a zero tail up to the 16-byte stride, the
// group table unopened, the slots empty, the state zero.  src rows are mask_stride apart and need not be aligned: bytes in, 16 out.
__global__ __launch_bounds__(256) void knn_group_init(uint8_t* __restrict__ mask, int64_t stride, const uint8_t* __restrict__ src,
                                                      int64_t src_stride, int64_t n, int* __restrict__ table, int n_groups,
                                                      int* __restrict__ state, int64_t* __restrict__ out_idx,
                                                      float* __restrict__ out_score, double* __restrict__ out_score64, int slots,
                                                      int l2) {
    const int q = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    uint4* row = reinterpret_cast<uint4*>(mask + (int64_t)q * stride);
    const uint8_t* s = src ? src + (int64_t)q * src_stride : nullptr;
    for (int64_t v = t0; v < stride / 16; v += step) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int b = 0; b < 16; ++b) {
            const int64_t i = v * 16 + b;
            const bool on = i < n && (s ? s[i] != 0 : true);
            w[b >> 2] |= (on ? 1u : 0u) << (8 * (b & 3));
        }
        row[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (table)
        for (int64_t g = t0; g < n_groups; g += step) table[(int64_t)q * n_groups + g] = -1;
    const float none = l2 ? INFINITY : -INFINITY;
    for (int64_t j = t0; j < slots; j += step) {
        out_idx[(int64_t)q * slots + j] = -1;
        out_score[(int64_t)q * slots + j] = none;
        if (out_score64) out_score64[(int64_t)q * slots + j] = (double)none;
    }
    if (t0 < 4) state[q * 4 + t0] = 0;
}

// One wave per query.  The round's hits -- ridx / rs / rs64 [q][r], closest first, -1 behind the hits that exist -- are staged 64 at a
// time (row, and group code or the reason the hit is not a candidate); every returned row leaves the query's mask; lane 0 walks the
// tile in order:
//   closer than range_filter        dropped
//   at or beyond radius             the query is complete: everything after it is farther
//   no hit (-1)                     the round returned fewer hits than asked: the query is exhausted
//   else                            accepted into its group's slot when the group is open and not full, or opened when fewer than
//                                   `limit` groups are; a hit of any other group is passed over
// and the query is complete when its slots are full.  group_of null: every row its own group (no table).
__global__ __launch_bounds__(64) void knn_group_accept(const int64_t* __restrict__ ridx, const float* __restrict__ rs,
                                                       const double* __restrict__ rs64, int r, const int* __restrict__ group_of,
                                                       int n_groups, int* __restrict__ table, int* __restrict__ state,
                                                       uint8_t* __restrict__ mask, int64_t stride, int64_t n, int limit, int group_size,
                                                       Range range, int64_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                       double* __restrict__ out_score64, int* __restrict__ unfinished) {
    __shared__ int s_code[64];
    const int q = blockIdx.x, lane = threadIdx.x;
    int* st = state + q * 4;
    if (st[2] != kActive) {      // finished in an earlier round: its mask is empty, the round returned nothing for it
        if (lane == 0) st[2] = kFinished;
        return;
    }
    const int slots = limit * group_size, target = group_of ? slots : limit;
    const int64_t* qi = ridx + (int64_t)q * r;
    int* tab = table ? table + (int64_t)q * n_groups : nullptr;
    uint8_t* mrow = mask + (int64_t)q * stride;
    int nopen = st[0], filled = st[1], done = 0, sweep = 0;
    for (int j0 = 0; j0 < r && !done; j0 += 64) {
        const int j = j0 + lane;
        int code = kHitNone;
        if (j < r) {
            const int64_t row = qi[j];
            if (row >= 0 && row < n) {
                mrow[row] = 0;
                const double s = rs64[(int64_t)q * r + j];
                const bool too_near = range.has_near && (range.l2 ? s < range.near : s > range.near);
                const bool beyond = range.has_far && (range.l2 ? s >= range.far : s <= range.far);
                if (beyond) code = kHitBeyond;
                else if (too_near) code = kHitDrop;
                else if (!group_of) code = 0;
                else {
                    const int g = group_of[row];
                    code = (unsigned)g < (unsigned)n_groups ? g : kHitDrop;
                }
            }
        }
        s_code[lane] = code;
        __syncthreads();
        if (lane == 0) {
            const int cnt = (r - j0) < 64 ? (r - j0) : 64;
            for (int t = 0; t < cnt; ++t) {
                const int c = s_code[t];
                if (c == kHitDrop) continue;
                if (c == kHitBeyond || c == kHitNone) {
                    done = 1;
                    break;
                }
                int slot;
                if (tab) {
                    int e = tab[c];
                    if (e < 0) {
                        if (nopen >= limit) continue;
                        e = nopen << kCountBits;
                        if (++nopen == limit) sweep = 1;
                    }
                    const int have = e & ((1 << kCountBits) - 1);
                    if (have >= group_size) continue;
                    slot = (e >> kCountBits) * group_size + have;
                    tab[c] = e + 1;
                    if (have + 1 == group_size) sweep = 1;
                } else {
                    slot = nopen * group_size;
                    ++nopen;
                }
                const int64_t src = (int64_t)q * r + j0 + t, dst = (int64_t)q * slots + slot;
                out_idx[dst] = qi[j0 + t];
                out_score[dst] = rs[src];
                if (out_score64) out_score64[dst] = rs64[src];
                ++filled;
                if ((tab ? filled : nopen) >= target) {
                    done = 1;
                    break;
                }
            }
        }
        done = __shfl(done, 0);
        __syncthreads();
    }
    if (lane == 0) {
        st[0] = nopen;
        st[1] = filled;
        st[2] = done ? kFinishedNow : kActive;
        st[3] = sweep;
        if (!done) atomicAdd(unfinished, 1);
    }
}

// The mask rows between two rounds, blockIdx.y = query, 16 bytes of the row per thread and step.  A query that finished in this round:
// its row is cleared (the next rounds return nothing for it).  An unfinished query whose table closed something: a row stays allowed
// only when it was allowed (the rows this round returned have left already) and its group can still take a row -- open and not full,
// or unopened while fewer than `limit` groups are open.  group_of is read once per row that is still allowed: 16-byte words of the
// mask that are zero skip it.  LDS: the query's table is staged in LDS (4 * n_groups bytes of dynamic LDS); else gathered from global.
template <bool LDS>
__global__ __launch_bounds__(256) void knn_group_mask(uint8_t* __restrict__ mask, int64_t stride, int64_t n,
                                                      const int* __restrict__ group_of, int codes_aligned, int n_groups,
                                                      const int* __restrict__ table, const int* __restrict__ state, int limit,
                                                      int group_size) {
    extern __shared__ __attribute__((aligned(16))) int s_tab[];
    const int q = blockIdx.y;
    const int* st = state + q * 4;
    const int status = st[2];
    if (status == kFinished) return;
    if (status == kActive && (!st[3] || !group_of)) return;
    uint4* row = reinterpret_cast<uint4*>(mask + (int64_t)q * stride);
    const int64_t v_begin = (int64_t)blockIdx.x * kMaskVecPerBlock, nvec = stride / 16;
    const int64_t v_end = v_begin + kMaskVecPerBlock < nvec ? v_begin + kMaskVecPerBlock : nvec;
    if (status == kFinishedNow) {
        for (int64_t v = v_begin + threadIdx.x; v < v_end; v += blockDim.x) row[v] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const int* tab = table + (int64_t)q * n_groups;
    if (LDS) {
        for (int g = threadIdx.x; g < n_groups; g += blockDim.x) s_tab[g] = tab[g];
        __syncthreads();
        tab = s_tab;
    }
    const bool closed = st[0] >= limit;
    for (int64_t v = v_begin + threadIdx.x; v < v_end; v += blockDim.x) {
        const uint4 m = row[v];
        if ((m.x | m.y | m.z | m.w) == 0u) continue;
        const int64_t base = v * 16;
        int code[16];
        if (codes_aligned && base + 16 <= n) {
            for (int w = 0; w < 4; ++w) {
                const int4 c = *reinterpret_cast<const int4*>(group_of + base + 4 * w);
                code[4 * w] = c.x, code[4 * w + 1] = c.y, code[4 * w + 2] = c.z, code[4 * w + 3] = c.w;
            }
        } else {
            for (int b = 0; b < 16; ++b) code[b] = base + b < n ? group_of[base + b] : -1;
        }
        const uint32_t in[4] = {m.x, m.y, m.z, m.w};
        uint32_t out[4] = {0u, 0u, 0u, 0u};
        for (int b = 0; b < 16; ++b) {
            if (((in[b >> 2] >> (8 * (b & 3))) & 0xffu) == 0u) continue;
            const int g = code[b];
            bool on = false;
            if ((unsigned)g < (unsigned)n_groups) {
                const int e = tab[g];
                on = e < 0 ? !closed : (e & ((1 << kCountBits) - 1)) < group_size;
            }
            out[b >> 2] |= (on ? 1u : 0u) << (8 * (b & 3));
        }
        if (out[0] != in[0] || out[1] != in[1] || out[2] != in[2] || out[3] != in[3]) row[v] = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
struct GroupedPlan {
    int qc;              // queries per chunk
    int64_t stride;      // bytes of a mask row: n rounded up to 16
    size_t inner_bytes;  // workspace of the rounds' astts_knn_search (the largest over the round sizes)
    size_t off_inner, off_mask, off_table, off_state, off_ridx, off_rs, off_rs64, off_count, total;
};

bool shape_ok(const astts_knn* h, int nq, int limit, int group_size, int n_groups_or_0) {
    return h && nq >= 1 && limit >= 1 && group_size >= 1 && (int64_t)limit * group_size <= ASTTS_KNN_MAX_K && n_groups_or_0 >= 0 &&
           n_groups_or_0 <= h->n;
}

int next_round(int r) { return r * kRoundGrowth < ASTTS_KNN_MAX_K ? r * kRoundGrowth : ASTTS_KNN_MAX_K; }

GroupedPlan make_grouped_plan(const astts_knn* h, int nq, int n_groups_or_0) {
    GroupedPlan p{};
    p.qc = nq < kChunkQ ? nq : kChunkQ;
    p.stride = (int64_t)align_up((size_t)h->n, 16);
    // (the workspace of a search is not monotone in its query count -- a tail chunk below 64 queries splits K where a full one runs a
    // GEMM -- so both chunk sizes are asked about, at every round size)
    const int tail = nq > kChunkQ ? nq % kChunkQ : 0;
    for (int r = kFirstRound;; r = next_round(r)) {
        for (int qc : {p.qc, tail}) {
            const size_t b = qc ? astts_knn_workspace_bytes(h, qc, r) : 0;
            if (b > p.inner_bytes) p.inner_bytes = b;
        }
        if (r == ASTTS_KNN_MAX_K) break;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    p.off_inner = take(p.inner_bytes);
    p.off_mask = take((size_t)p.qc * (size_t)p.stride);
    p.off_table = take(n_groups_or_0 ? sizeof(int) * (size_t)p.qc * n_groups_or_0 : 16);
    p.off_state = take(sizeof(int) * 4 * (size_t)p.qc);
    p.off_ridx = take(sizeof(int64_t) * (size_t)p.qc * ASTTS_KNN_MAX_K);
    p.off_rs = take(sizeof(float) * (size_t)p.qc * ASTTS_KNN_MAX_K);
    p.off_rs64 = take(sizeof(double) * (size_t)p.qc * ASTTS_KNN_MAX_K);
    p.off_count = take(256);
    p.total = o;
    return p;
}

}  // namespace

extern "C" {

size_t astts_knn_grouped_workspace_bytes(const astts_knn_t* h, int32_t nq, int32_t limit, int32_t group_size, int32_t n_groups) {
    if (!shape_ok(h, nq, limit, group_size, n_groups)) return 0;
    return make_grouped_plan(h, nq, n_groups).total;
}

int astts_knn_search_grouped(astts_knn_t* h, const float* queries, int32_t nq, int32_t limit, int32_t group_size,
                             const int32_t* group_of, int32_t n_groups, const double* radius, const double* range_filter,
                             int64_t* out_idx, float* out_score, double* out_score64, const uint8_t* row_mask, int64_t mask_stride,
                             void* workspace, size_t workspace_bytes, int32_t flags, int32_t max_rounds, int32_t* rounds_host,
                             astts_stream_t stream) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_search_grouped: handle is null");
    ASTTS_REQUIRE(queries && out_idx && out_score, ASTTS_ERR_INVALID, "astts_knn_search_grouped: null pointer argument");
    ASTTS_REQUIRE(nq >= 1, ASTTS_ERR_INVALID, "astts_knn_search_grouped: nq=%d", nq);
    ASTTS_REQUIRE(limit >= 1 && group_size >= 1 && (int64_t)limit * group_size <= ASTTS_KNN_MAX_K, ASTTS_ERR_INVALID,
                  "astts_knn_search_grouped: limit=%d x group_size=%d (the product: 1..%d)", limit, group_size, ASTTS_KNN_MAX_K);
    ASTTS_REQUIRE(n_groups >= 1, ASTTS_ERR_INVALID, "astts_knn_search_grouped: n_groups=%d", n_groups);
    ASTTS_REQUIRE(group_of == nullptr || n_groups <= h->n, ASTTS_ERR_INVALID,
                  "astts_knn_search_grouped: n_groups=%d for a bank of %lld rows", n_groups, (long long)h->n);
    ASTTS_REQUIRE(max_rounds >= 0, ASTTS_ERR_INVALID, "astts_knn_search_grouped: max_rounds=%d", max_rounds);
    const bool l2 = h->metric == ASTTS_METRIC_L2;
    Range range{range_filter ? 1 : 0, radius ? 1 : 0, l2 ? 1 : 0, range_filter ? *range_filter : 0.0, radius ? *radius : 0.0};
    ASTTS_REQUIRE(!(range.has_near && range.near != range.near) && !(range.has_far && range.far != range.far), ASTTS_ERR_INVALID,
                  "astts_knn_search_grouped: a range bound is NaN");
    if (range.has_near && range.has_far)
        ASTTS_REQUIRE(l2 ? range.near < range.far : range.far < range.near, ASTTS_ERR_INVALID,
                      "astts_knn_search_grouped: empty range radius=%g range_filter=%g (%s)", range.far, range.near,
                      l2 ? "L2: range_filter <= distance < radius" : "COSINE / IP: radius < score <= range_filter");
    ASTTS_REQUIRE(row_mask == nullptr || mask_stride == 0 || mask_stride >= h->n, ASTTS_ERR_INVALID,
                  "astts_knn_search_grouped: mask_stride %lld (0 = one mask for every query, else >= n = %lld)", (long long)mask_stride,
                  (long long)h->n);
    ASTTS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 255) == 0, ASTTS_ERR_WORKSPACE,
                  "astts_knn_search_grouped: workspace must be 256-byte aligned");
    const int table_groups = group_of ? n_groups : 0;
    const GroupedPlan p = make_grouped_plan(h, nq, table_groups);
    ASTTS_REQUIRE(workspace_bytes >= p.total, ASTTS_ERR_WORKSPACE, "astts_knn_search_grouped: workspace %zu < required %zu",
                  workspace_bytes, p.total);
    if (max_rounds == 0) max_rounds = ASTTS_KNN_GROUPED_DEFAULT_ROUNDS;

    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint8_t* mask = (uint8_t*)(ws + p.off_mask);
    int *table = group_of ? (int*)(ws + p.off_table) : nullptr, *state = (int*)(ws + p.off_state), *count = (int*)(ws + p.off_count);
    int64_t* ridx = (int64_t*)(ws + p.off_ridx);
    float* rs = (float*)(ws + p.off_rs);
    double* rs64 = (double*)(ws + p.off_rs64);
    const int slots = limit * group_size;
    const int64_t nvec = p.stride / 16;
    const unsigned pieces = (unsigned)cdiv(nvec, kMaskVecPerBlock);
    const int codes_aligned = ((uintptr_t)group_of & 15) == 0 ? 1 : 0;
    const bool lds = table_groups <= kTableLds;
    if (rounds_host) *rounds_host = 0;

    for (int q0 = 0; q0 < nq; q0 += p.qc) {
        const int qc = (nq - q0) < p.qc ? (nq - q0) : p.qc;
        const size_t o = (size_t)q0 * slots;
        int64_t* oi = out_idx + o;
        float* os = out_score + o;
        double* os64 = out_score64 ? out_score64 + o : nullptr;
        const int64_t init_work = nvec > table_groups ? nvec : table_groups;
        const unsigned init_blocks = (unsigned)(cdiv(init_work > slots ? init_work : slots, 256) < 1024
                                                    ? cdiv(init_work > slots ? init_work : slots, 256)
                                                    : 1024);
        hipLaunchKernelGGL(knn_group_init, dim3(init_blocks, qc), dim3(256), 0, st, mask, p.stride,
                           row_mask ? row_mask + (int64_t)q0 * mask_stride : nullptr, mask_stride, h->n, table, table_groups, state, oi, os,
                           os64, slots, l2 ? 1 : 0);
        ASTTS_CHECK_LAUNCH();
        int unfinished = 0;
        for (int round = 1, r = kFirstRound;; ++round, r = next_round(r)) {
            ASTTS_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int), st));
            const int rc = astts_knn_search(h, queries + (size_t)q0 * h->d, qc, r, ridx, rs, rs64, mask, p.stride, ws + p.off_inner,
                                            p.inner_bytes, flags, stream);
            if (rc != ASTTS_OK) return rc;
            hipLaunchKernelGGL(knn_group_accept, dim3(qc), dim3(64), 0, st, (const int64_t*)ridx, (const float*)rs, (const double*)rs64, r,
                               (const int*)group_of, table_groups, table, state, mask, p.stride, h->n, limit, group_size, range, oi, os, os64,
                               count);
            ASTTS_CHECK_LAUNCH();
            ASTTS_CHECK_HIP(hipMemcpyAsync(&unfinished, count, sizeof(int), hipMemcpyDeviceToHost, st));
            ASTTS_CHECK_HIP(hipStreamSynchronize(st));
            if (rounds_host && round > *rounds_host) *rounds_host = round;
            if (unfinished == 0) break;
            if (round == max_rounds) {
                set_error("astts_knn_search_grouped: %d of %d queries unfinished after max_rounds=%d rounds (the outputs are incomplete)",
                          unfinished, qc, max_rounds);
                return ASTTS_ERR_UNSUPPORTED;
            }
            if (lds)
                hipLaunchKernelGGL((knn_group_mask<true>), dim3(pieces, qc), dim3(256), sizeof(int) * (size_t)table_groups, st, mask, p.stride,
                                   h->n, (const int*)group_of, codes_aligned, table_groups, (const int*)table, (const int*)state, limit,
                                   group_size);
            else
                hipLaunchKernelGGL((knn_group_mask<false>), dim3(pieces, qc), dim3(256), 0, st, mask, p.stride, h->n, (const int*)group_of,
                                   codes_aligned, table_groups, (const int*)table, (const int*)state, limit, group_size);
            ASTTS_CHECK_LAUNCH();
        }
    }
    return ASTTS_OK;
}

}  // extern "C"
