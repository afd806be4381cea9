// knn_ivf.hip -- IVF_FLAT index over the style bank (include/knn/astts_knn_ivf.h: the definition of the index and of a search result;
// DESIGN.md section 3, "IVF_FLAT").
//
// The coarse step -- which centroid is closest to a row (build, append), which lists a query probes (search) -- is astts_knn_search
// against a handle made of the centroids; nothing here scores a centroid.  What is new:
//   ivf_scan             the list scan, list-major: a workgroup owns (list, slice of ASTTS_KNN_IVF_SLICE_ROWS rows), finds the queries of
//                        the chunk that probe its list in the [nq, nprobe] probe table (in query order: no atomics), stages them through
//                        LDS a few at a time and scores every (staged query, row) in fp64 with the sums of knn_exact.h in their order.
//                        A row is gathered once per batch of staged queries and held in registers across them.
//   ivf_select           one workgroup per query: the k best of its candidates on (fp64 score, row index), 64 per pass (toplist.h)
//   ivf_prep_queries     padded fp32 queries and their fp64 norms, summed as the brute-force search of the same call sums them
//   ivf_widen_rows       rows of the exact plane -> fp32 queries of the assignment search (training, append)
//   ivf_update_centroids per (list, 256 columns): the fp32 mean over the list's live rows in ascending row order
#include "common.h"
#include "knn_exact.h"
#include "knn_handle.h"
#include "toplist.h"
#include "../../include/knn/astts_knn_ivf.h"

#include <algorithm>
#include <initializer_list>
#include <vector>

using namespace astts;

struct astts_knn_ivf {
    int nlist = 0;                 // nlist_eff: lists that exist
    int d = 0, dp = 0, metric = 0;
    int64_t n_indexed = 0;         // rows of the bank handle the tables cover
    int64_t max_list_len = 0;
    float* cent_dev = nullptr;     // [nlist][d]
    astts_knn* cent = nullptr;     // the centroids as a bank: the coarse step is astts_knn_search of it
    int* list_off = nullptr;       // device [nlist + 1]
    int* list_ids = nullptr;       // device [ids_cap]: per list its rows, ascending
    int64_t ids_cap = 0;
    std::vector<int32_t> list_of_host;      // [n_indexed]
};

namespace {

static constexpr int kChunkQ = 256;           // queries per chunk, as the multi-pass search (kMaxQPerPass of knn_kernels.h)
static constexpr int kSlice = ASTTS_KNN_IVF_SLICE_ROWS;
static constexpr int kScanThreads = 256;      // four waves: each takes every fourth row of the slice
static constexpr int kMaxQB = 8;              // queries staged in LDS at a time (fewer when 4 dp kMaxQB bytes pass kStageBytes)
static constexpr int kStageBytes = 64 * 1024; // LDS of one scan workgroup: two of them share a CU's 160 KB
static constexpr int kSelPass = 64;           // hits per selection pass: one TopList
static constexpr int kAssignChunk = 4096;     // rows per assignment search
static_assert(ASTTS_KNN_IVF_MAX_DP * 4 <= kStageBytes, "one staged query fits the scan's LDS");

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// The sums of wave_sum64_ldsq (knn_exact.h) for up to kMaxQB queries staged in LDS dp floats apart, the row's pieces loaded ONCE per
// step and kept in registers across the queries.  Per query and lane: the same products in the same order (steps ascending, the eight
// elements of a piece ascending), then the same butterfly -- bit-identical to wave_dot64 / wave_dist64.
template <typename RowT, bool DIST>
__device__ __forceinline__ void wave_sum64_ldsq_multi(const float* q_lds, int nb, const RowT* __restrict__ row, int dp, int lane,
                                                      double (&acc)[kMaxQB]) {
#pragma unroll
    for (int i = 0; i < kMaxQB; ++i) acc[i] = 0.0;
    constexpr int U = sizeof(RowT) == 2 ? 16 : 6;
    typedef typename std::conditional<sizeof(RowT) == 2, half8, float4>::type Piece;
    for (int k0 = lane * 8; k0 < dp; k0 += U * kWave * 8) {
        Piece pa[U], pb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = min(k0 + u * kWave * 8, dp - 8);          // clamped: a valid address, unused past the end
            pa[u] = *reinterpret_cast<const Piece*>(row + k);
            if constexpr (sizeof(RowT) != 2) pb[u] = *reinterpret_cast<const Piece*>(row + k + 4);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * kWave * 8;
            if (k < dp) {
                float bv[8];
                if constexpr (sizeof(RowT) == 2) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) bv[j] = (float)pa[u][j];
                } else {
                    bv[0] = pa[u].x; bv[1] = pa[u].y; bv[2] = pa[u].z; bv[3] = pa[u].w;
                    bv[4] = pb[u].x; bv[5] = pb[u].y; bv[6] = pb[u].z; bv[7] = pb[u].w;
                }
#pragma unroll
                for (int i = 0; i < kMaxQB; ++i) {
                    if (i < nb) {                                   // (wave-uniform)
                        const float4 q0 = *reinterpret_cast<const float4*>(q_lds + (size_t)i * dp + k);
                        const float4 q1 = *reinterpret_cast<const float4*>(q_lds + (size_t)i * dp + k + 4);
                        const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if constexpr (DIST) {
                                const double df = (double)qv[j] - (double)bv[j];
                                acc[i] = fma(df, df, acc[i]);
                            } else {
                                acc[i] = fma((double)qv[j], (double)bv[j], acc[i]);
                            }
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kMaxQB; ++i)
        if (i < nb) acc[i] = wave_sum_f64(acc[i]);
}

// The list scan.  grid (slices of the longest list, lists), kScanThreads threads, dynamic LDS = qb * dp floats.
// probes [nq][np]: the coarse search's hits (a list appears at most once per query).  A workgroup whose slice lies behind its list, or
// whose list no query of the chunk probes, leaves at once.  cand [nq][np][L]: the internal score S (larger = closer) of query q against
// the i-th row of its p-th probed list; rows the tombstones or a mask shared by all queries take out are not fetched and leave their
// slot unwritten -- ivf_select looks at the same bytes before it reads a slot.
template <typename RowT, bool DIST>
__global__ __launch_bounds__(kScanThreads) void ivf_scan(const RowT* __restrict__ plane, const double* __restrict__ norm64,
                                                         const uint8_t* __restrict__ live, const uint8_t* __restrict__ shared_mask,
                                                         const int* __restrict__ list_off, const int* __restrict__ list_ids,
                                                         const int64_t* __restrict__ probes, int nq, int np,
                                                         const float* __restrict__ qf, const double* __restrict__ qn, int dp, int metric,
                                                         int qb, int64_t L, double* __restrict__ cand) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];
    __shared__ int s_hit[kChunkQ];      // q * np + p of the queries that probe this list, in query order
    __shared__ int s_cnt[kScanThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int list = blockIdx.y;
    const int begin = list_off[list], len = list_off[list + 1] - begin;
    const int r0 = blockIdx.x * kSlice;
    if (r0 >= len) return;
    int slot = -1;
    if (tid < nq) {
        const int64_t* pq = probes + (int64_t)tid * np;
        for (int p = 0; p < np; ++p)
            if (pq[p] == (int64_t)list) {
                slot = tid * np + p;
                break;
            }
    }
    const unsigned long long hit = __ballot(slot >= 0);
    if (lane == 0) s_cnt[wid] = __popcll(hit);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / kWave; ++w) {
        if (w < wid) before += s_cnt[w];
        total += s_cnt[w];
    }
    if (total == 0) return;
    if (slot >= 0) s_hit[before + __popcll(hit & ((1ull << lane) - 1ull))] = slot;
    const int nrows = (len - r0) < kSlice ? (len - r0) : kSlice;
    for (int b0 = 0; b0 < total; b0 += qb) {
        const int nb = (total - b0) < qb ? (total - b0) : qb;
        __syncthreads();                 // s_hit is written; the previous batch's readers of s_q are done
        for (int e = tid * 4; e < nb * dp; e += kScanThreads * 4) {      // (dp is a multiple of 64: a float4 stays inside one query)
            const int i = e / dp, k = e - i * dp;
            *reinterpret_cast<float4*>(s_q + e) = *reinterpret_cast<const float4*>(qf + (size_t)(s_hit[b0 + i] / np) * dp + k);
        }
        __syncthreads();
        for (int r = wid; r < nrows; r += kScanThreads / kWave) {
            const int row = list_ids[begin + r0 + r];
            if ((live && !live[row]) || (shared_mask && !shared_mask[row])) continue;      // (wave-uniform)
            double acc[kMaxQB];
            wave_sum64_ldsq_multi<RowT, DIST>(s_q, nb, plane + (int64_t)row * dp, dp, lane, acc);
            const double bn = norm64[row];
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < kMaxQB; ++i)
                    if (i < nb) {
                        const int s = s_hit[b0 + i];
                        cand[(int64_t)s * L + r0 + r] = exact_finish(metric, DIST ? -acc[i] : acc[i], qn[s / np], bn);
                    }
            }
        }
    }
}

// One workgroup (four waves) per query: the k best of the query's candidates -- the rows of its probed lists that the tombstones and
// its mask allow -- on (score, row index), kSelPass per pass; a pass ranks what lies behind the last hit of the pass before it.
__global__ __launch_bounds__(256) void ivf_select(const double* __restrict__ cand, int64_t L, const int64_t* __restrict__ probes, int np,
                                                  int nlist, const int* __restrict__ list_off, const int* __restrict__ list_ids,
                                                  const uint8_t* __restrict__ live, const uint8_t* __restrict__ mask, int64_t mask_stride,
                                                  int k, int metric, int64_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                  double* __restrict__ out_score64) {
    __shared__ double sh_s[4 * 64];
    __shared__ int sh_i[4 * 64];
    __shared__ double s_last_s;
    __shared__ int s_last_i, s_more;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint8_t* mq = mask ? mask + (int64_t)q * mask_stride : nullptr;
    const int64_t ob = (int64_t)q * k;
    const double no_hit = metric == ASTTS_METRIC_L2 ? INFINITY : -INFINITY;
    double last_s = INFINITY;           // (with row -1: every candidate lies behind it)
    int last_i = -1;
    for (int done = 0; done < k; done += kSelPass) {
        const int kp = (k - done) < kSelPass ? (k - done) : kSelPass;
        TopList<double> tl;
        tl.init();
        for (int p = 0; p < np; ++p) {
            const int64_t list = probes[(int64_t)q * np + p];
            if (list < 0 || list >= nlist) continue;
            const int begin = list_off[list], len = list_off[list + 1] - begin;
            const double* cs = cand + ((int64_t)q * np + p) * L;
            for (int base = wid * 64; base < len; base += 256) {
                const int i = base + lane;
                bool valid = i < len;
                int row = kNoIdx;
                double s = -INFINITY;
                if (valid) {
                    row = list_ids[begin + i];
                    valid = (!live || live[row]) && (!mq || mq[row]);
                    if (valid) {
                        s = cs[i];
                        valid = better<double>(last_s, last_i, s, row);
                    }
                }
                tl.offer(s, row, valid, lane, kp);
            }
        }
        merge_lists<double>(tl, sh_s, sh_i, kp);
        if (wid == 0) {
            const bool ok = lane < kp && tl.idx != kNoIdx;
            if (lane < kp) {
                out_idx[ob + done + lane] = ok ? tl.idx : -1;
                out_score[ob + done + lane] = ok ? (float)user_score(metric, tl.s) : (float)no_hit;
                if (out_score64) out_score64[ob + done + lane] = ok ? user_score(metric, tl.s) : no_hit;
            }
            const int found = __popcll(__ballot(ok));
            if (lane == kp - 1) {
                s_last_s = tl.s;
                s_last_i = tl.idx;
            }
            if (lane == 0) s_more = found == kp ? 1 : 0;
        }
        __syncthreads();
        if (!s_more) {                  // the candidates are used up: the rest of the row is empty
            for (int j = done + kSelPass + tid; j < k; j += 256) {
                out_idx[ob + j] = -1;
                out_score[ob + j] = (float)no_hit;
                if (out_score64) out_score64[ob + j] = no_hit;
            }
            return;
        }
        last_s = s_last_s;
        last_i = s_last_i;
        __syncthreads();
    }
}

// One workgroup of 1024 per query: the padded fp32 copy qf [dp] and the fp64 norm.  The norm is summed in the order the brute-force
// search of the same call sums it, so that a COSINE score comes out bit for bit: direct = 0, knn_prep_queries' (256 threads, thread t
// the 8-element groups t, t + 256, ..; four wave sums added in pairs); direct = 1, the finishing kernel's of the DIRECT route (1024
// threads, thread t elements [8 t, 8 t + 8); sixteen wave sums added in wave order; dp == d there).
__global__ __launch_bounds__(1024) void ivf_prep_queries(const float* __restrict__ q, int d, int dp, float* __restrict__ qf,
                                                         double* __restrict__ qn64, int direct) {
    __shared__ double ssum[16];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* s = q + (int64_t)row * d;
    float* of = qf + (int64_t)row * dp;
    for (int k = tid; k < dp; k += 1024) of[k] = k < d ? s[k] : 0.0f;
    double acc = 0.0;
    if (direct) {
        if (tid * 8 < dp) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = tid * 8 + j < d ? s[tid * 8 + j] : 0.0f;
                acc = fma((double)v, (double)v, acc);
            }
        }
    } else if (tid < 256) {
        const int ngroups = dp >> 3;
        for (int gi = 0; gi < 4; ++gi) {
            if (tid + gi * 256 < ngroups) {
                const int g8 = (tid + gi * 256) * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = g8 + j < d ? s[g8 + j] : 0.0f;
                    acc = fma((double)v, (double)v, acc);
                }
            }
        }
        for (int k = 4 * 2048 + tid; k < dp; k += 256) {      // rows longer than 8192
            const float v = k < d ? s[k] : 0.0f;
            acc = fma((double)v, (double)v, acc);
        }
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) ssum[wid] = acc;
    __syncthreads();
    if (tid == 0) {
        double tot;
        if (direct) {
            tot = 0.0;
            for (int w = 0; w < 16; ++w) tot += ssum[w];
        } else {
            tot = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        }
        qn64[row] = sqrt(tot);
    }
}

// fp32 rows [m][d] from the exact plane: row rows[i] when `rows` is given, else row0 + i (blockIdx.y = i)
template <typename RowT>
__global__ __launch_bounds__(256) void ivf_widen_rows(const RowT* __restrict__ plane, int dp, int d, int64_t row0,
                                                      const int64_t* __restrict__ rows, float* __restrict__ out) {
    const int64_t i = blockIdx.y, row = rows ? rows[i] : row0 + i;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < d) out[i * d + k] = (float)plane[row * (int64_t)dp + k];
}

// Centroid of list blockIdx.y, columns blockIdx.x * 256 ..: the fp32 sum over the list's live rows in ascending row order (COSINE: each
// row times the fp32 reciprocal of its fp64 norm, a zero row adds nothing), divided by their count.  A list without a live row keeps
// its centroid.
template <typename RowT>
__global__ __launch_bounds__(256) void ivf_update_centroids(const RowT* __restrict__ plane, int dp, int d, const double* __restrict__ norm64,
                                                            const uint8_t* __restrict__ live, const int* __restrict__ list_off,
                                                            const int* __restrict__ list_ids, float* __restrict__ cent, int cosine) {
    const int list = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int begin = list_off[list], end = list_off[list + 1];
    float acc = 0.0f;
    int cnt = 0;
    for (int i = begin; i < end; ++i) {
        const int row = list_ids[i];
        if (live && !live[row]) continue;
        float v = k < d ? (float)plane[(int64_t)row * dp + k] : 0.0f;
        if (cosine) {
            const double nrm = norm64[row];
            v *= nrm > 0.0 ? (float)(1.0 / nrm) : 0.0f;
        }
        acc += v;
        ++cnt;
    }
    if (cnt > 0 && k < d) cent[(int64_t)list * d + k] = acc / (float)cnt;
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
template <typename F>
void with_plane(const astts_knn* h, F&& launch) {
    if (h->exact16) launch((const _Float16*)h->plane16);
    else launch((const float*)h->plane32);
}

// device scratch of the calls that synchronise anyway (create, assign): freed when it leaves scope
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    ~Scratch() {
        if (p) (void)hipFree(p);
    }
    hipError_t need(size_t b) {
        if (b <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        const hipError_t e = hipMalloc(&p, b);
        if (e == hipSuccess) bytes = b;
        return e;
    }
};

// list_of_host -> offsets, ascending ids (a counting sort on the host: O(n) integers), uploaded; max_list_len
int build_tables(astts_knn_ivf* ivf, hipStream_t st) {
    const int64_t n = (int64_t)ivf->list_of_host.size();
    std::vector<int> off((size_t)ivf->nlist + 1, 0), ids((size_t)n);
    for (int64_t r = 0; r < n; ++r) ++off[(size_t)ivf->list_of_host[(size_t)r] + 1];
    int64_t longest = 0;
    for (int l = 0; l < ivf->nlist; ++l) {
        longest = std::max<int64_t>(longest, off[(size_t)l + 1]);
        off[(size_t)l + 1] += off[(size_t)l];
    }
    std::vector<int> at(off.begin(), off.end() - 1);
    for (int64_t r = 0; r < n; ++r) ids[(size_t)at[(size_t)ivf->list_of_host[(size_t)r]]++] = (int)r;
    if (n > ivf->ids_cap) {
        if (ivf->list_ids) (void)hipFree(ivf->list_ids);
        ivf->list_ids = nullptr;
        ivf->ids_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 1024);
        ASTTS_CHECK_HIP(hipMalloc(&ivf->list_ids, sizeof(int) * (size_t)cap));
        ivf->ids_cap = cap;
    }
    ASTTS_CHECK_HIP(hipMemcpyAsync(ivf->list_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, st));
    ASTTS_CHECK_HIP(hipMemcpyAsync(ivf->list_ids, ids.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    ASTTS_CHECK_HIP(hipStreamSynchronize(st));      // (the host vectors go out of scope)
    ivf->max_list_len = longest;
    ivf->n_indexed = n;
    return ASTTS_OK;
}

// list_of_host[r0, r1) by the assignment rule: chunks of rows widened to fp32 queries, astts_knn_search(centroid bank, k = 1)
int assign_rows(astts_knn_ivf* ivf, astts_knn* h, int64_t r0, int64_t r1, hipStream_t st) {
    if (r1 <= r0) return ASTTS_OK;
    ivf->list_of_host.resize((size_t)r1);
    Scratch qbuf, out, ws;
    const int64_t chunk = std::min<int64_t>(kAssignChunk, r1 - r0);
    ASTTS_CHECK_HIP(qbuf.need(sizeof(float) * (size_t)chunk * ivf->d));
    ASTTS_CHECK_HIP(out.need((sizeof(int64_t) + sizeof(float)) * (size_t)chunk));
    std::vector<int64_t> hit((size_t)chunk);
    for (int64_t b = r0; b < r1; b += chunk) {
        const int m = (int)std::min<int64_t>(chunk, r1 - b);
        const size_t need = astts_knn_workspace_bytes(ivf->cent, m, 1);
        ASTTS_CHECK_HIP(ws.need(need));
        with_plane(h, [&](auto plane) {
            hipLaunchKernelGGL((ivf_widen_rows<std::remove_cv_t<std::remove_pointer_t<decltype(plane)>>>), dim3((unsigned)cdiv(ivf->d, 256), m),
                               dim3(256), 0, st, plane, h->dp, h->d, b, (const int64_t*)nullptr, (float*)qbuf.p);
        });
        ASTTS_CHECK_LAUNCH();
        int64_t* idx = (int64_t*)out.p;
        float* sc = (float*)((char*)out.p + sizeof(int64_t) * (size_t)chunk);
        const int rc = astts_knn_search(ivf->cent, (const float*)qbuf.p, m, 1, idx, sc, nullptr, nullptr, 0, ws.p, ws.bytes, 0,
                                        (astts_stream_t)st);
        if (rc != ASTTS_OK) return rc;
        ASTTS_CHECK_HIP(hipMemcpyAsync(hit.data(), idx, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, st));
        ASTTS_CHECK_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < m; ++i) {
            // (no hit: a row that compares with nothing, NaN scores -- list 0 keeps the tables whole; a bank holds finite values)
            const int64_t l = hit[(size_t)i];
            ivf->list_of_host[(size_t)(b + i)] = (l >= 0 && l < ivf->nlist) ? (int32_t)l : 0;
        }
    }
    return ASTTS_OK;
}

// the centroid bank from cent_dev (replaces the one there is)
int make_centroid_bank(astts_knn_ivf* ivf, hipStream_t st) {
    if (ivf->cent) astts_knn_destroy(ivf->cent);
    ivf->cent = nullptr;
    return astts_knn_create(ivf->cent_dev, ivf->nlist, ivf->d, ASTTS_DTYPE_F32, ivf->metric, (astts_stream_t)st, &ivf->cent);
}

struct IvfPlan {
    int qc, np, qb, direct;
    int64_t L;
    size_t inner_bytes, off_inner, off_pidx, off_ps, off_qf, off_qn, off_cand, total;
};

IvfPlan make_ivf_plan(const astts_knn_ivf* ivf, int nq, int k, int nprobe) {
    IvfPlan p{};
    p.qc = nq < kChunkQ ? nq : kChunkQ;
    p.np = nprobe < ivf->nlist ? nprobe : ivf->nlist;
    p.L = ivf->max_list_len;
    p.qb = kStageBytes / (4 * ivf->dp) < kMaxQB ? kStageBytes / (4 * ivf->dp) : kMaxQB;
    // (the workspace of a search is not monotone in its query count: both chunk sizes are asked about)
    const int tail = nq > kChunkQ ? nq % kChunkQ : 0;
    for (int qc : {p.qc, tail}) {
        const size_t b = qc ? astts_knn_workspace_bytes(ivf->cent, qc, p.np) : 0;
        if (b > p.inner_bytes) p.inner_bytes = b;
    }
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    p.off_inner = take(p.inner_bytes);
    p.off_pidx = take(sizeof(int64_t) * (size_t)p.qc * p.np);
    p.off_ps = take(sizeof(float) * (size_t)p.qc * p.np);
    p.off_qf = take(sizeof(float) * (size_t)p.qc * ivf->dp);
    p.off_qn = take(sizeof(double) * (size_t)p.qc);
    p.off_cand = take(sizeof(double) * (size_t)p.qc * p.np * (size_t)p.L);
    p.total = o;
    return p;
}

bool search_shape_ok(const astts_knn_ivf* ivf, const astts_knn* h, int nq, int k, int nprobe) {
    return ivf && h && ivf->cent && nq >= 1 && k >= 1 && k <= ASTTS_KNN_MAX_K && nprobe >= 1 &&
           (nprobe < ivf->nlist ? nprobe : ivf->nlist) <= ASTTS_KNN_MAX_K;
}

}  // namespace

extern "C" {

int astts_knn_ivf_destroy(astts_knn_ivf_t* ivf) {
    if (!ivf) return ASTTS_OK;
    if (ivf->cent) astts_knn_destroy(ivf->cent);
    if (ivf->cent_dev) (void)hipFree(ivf->cent_dev);
    if (ivf->list_off) (void)hipFree(ivf->list_off);
    if (ivf->list_ids) (void)hipFree(ivf->list_ids);
    delete ivf;
    return ASTTS_OK;
}

int astts_knn_ivf_create(astts_knn_t* h, int32_t nlist, int32_t niter, const float* init_centroids_host, astts_stream_t stream,
                         astts_knn_ivf_t** out) {
    ASTTS_REQUIRE(out != nullptr, ASTTS_ERR_INVALID, "astts_knn_ivf_create: out is null");
    *out = nullptr;
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_ivf_create: handle is null");
    ASTTS_REQUIRE(nlist >= 1 && nlist <= ASTTS_KNN_IVF_MAX_NLIST, ASTTS_ERR_INVALID, "astts_knn_ivf_create: nlist=%d (1..%d)", nlist,
                  ASTTS_KNN_IVF_MAX_NLIST);
    ASTTS_REQUIRE(niter >= 0, ASTTS_ERR_INVALID, "astts_knn_ivf_create: niter=%d", niter);
    ASTTS_REQUIRE(h->dp <= ASTTS_KNN_IVF_MAX_DP, ASTTS_ERR_UNSUPPORTED, "astts_knn_ivf_create: d=%d (the list scan stages rows of up to %d)",
                  h->d, ASTTS_KNN_IVF_MAX_DP);
    const int64_t live = h->n - h->deleted;
    ASTTS_REQUIRE(live >= 1, ASTTS_ERR_INVALID, "astts_knn_ivf_create: the bank has no live row");
    hipStream_t st = (hipStream_t)stream;
    astts_knn_ivf* ivf = new astts_knn_ivf();
    ivf->nlist = (int)std::min<int64_t>(nlist, live);
    ivf->d = h->d;
    ivf->dp = h->dp;
    ivf->metric = h->metric;
    int rc = ASTTS_OK;
    auto run = [&]() -> int {
        const size_t cbytes = sizeof(float) * (size_t)ivf->nlist * ivf->d;
        ASTTS_CHECK_HIP(hipMalloc(&ivf->cent_dev, cbytes));
        ASTTS_CHECK_HIP(hipMalloc(&ivf->list_off, sizeof(int) * ((size_t)ivf->nlist + 1)));
        if (init_centroids_host) {
            ASTTS_CHECK_HIP(hipMemcpyAsync(ivf->cent_dev, init_centroids_host, cbytes, hipMemcpyHostToDevice, st));
            ASTTS_CHECK_HIP(hipStreamSynchronize(st));
        } else {      // the live rows at positions floor(i * live / nlist)
            std::vector<int64_t> alive;
            alive.reserve((size_t)live);
            for (int64_t r = 0; r < h->n; ++r)
                if (!h->live || h->live_host[(size_t)r]) alive.push_back(r);
            std::vector<int64_t> pick((size_t)ivf->nlist);
            for (int i = 0; i < ivf->nlist; ++i) pick[(size_t)i] = alive[(size_t)((int64_t)i * live / ivf->nlist)];
            Scratch rows;
            ASTTS_CHECK_HIP(rows.need(sizeof(int64_t) * pick.size()));
            ASTTS_CHECK_HIP(hipMemcpyAsync(rows.p, pick.data(), sizeof(int64_t) * pick.size(), hipMemcpyHostToDevice, st));
            with_plane(h, [&](auto plane) {
                hipLaunchKernelGGL((ivf_widen_rows<std::remove_cv_t<std::remove_pointer_t<decltype(plane)>>>),
                                   dim3((unsigned)cdiv(ivf->d, 256), ivf->nlist), dim3(256), 0, st, plane, h->dp, h->d, (int64_t)0,
                                   (const int64_t*)rows.p, ivf->cent_dev);
            });
            ASTTS_CHECK_LAUNCH();
            ASTTS_CHECK_HIP(hipStreamSynchronize(st));
        }
        for (int it = 0;; ++it) {
            int r = make_centroid_bank(ivf, st);
            if (r != ASTTS_OK) return r;
            ivf->list_of_host.clear();
            if ((r = assign_rows(ivf, h, 0, h->n, st)) != ASTTS_OK) return r;
            if ((r = build_tables(ivf, st)) != ASTTS_OK) return r;
            if (it == niter) break;
            with_plane(h, [&](auto plane) {
                hipLaunchKernelGGL((ivf_update_centroids<std::remove_cv_t<std::remove_pointer_t<decltype(plane)>>>),
                                   dim3((unsigned)cdiv(ivf->d, 256), ivf->nlist), dim3(256), 0, st, plane, h->dp, h->d,
                                   (const double*)h->norm64, (const uint8_t*)h->live, (const int*)ivf->list_off, (const int*)ivf->list_ids,
                                   ivf->cent_dev, ivf->metric == ASTTS_METRIC_COSINE ? 1 : 0);
            });
            ASTTS_CHECK_LAUNCH();
        }
        return ASTTS_OK;
    };
    rc = run();
    if (rc != ASTTS_OK) {
        astts_knn_ivf_destroy(ivf);
        return rc;
    }
    *out = ivf;
    return ASTTS_OK;
}

int astts_knn_ivf_info(const astts_knn_ivf_t* ivf, int32_t* nlist, int64_t* n_indexed, int64_t* max_list_len) {
    ASTTS_REQUIRE(ivf != nullptr, ASTTS_ERR_INVALID, "astts_knn_ivf_info: index is null");
    if (nlist) *nlist = ivf->nlist;
    if (n_indexed) *n_indexed = ivf->n_indexed;
    if (max_list_len) *max_list_len = ivf->max_list_len;
    return ASTTS_OK;
}

int astts_knn_ivf_export(const astts_knn_ivf_t* ivf, float* centroids_host, int32_t* list_of_host) {
    ASTTS_REQUIRE(ivf != nullptr, ASTTS_ERR_INVALID, "astts_knn_ivf_export: index is null");
    if (centroids_host)
        ASTTS_CHECK_HIP(hipMemcpy(centroids_host, ivf->cent_dev, sizeof(float) * (size_t)ivf->nlist * ivf->d, hipMemcpyDeviceToHost));
    if (list_of_host) std::copy(ivf->list_of_host.begin(), ivf->list_of_host.end(), list_of_host);
    return ASTTS_OK;
}

int astts_knn_ivf_assign(astts_knn_ivf_t* ivf, astts_knn_t* h, astts_stream_t stream) {
    ASTTS_REQUIRE(ivf && h, ASTTS_ERR_INVALID, "astts_knn_ivf_assign: null argument");
    ASTTS_REQUIRE(h->d == ivf->d && h->metric == ivf->metric, ASTTS_ERR_INVALID, "astts_knn_ivf_assign: the handle is not the index's bank");
    ASTTS_REQUIRE(h->n >= ivf->n_indexed, ASTTS_ERR_INVALID,
                  "astts_knn_ivf_assign: the bank has %lld rows, the index covers %lld (after astts_knn_compact: astts_knn_ivf_remap)",
                  (long long)h->n, (long long)ivf->n_indexed);
    if (h->n == ivf->n_indexed) return ASTTS_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t old_n = ivf->n_indexed;
    int rc = assign_rows(ivf, h, old_n, h->n, st);
    if (rc == ASTTS_OK) rc = build_tables(ivf, st);
    if (rc != ASTTS_OK) ivf->list_of_host.resize((size_t)old_n);      // (the tables still describe the rows they did)
    return rc;
}

int astts_knn_ivf_remap(astts_knn_ivf_t* ivf, const int64_t* old_to_new_host, int64_t new_n, astts_stream_t stream) {
    ASTTS_REQUIRE(ivf && old_to_new_host, ASTTS_ERR_INVALID, "astts_knn_ivf_remap: null argument");
    ASTTS_REQUIRE(new_n >= 1 && new_n <= ivf->n_indexed, ASTTS_ERR_INVALID, "astts_knn_ivf_remap: new_n=%lld of %lld rows", (long long)new_n,
                  (long long)ivf->n_indexed);
    std::vector<int32_t> next((size_t)new_n, -1);
    for (int64_t r = 0; r < ivf->n_indexed; ++r) {
        const int64_t t = old_to_new_host[r];
        if (t < 0) continue;
        ASTTS_REQUIRE(t < new_n && next[(size_t)t] < 0, ASTTS_ERR_INVALID, "astts_knn_ivf_remap: row %lld maps to %lld (new_n=%lld, or twice)",
                      (long long)r, (long long)t, (long long)new_n);
        next[(size_t)t] = ivf->list_of_host[(size_t)r];
    }
    for (int64_t t = 0; t < new_n; ++t)
        ASTTS_REQUIRE(next[(size_t)t] >= 0, ASTTS_ERR_INVALID, "astts_knn_ivf_remap: no old row maps to row %lld", (long long)t);
    ivf->list_of_host.swap(next);
    return build_tables(ivf, (hipStream_t)stream);
}

size_t astts_knn_ivf_workspace_bytes(const astts_knn_ivf_t* ivf, const astts_knn_t* h, int32_t nq, int32_t k, int32_t nprobe) {
    if (!search_shape_ok(ivf, h, nq, k, nprobe)) return 0;
    return make_ivf_plan(ivf, nq, k, nprobe).total;
}

int astts_knn_ivf_search(astts_knn_ivf_t* ivf, astts_knn_t* h, const float* queries, int32_t nq, int32_t k, int32_t nprobe,
                         int64_t* out_idx, float* out_score, double* out_score64, const uint8_t* row_mask, int64_t mask_stride,
                         void* workspace, size_t workspace_bytes, astts_stream_t stream) {
    ASTTS_REQUIRE(ivf && h, ASTTS_ERR_INVALID, "astts_knn_ivf_search: null index or handle");
    ASTTS_REQUIRE(queries && out_idx && out_score, ASTTS_ERR_INVALID, "astts_knn_ivf_search: null pointer argument");
    ASTTS_REQUIRE(nq >= 1, ASTTS_ERR_INVALID, "astts_knn_ivf_search: nq=%d", nq);
    ASTTS_REQUIRE(k >= 1 && k <= ASTTS_KNN_MAX_K, ASTTS_ERR_INVALID, "astts_knn_ivf_search: k=%d (1..%d)", k, ASTTS_KNN_MAX_K);
    ASTTS_REQUIRE(nprobe >= 1, ASTTS_ERR_INVALID, "astts_knn_ivf_search: nprobe=%d", nprobe);
    ASTTS_REQUIRE((nprobe < ivf->nlist ? nprobe : ivf->nlist) <= ASTTS_KNN_MAX_K, ASTTS_ERR_UNSUPPORTED,
                  "astts_knn_ivf_search: nprobe=%d of %d lists (the coarse search returns at most %d)", nprobe, ivf->nlist, ASTTS_KNN_MAX_K);
    ASTTS_REQUIRE(h->n == ivf->n_indexed && h->d == ivf->d && h->metric == ivf->metric, ASTTS_ERR_INVALID,
                  "astts_knn_ivf_search: the bank has %lld rows, the index covers %lld (astts_knn_ivf_assign after an append, "
                  "astts_knn_ivf_remap after a compaction)", (long long)h->n, (long long)ivf->n_indexed);
    ASTTS_REQUIRE(row_mask == nullptr || mask_stride == 0 || mask_stride >= h->n, ASTTS_ERR_INVALID,
                  "astts_knn_ivf_search: mask_stride %lld (0 = one mask for every query, else >= n = %lld)", (long long)mask_stride,
                  (long long)h->n);
    ASTTS_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 255) == 0, ASTTS_ERR_WORKSPACE,
                  "astts_knn_ivf_search: workspace must be 256-byte aligned");
    const IvfPlan p = make_ivf_plan(ivf, nq, k, nprobe);
    ASTTS_REQUIRE(workspace_bytes >= p.total, ASTTS_ERR_WORKSPACE, "astts_knn_ivf_search: workspace %zu < required %zu", workspace_bytes,
                  p.total);
    // COSINE divides by the query's norm: it is summed as astts_knn_search of these queries sums it, which depends on its route
    int32_t scan_route = 0;
    int rc = astts_knn_route(h->n, h->d, nq, k, 1, ((uintptr_t)queries & 15) == 0 ? 1 : 0, 0, nullptr, &scan_route, nullptr, nullptr);
    if (rc != ASTTS_OK) return rc;
    const int direct = scan_route == ASTTS_KNN_SCAN_DIRECT ? 1 : 0;

    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int64_t* pidx = (int64_t*)(ws + p.off_pidx);
    float *ps = (float*)(ws + p.off_ps), *qf = (float*)(ws + p.off_qf);
    double *qn = (double*)(ws + p.off_qn), *cand = (double*)(ws + p.off_cand);
    const bool l2 = h->metric == ASTTS_METRIC_L2;
    const dim3 scan_grid((unsigned)cdiv(p.L, kSlice), (unsigned)ivf->nlist);
    const size_t lds = sizeof(float) * (size_t)p.qb * ivf->dp;
    for (int q0 = 0; q0 < nq; q0 += p.qc) {
        const int qc = (nq - q0) < p.qc ? (nq - q0) : p.qc;
        const float* qs = queries + (size_t)q0 * h->d;
        rc = astts_knn_search(ivf->cent, qs, qc, p.np, pidx, ps, nullptr, nullptr, 0, ws + p.off_inner, p.inner_bytes, 0, stream);
        if (rc != ASTTS_OK) return rc;
        hipLaunchKernelGGL(ivf_prep_queries, dim3(qc), dim3(1024), 0, st, qs, h->d, h->dp, qf, qn, direct);
        ASTTS_CHECK_LAUNCH();
        const uint8_t* shared = row_mask && mask_stride == 0 ? row_mask : nullptr;
        with_plane(h, [&](auto plane) {
            using RowT = std::remove_cv_t<std::remove_pointer_t<decltype(plane)>>;
            if (l2)
                hipLaunchKernelGGL((ivf_scan<RowT, true>), scan_grid, dim3(kScanThreads), lds, st, plane, (const double*)h->norm64,
                                   (const uint8_t*)h->live, shared, (const int*)ivf->list_off, (const int*)ivf->list_ids,
                                   (const int64_t*)pidx, qc, p.np, (const float*)qf, (const double*)qn, h->dp, h->metric, p.qb, p.L, cand);
            else
                hipLaunchKernelGGL((ivf_scan<RowT, false>), scan_grid, dim3(kScanThreads), lds, st, plane, (const double*)h->norm64,
                                   (const uint8_t*)h->live, shared, (const int*)ivf->list_off, (const int*)ivf->list_ids,
                                   (const int64_t*)pidx, qc, p.np, (const float*)qf, (const double*)qn, h->dp, h->metric, p.qb, p.L, cand);
        });
        ASTTS_CHECK_LAUNCH();
        hipLaunchKernelGGL(ivf_select, dim3(qc), dim3(256), 0, st, (const double*)cand, p.L, (const int64_t*)pidx, p.np, ivf->nlist,
                           (const int*)ivf->list_off, (const int*)ivf->list_ids, (const uint8_t*)h->live,
                           row_mask ? row_mask + (int64_t)q0 * mask_stride : nullptr, mask_stride, k, h->metric,
                           out_idx + (size_t)q0 * k, out_score + (size_t)q0 * k, out_score64 ? out_score64 + (size_t)q0 * k : nullptr);
        ASTTS_CHECK_LAUNCH();
    }
    return ASTTS_OK;
}

}  // extern "C"
