// knn_mutable.hip -- the style bank changes while it stays resident in HBM: reserve, append, tombstones, compaction
// (include/knn/astts_knn_mutable.h; the handle and its layout invariants: knn_handle.h; create and search: knn.hip).
//
// Nothing here packs a row that the handle already holds.  An append runs the bank-build kernels of astts_knn_create on the new rows
// alone (knn_build_rows / knn_rescale with a row offset), so a grown bank is bit-identical to one created at once.  Growth and
// compaction write into FRESH planes and swap them in when the stream has finished: a failed allocation or a refused batch leaves the
// handle as it was, and no kernel reads rows that another wave of the same launch writes.
#include "common.h"
#include "knn_handle.h"
#include "../../include/knn/astts_knn_mutable.h"

#include <cstring>
#include <vector>

using namespace astts;

namespace {

static constexpr int kRowsPerBlock = 4;      // one wave per row, as the build kernels

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// What knn_build_bank would flag for this batch, without writing a plane: flags[0] a value is not fp16-exact, flags[1] a value is not
// finite.  One wave per row; the rows of a caller's [m][d] array need not be 16-byte aligned (d is arbitrary), so the loads are the
// build kernel's: lane l reads elements l, l + 64, ... -- consecutive lanes, consecutive addresses.
template <typename SrcT>
__global__ __launch_bounds__(256) void knn_check_rows(const SrcT* __restrict__ src, int64_t m, int d, int* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= m) return;
    const SrcT* s = src + row * (int64_t)d;
    bool inexact = false, bad = false;
    for (int k = lane; k < d; k += 64) {
        const float v = (float)s[k];
        if ((float)(_Float16)v != v) inexact = true;
        if (!isfinite(v)) bad = true;
    }
    if (__any(inexact) && lane == 0) atomicOr(&flags[0], 1);
    if (__any(bad) && lane == 0) atomicOr(&flags[1], 1);
}

// Promotion of an fp16-exact handle: rows [0, n) of the fp32 exact plane from the fp16 one (lossless: that is what exact means).
// One wave per row, 16 bytes in and 2 x 16 bytes out per lane and step (dp is a multiple of 64, the planes come from hipMalloc).
__global__ __launch_bounds__(256) void knn_widen_rows(const _Float16* __restrict__ plane16, float* __restrict__ plane32, int64_t n, int dp) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= n) return;
    const _Float16* s = plane16 + row * (int64_t)dp;
    float* o = plane32 + row * (int64_t)dp;
    for (int k = lane * 8; k < dp; k += 64 * 8) {
        const half8 v = *reinterpret_cast<const half8*>(s + k);
        *reinterpret_cast<float4*>(o + k) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        *reinterpret_cast<float4*>(o + k + 4) = make_float4((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
    }
}

// tombstones: live[rows[i]] = 0 (the host has checked the range and dropped rows that were deleted before)
__global__ void knn_live_clear(const int64_t* __restrict__ rows, int64_t m, uint8_t* __restrict__ live) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) live[rows[i]] = 0;
}

// Compaction: new row r of every plane = old row src_of[r] (the host's prefix sum over the live mask: increasing, so the survivors keep
// their order, and no atomics decide a position -- the result is repeatable).  One wave per row, 16-byte accesses; source and
// destination are different allocations.  The scan image of a row holds the values of its plane16 row (both build kernels write the
// same fp16 value to the two), in 16-byte groups: group g of row r sits at ((r / 32 * dp / 64 + line) * 2048 + i * 512 +
// (hh * 32 + r % 32) * 8 with line = g / 8, hh = g % 8 / 4, i = g % 4 -- one load serves both stores.
// bmax_bits: the largest finite norm of the survivors (fp64 bits of a non-negative value order as integers; a maximum does not depend
// on the order of the atomics).
__global__ __launch_bounds__(256) void knn_gather_rows(const int64_t* __restrict__ src_of, int64_t new_n, int dp,
                                                       const _Float16* __restrict__ p16_s, _Float16* __restrict__ p16_d,
                                                       _Float16* __restrict__ scan_d, const float* __restrict__ p32_s,
                                                       float* __restrict__ p32_d, const double* __restrict__ norm_s,
                                                       double* __restrict__ norm_d, const float* __restrict__ inv_s,
                                                       float* __restrict__ inv_d, const float* __restrict__ bias_s,
                                                       float* __restrict__ bias_d, unsigned long long* __restrict__ bmax_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (row >= new_n) return;
    const int64_t src = src_of[row];
    const int64_t tile_base = (row >> 5) * (int64_t)(dp >> 6);
    const int r = (int)(row & 31);
    for (int g = lane; g < (dp >> 3); g += 64) {
        const half8 v = *reinterpret_cast<const half8*>(p16_s + src * (int64_t)dp + g * 8);
        *reinterpret_cast<half8*>(p16_d + row * (int64_t)dp + g * 8) = v;
        const int line = g >> 3, hh = (g & 7) >> 2, i = g & 3;
        *reinterpret_cast<half8*>(scan_d + ((tile_base + line) << 11) + i * 512 + (hh * 32 + r) * 8) = v;
        if (p32_s) {
            const float4 a = *reinterpret_cast<const float4*>(p32_s + src * (int64_t)dp + g * 8);
            const float4 b = *reinterpret_cast<const float4*>(p32_s + src * (int64_t)dp + g * 8 + 4);
            *reinterpret_cast<float4*>(p32_d + row * (int64_t)dp + g * 8) = a;
            *reinterpret_cast<float4*>(p32_d + row * (int64_t)dp + g * 8 + 4) = b;
        }
    }
    if (lane == 0) {
        const double nrm = norm_s[src];
        norm_d[row] = nrm;
        inv_d[row] = inv_s[src];
        if (bias_s) bias_d[row] = bias_s[src];
        if (isfinite(nrm)) atomicMax(bmax_bits, (unsigned long long)__double_as_longlong(nrm));
    }
}

// ------------------------------------------------------------------------------------------
// host: a set of planes that is allocated whole, filled on the stream and then swapped into the handle
// ------------------------------------------------------------------------------------------
struct Planes {
    _Float16 *scan = nullptr, *plane16 = nullptr;
    float* plane32 = nullptr;
    double* norm64 = nullptr;
    float *inv_norm = nullptr, *bias = nullptr;
    uint8_t* live = nullptr;
    void release() {
        for (void* p : {(void*)scan, (void*)plane16, (void*)plane32, (void*)norm64, (void*)inv_norm, (void*)bias, (void*)live})
            if (p) (void)hipFree(p);
        *this = Planes{};
    }
};

// planes of `cap` rows in the shape of the handle (fp32 plane / bias as it has them; live mask on request); all or nothing
int alloc_planes(const astts_knn* h, int64_t cap, bool with_live, Planes* out) {
    Planes p;
    const size_t elems = (size_t)cap * h->dp;
    hipError_t e = hipMalloc(&p.scan, sizeof(_Float16) * elems);
    if (e == hipSuccess) e = hipMalloc(&p.plane16, sizeof(_Float16) * elems);
    if (e == hipSuccess && h->plane32) e = hipMalloc(&p.plane32, sizeof(float) * elems);
    if (e == hipSuccess) e = hipMalloc(&p.norm64, sizeof(double) * (size_t)cap);
    if (e == hipSuccess) e = hipMalloc(&p.inv_norm, sizeof(float) * (size_t)cap);
    if (e == hipSuccess && h->bias) e = hipMalloc(&p.bias, sizeof(float) * (size_t)cap);
    if (e == hipSuccess && with_live) e = hipMalloc(&p.live, (size_t)cap);
    if (e != hipSuccess) {
        p.release();
        set_error("style bank: allocating planes of %lld rows failed: %s", (long long)cap, hipGetErrorString(e));
        return ASTTS_ERR_HIP;
    }
    *out = p;
    return ASTTS_OK;
}

// the handle takes `p` (the stream has finished writing it) and gives up what it had
void swap_in(astts_knn* h, Planes& p, int64_t cap) {
    Planes old;
    old.scan = h->scan, old.plane16 = h->plane16, old.plane32 = h->plane32, old.norm64 = h->norm64, old.inv_norm = h->inv_norm;
    old.bias = h->bias, old.live = h->live;
    h->scan = p.scan, h->plane16 = p.plane16, h->plane32 = p.plane32, h->norm64 = p.norm64, h->inv_norm = p.inv_norm;
    h->bias = p.bias, h->live = p.live;
    h->capacity = cap;
    p = Planes{};
    old.release();
}

#define KNN_TRY_OR(cleanup, expr)                                                            \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            cleanup;                                                                         \
            return ASTTS_ERR_HIP;                                                            \
        }                                                                                    \
    } while (0)

// every plane to `cap` rows (a multiple of 128, > h->capacity), contents preserved, zero / live rows behind them
int grow(astts_knn* h, int64_t cap, hipStream_t st) {
    Planes p;
    int rc = alloc_planes(h, cap, h->live != nullptr, &p);
    if (rc != ASTTS_OK) return rc;
    // the scan plane is row-tile-major and the others row-major: in each the old capacity is a prefix (its zero tail included)
    const size_t old_elems = (size_t)h->capacity * h->dp, new_elems = (size_t)cap * h->dp, n = (size_t)h->n;
    KNN_TRY_OR(p.release(), hipMemcpyAsync(p.scan, h->scan, sizeof(_Float16) * old_elems, hipMemcpyDeviceToDevice, st));
    KNN_TRY_OR(p.release(), hipMemsetAsync(p.scan + old_elems, 0, sizeof(_Float16) * (new_elems - old_elems), st));
    KNN_TRY_OR(p.release(), hipMemcpyAsync(p.plane16, h->plane16, sizeof(_Float16) * old_elems, hipMemcpyDeviceToDevice, st));
    KNN_TRY_OR(p.release(), hipMemsetAsync(p.plane16 + old_elems, 0, sizeof(_Float16) * (new_elems - old_elems), st));
    if (p.plane32) {
        KNN_TRY_OR(p.release(), hipMemcpyAsync(p.plane32, h->plane32, sizeof(float) * n * h->dp, hipMemcpyDeviceToDevice, st));
        KNN_TRY_OR(p.release(), hipMemsetAsync(p.plane32 + n * h->dp, 0, sizeof(float) * (new_elems - n * h->dp), st));
    }
    KNN_TRY_OR(p.release(), hipMemcpyAsync(p.norm64, h->norm64, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    KNN_TRY_OR(p.release(), hipMemcpyAsync(p.inv_norm, h->inv_norm, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
    if (p.bias) KNN_TRY_OR(p.release(), hipMemcpyAsync(p.bias, h->bias, sizeof(float) * n, hipMemcpyDeviceToDevice, st));
    if (p.live) {
        KNN_TRY_OR(p.release(), hipMemcpyAsync(p.live, h->live, (size_t)h->capacity, hipMemcpyDeviceToDevice, st));
        KNN_TRY_OR(p.release(), hipMemsetAsync(p.live + h->capacity, 1, (size_t)(cap - h->capacity), st));
    }
    KNN_TRY_OR(p.release(), hipStreamSynchronize(st));
    swap_in(h, p, cap);
    return ASTTS_OK;
}

// an fp16-exact handle gets its fp32 exact plane: old rows widened, zero behind them.  The caller rescales every row afterwards.
int promote(astts_knn* h, hipStream_t st) {
    float* p32 = nullptr;
    const size_t elems = (size_t)h->capacity * h->dp;
    KNN_TRY_OR((void)0, hipMalloc(&p32, sizeof(float) * elems));
    KNN_TRY_OR((void)hipFree(p32), hipMemsetAsync(p32 + (size_t)h->n * h->dp, 0, sizeof(float) * (elems - (size_t)h->n * h->dp), st));
    hipLaunchKernelGGL(knn_widen_rows, dim3((unsigned)cdiv(h->n, kRowsPerBlock)), dim3(256), 0, st, (const _Float16*)h->plane16, p32, h->n,
                       h->dp);
    KNN_TRY_OR((void)hipFree(p32), hipGetLastError());
    h->plane32 = p32;
    h->exact16 = false;
    knn_set_err_bound(h);
    return ASTTS_OK;
}

}  // namespace

extern "C" {

int astts_knn_reserve(astts_knn_t* h, int64_t capacity, astts_stream_t stream) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_reserve: handle is null");
    ASTTS_REQUIRE(capacity >= 0, ASTTS_ERR_INVALID, "astts_knn_reserve: capacity=%lld", (long long)capacity);
    ASTTS_REQUIRE(capacity <= kKnnMaxRows, ASTTS_ERR_UNSUPPORTED, "astts_knn_reserve: capacity=%lld rows (a bank holds at most %lld)",
                  (long long)capacity, (long long)kKnnMaxRows);
    const int64_t cap = (int64_t)align_up((size_t)capacity, 128);
    if (cap <= h->capacity) return ASTTS_OK;
    return grow(h, cap, (hipStream_t)stream);
}

int astts_knn_append(astts_knn_t* h, const void* rows, int64_t m, int32_t dtype, astts_stream_t stream, int64_t* first_row) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_append: handle is null");
    ASTTS_REQUIRE(m >= 0 && (m == 0 || rows != nullptr), ASTTS_ERR_INVALID, "astts_knn_append: m=%lld rows=%p", (long long)m, rows);
    ASTTS_REQUIRE(dtype == ASTTS_DTYPE_F16 || dtype == ASTTS_DTYPE_F32, ASTTS_ERR_INVALID,
                  "astts_knn_append: dtype %d (want ASTTS_DTYPE_F16|F32)", dtype);
    if (first_row) *first_row = h->n;
    if (m == 0) return ASTTS_OK;
    ASTTS_REQUIRE(m <= kKnnMaxRows && h->n + m <= kKnnMaxRows, ASTTS_ERR_UNSUPPORTED,
                  "astts_knn_append: %lld + %lld rows (a bank holds at most %lld)", (long long)h->n, (long long)m, (long long)kKnnMaxRows);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n0 = h->n, n1 = h->n + m;
    int* flags = nullptr;
    ASTTS_CHECK_HIP(hipMalloc(&flags, 4 * sizeof(int)));
    // 1. the batch is judged before anything changes: a refused append leaves n, the capacity and every plane as they were
    KNN_TRY_OR((void)hipFree(flags), hipMemsetAsync(flags, 0, 4 * sizeof(int), st));
    const dim3 grid((unsigned)cdiv(m, kRowsPerBlock));
    if (dtype == ASTTS_DTYPE_F32) hipLaunchKernelGGL((knn_check_rows<float>), grid, dim3(256), 0, st, (const float*)rows, m, h->d, flags);
    else hipLaunchKernelGGL((knn_check_rows<_Float16>), grid, dim3(256), 0, st, (const _Float16*)rows, m, h->d, flags);
    KNN_TRY_OR((void)hipFree(flags), hipGetLastError());
    int hf[4] = {0, 0, 0, 0};
    KNN_TRY_OR((void)hipFree(flags), hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    KNN_TRY_OR((void)hipFree(flags), hipStreamSynchronize(st));
    if (hf[1]) {
        (void)hipFree(flags);
        set_error("astts_knn_append: the rows hold non-finite values");
        return ASTTS_ERR_RANGE;
    }
    auto fail = [&](int rc) {
        (void)hipFree(flags);
        return rc;
    };
    // 2. room: at least doubled, so a bank that grows row by row is copied O(log n) times
    if (n1 > h->capacity) {
        int64_t cap = 2 * h->capacity;
        if (cap < n1) cap = n1;
        if (cap > kKnnMaxRows) cap = kKnnMaxRows;
        const int rc = grow(h, (int64_t)align_up((size_t)cap, 128), st);
        if (rc != ASTTS_OK) return fail(rc);
    }
    // 3. an fp16-exact handle meets rows that are not: from here on it is the handle astts_knn_create builds from fp32 rows
    const bool promoted = h->exact16 && hf[0] != 0;
    if (promoted) {
        const int rc = promote(h, st);
        if (rc != ASTTS_OK) return fail(rc);
    }
    // 4. the new rows, packed by the kernels of astts_knn_create behind the old ones (flags: their largest norm)
    int rc = knn_build_rows(h, rows, n0, m, dtype, flags, st);
    if (rc == ASTTS_OK && !h->exact16) rc = promoted ? knn_rescale(h, 0, n1, st) : knn_rescale(h, n0, m, st);
    if (rc != ASTTS_OK) return fail(rc);
    KNN_TRY_OR((void)hipFree(flags), hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    KNN_TRY_OR((void)hipFree(flags), hipStreamSynchronize(st));
    (void)hipFree(flags);
    double bmax_new = 0.0;
    memcpy(&bmax_new, &hf[2], sizeof(double));
    if (bmax_new > h->bmax) h->bmax = bmax_new;
    h->n = n1;
    h->nld = (int)align_up((size_t)n1, 128);
    if (h->live) h->live_host.resize((size_t)n1, 1);      // (the device mask is 1 behind the bank already)
    return ASTTS_OK;
}

int astts_knn_set_deleted(astts_knn_t* h, const int64_t* rows_host, int64_t m, astts_stream_t stream) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_set_deleted: handle is null");
    ASTTS_REQUIRE(m >= 0 && (m == 0 || rows_host != nullptr), ASTTS_ERR_INVALID, "astts_knn_set_deleted: m=%lld", (long long)m);
    for (int64_t i = 0; i < m; ++i)
        ASTTS_REQUIRE(rows_host[i] >= 0 && rows_host[i] < h->n, ASTTS_ERR_INVALID, "astts_knn_set_deleted: row %lld outside [0, %lld)",
                      (long long)rows_host[i], (long long)h->n);
    if (m == 0) return ASTTS_OK;
    hipStream_t st = (hipStream_t)stream;
    if (!h->live) {      // the first delete: until here the handle carried no mask
        uint8_t* live = nullptr;
        ASTTS_CHECK_HIP(hipMalloc(&live, (size_t)h->capacity));
        KNN_TRY_OR((void)hipFree(live), hipMemsetAsync(live, 1, (size_t)h->capacity, st));
        h->live = live;
        h->live_host.assign((size_t)h->n, 1);
        h->deleted = 0;
    }
    std::vector<int64_t> fresh;      // rows that were live (once each)
    for (int64_t i = 0; i < m; ++i)
        if (h->live_host[(size_t)rows_host[i]]) {
            h->live_host[(size_t)rows_host[i]] = 0;
            fresh.push_back(rows_host[i]);
        }
    h->deleted += (int64_t)fresh.size();
    if (!fresh.empty()) {
        int64_t* dev = nullptr;
        ASTTS_CHECK_HIP(hipMalloc(&dev, sizeof(int64_t) * fresh.size()));
        KNN_TRY_OR((void)hipFree(dev), hipMemcpyAsync(dev, fresh.data(), sizeof(int64_t) * fresh.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(knn_live_clear, dim3((unsigned)cdiv((int64_t)fresh.size(), 256)), dim3(256), 0, st, (const int64_t*)dev,
                           (int64_t)fresh.size(), h->live);
        KNN_TRY_OR((void)hipFree(dev), hipGetLastError());
        KNN_TRY_OR((void)hipFree(dev), hipStreamSynchronize(st));
        (void)hipFree(dev);
    } else {
        ASTTS_CHECK_HIP(hipStreamSynchronize(st));
    }
    return ASTTS_OK;
}

int astts_knn_compact(astts_knn_t* h, astts_stream_t stream, int64_t* new_n, int64_t* old_to_new_host) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_compact: handle is null");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n0 = h->n, n1 = h->n - h->deleted;
    ASTTS_REQUIRE(n1 >= 1, ASTTS_ERR_UNSUPPORTED, "astts_knn_compact: every row is deleted (a handle holds at least one row: destroy it)");
    if (h->deleted == 0) {      // nothing to remove: drop an all-ones mask, the planes stay
        ASTTS_CHECK_HIP(hipStreamSynchronize(st));
        if (h->live) (void)hipFree(h->live);
        h->live = nullptr;
        h->live_host.clear();
        if (new_n) *new_n = n0;
        if (old_to_new_host)
            for (int64_t i = 0; i < n0; ++i) old_to_new_host[i] = i;
        return ASTTS_OK;
    }
    std::vector<int64_t> src_of((size_t)n1);      // the prefix sum over the live mask, on the host: new row -> old row, increasing
    int64_t next = 0;
    for (int64_t i = 0; i < n0; ++i) {
        const bool live = h->live_host[(size_t)i] != 0;
        if (live) src_of[(size_t)next] = i;
        if (old_to_new_host) old_to_new_host[i] = live ? next : -1;
        next += live ? 1 : 0;
    }
    Planes p;
    int64_t* map = nullptr;
    unsigned long long* bmax_bits = nullptr;
    auto cleanup = [&] {
        p.release();
        if (map) (void)hipFree(map);
        if (bmax_bits) (void)hipFree(bmax_bits);
    };
    int rc = alloc_planes(h, h->capacity, false, &p);
    if (rc != ASTTS_OK) return rc;
    const size_t elems = (size_t)h->capacity * h->dp;
    KNN_TRY_OR(cleanup(), hipMalloc(&map, sizeof(int64_t) * (size_t)n1));
    KNN_TRY_OR(cleanup(), hipMalloc(&bmax_bits, sizeof(unsigned long long)));
    KNN_TRY_OR(cleanup(), hipMemcpyAsync(map, src_of.data(), sizeof(int64_t) * (size_t)n1, hipMemcpyHostToDevice, st));
    KNN_TRY_OR(cleanup(), hipMemsetAsync(bmax_bits, 0, sizeof(unsigned long long), st));
    // the new planes start as zeros: the vacated tail [n1, capacity) stays so
    KNN_TRY_OR(cleanup(), hipMemsetAsync(p.scan, 0, sizeof(_Float16) * elems, st));
    KNN_TRY_OR(cleanup(), hipMemsetAsync(p.plane16, 0, sizeof(_Float16) * elems, st));
    if (p.plane32) KNN_TRY_OR(cleanup(), hipMemsetAsync(p.plane32, 0, sizeof(float) * elems, st));
    hipLaunchKernelGGL(knn_gather_rows, dim3((unsigned)cdiv(n1, kRowsPerBlock)), dim3(256), 0, st, (const int64_t*)map, n1, h->dp,
                       (const _Float16*)h->plane16, p.plane16, p.scan, (const float*)h->plane32, p.plane32, (const double*)h->norm64, p.norm64,
                       (const float*)h->inv_norm, p.inv_norm, (const float*)h->bias, p.bias, bmax_bits);
    KNN_TRY_OR(cleanup(), hipGetLastError());
    unsigned long long bits = 0;
    KNN_TRY_OR(cleanup(), hipMemcpyAsync(&bits, bmax_bits, sizeof(bits), hipMemcpyDeviceToHost, st));
    KNN_TRY_OR(cleanup(), hipStreamSynchronize(st));
    swap_in(h, p, h->capacity);      // (frees the old planes and the live mask: p has none)
    cleanup();
    memcpy(&h->bmax, &bits, sizeof(double));
    h->live_host.clear();
    h->deleted = 0;
    h->n = n1;
    h->nld = (int)align_up((size_t)n1, 128);
    if (new_n) *new_n = n1;
    return ASTTS_OK;
}

int astts_knn_stats(const astts_knn_t* h, int64_t* n, int64_t* live, int64_t* capacity) {
    ASTTS_REQUIRE(h != nullptr, ASTTS_ERR_INVALID, "astts_knn_stats: handle is null");
    if (n) *n = h->n;
    if (live) *live = h->n - h->deleted;
    if (capacity) *capacity = h->capacity;
    return ASTTS_OK;
}

}  // extern "C"
