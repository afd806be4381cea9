// knn_handle.h -- the kNN handle and the host calls that knn.hip (create, search) and knn_mutable.hip (append, delete, compact) share.
// Private to csrc/: the public side is include/astts.h and include/knn/astts_knn_mutable.h.
//
// Layout invariants every mutation keeps:
//   * capacity is a multiple of 128 rows and >= n; every plane holds `capacity` rows;
//   * rows [n, capacity) of `scan` and `plane16` are ZERO: the register-streaming scan reads whole 32 / 64-row tiles, the GEMM scan's
//     tile kernels whole tiles of up to 128 rows behind the bank;
//   * the per-row packing (scan image, plane16, plane32, norm64, inv_norm, bias) of a row depends on that row alone, so a row that is
//     appended is packed exactly as astts_knn_create packs it, and a grown bank returns what a bank created at once returns;
//   * `live` is null until the first delete.  While it is set every search is a masked one (its row mask ANDed with `live`).
#pragma once
#include "common.h"

#include <vector>

struct astts_knn {
    int64_t n = 0;
    int64_t capacity = 0;         // rows every plane is allocated for: a multiple of 128, >= n
    int d = 0, dp = 0, nld = 0;   // nld = align_up(n, 128): the leading dimension of a search's score plane (follows n)
    int metric = 0;
    bool exact16 = true;          // scan plane is a lossless image of the bank
    _Float16* scan = nullptr;     // tiled scan plane [capacity / 32 row tiles][dp/64][4][64][8]
    _Float16* plane16 = nullptr;  // [capacity][dp] row-major (exact plane when exact16), zero rows behind row n
    float* plane32 = nullptr;     // [capacity][dp], only when !exact16
    double* norm64 = nullptr;     // [capacity]
    float* inv_norm = nullptr;    // [capacity]  COSINE: 1 / |b| (x the row's power-of-two scale); IP / L2: that scale alone
    float* bias = nullptr;        // [capacity]  L2 only: -|b|^2 / 2
    // largest row norm (IP / L2 certification works on the absolute scale).  After deletes it may OVER-estimate (the largest row may be
    // a tombstone): it only enters the certification bound, so a search may take the exact path more often, and its ids stay exact.
    // astts_knn_compact recomputes it over the survivors.
    double bmax = 0.0;
    double err_bound = 0.0;
    // tombstones (astts_knn_set_deleted): one byte per row of the capacity, 1 = live (rows behind n: 1, so an append needs no write)
    uint8_t* live = nullptr;
    std::vector<uint8_t> live_host;  // host mirror of live[0, n): counts a row once, gives compaction its prefix sum
    int64_t deleted = 0;
    // bench-only profiling (astts_knn_profile_*)
    bool profile = false;
    std::vector<hipEvent_t> ev;  // pairs (start, stop)
    size_t ev_used = 0;
};

namespace astts {

static constexpr int64_t kKnnMaxRows = (int64_t)1024 * 8192;      // 1024 selection segments of kSelSeg scores (knn_kernels.h)

// rows [row0, row0 + m) of every plane from `rows` ([m][d], device, ASTTS_DTYPE_F16 | F32): knn_build_bank.  plane32 is written when
// the handle has one.  flags: device int[4], zeroed by the caller -- [0] some value is not fp16-exact, [1] some value is not finite,
// [2..3] the largest finite row norm (fp64 bits).  Enqueued on st.
int knn_build_rows(astts_knn* h, const void* rows, int64_t row0, int64_t m, int dtype, int* flags, hipStream_t st);
// knn_rescale_rows over rows [row0, row0 + m) of a handle that has a plane32.  Enqueued on st.
int knn_rescale(astts_knn* h, int64_t row0, int64_t m, hipStream_t st);
// the certification bound of the fp16 scan from dp and exact16
void knn_set_err_bound(astts_knn* h);

}  // namespace astts
