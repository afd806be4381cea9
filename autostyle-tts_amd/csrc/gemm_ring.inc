// gemm_ring.inc -- the two LDS-DMA ring kernels of ops_gemm.hip, included there TWICE: as the GEMM kernels (RING_KERNEL = gemm_ring,
// RING8_KERNEL = gemm_ring8, RING_ARGS = GemmArgs, RING_LSE = 0) and as the LM head's kernels whose epilogue is a log-sum-exp instead of a store
// (head_lse_ring / head_lse_ring8, RING_ARGS = HeadLseArgs, RING_LSE = 1: tile_epilogue_lse).  One text, two kernels: the GEMM kernels' emitted code is what it
// was before the second use existed (a shared inlined body changed their register allocation and schedule; tests/test_isa_checks.py
// holds gemm_ring8's steady-state loop to its shape).
template <int TM, int TN, int STAGES, int WN = 2, int NW = 4>      // NW waves as (NW / WN) x WN; wave tile (32 TM) x (32 TN)
__global__ __launch_bounds__(NW * 64) void RING_KERNEL(RING_ARGS a) {
#if defined(__HIP_DEVICE_COMPILE__)   // the host pass only needs the launch stub (it cannot parse the LDS-DMA builtin)
    constexpr int WM = NW / WN;
    constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
    constexpr int ROWS = BM + BN;
    constexpr int STAGE_BYTES = ROWS * 128;
    constexpr int IPW = ROWS / (8 * NW);           // DMA instructions per wave and stage (8 rows each)
    constexpr int EPI_W = 32 * TN + 4;
    static_assert(STAGES >= 2 && STAGES <= 4, "ring depth");
    static_assert(ROWS % (8 * NW) == 0, "whole DMA instructions per wave");
    static_assert(NW * 32 * EPI_W * 4 <= STAGES * STAGE_BYTES, "epilogue slabs must fit in the ring");
    static_assert((STAGES - 2) * IPW <= 63, "vmcnt immediate");
    extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WN, wn = wid % WN;
    const int r = lane & 31, h = lane >> 5;
    // XCD-aware tile order (1-D launch): the hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with
    // its own L2.  Workgroup w becomes logical tile L = (its XCD's contiguous range) + w / 8, and L walks groups of 4 (256 x 256)
    // or 8 row panels column by column (ring_tile_of): the blocks that run on one XCD at the same time share a few activation AND
    // weight panels in its L2.  PMC on 8192^3 with the 256 x 256 tile, one row panel at a time -> groups of 4: TCC hit rate 48 % -> 80 %,
    // FETCH_SIZE 4.45 GB -> 1.7 GB per launch, +4 % (profiles/r06_ring_group_ab.log, r06_pmc_ring8.txt).
    const int gy = (a.n + BN - 1) / BN;
    int bx, by;
    {
        const int nwg = gridDim.x, w = blockIdx.x;
        const int xcd = w & 7, q = nwg >> 3, r = nwg & 7;
        const int L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (w >> 3);
        ring_tile_of(L, (int)((a.m + BM - 1) / BM), gy, a.m_first ? 0 : (BM >= 256 ? 4 : 8), bx, by);
    }
    const int64_t m0 = (int64_t)bx * BM;
    const int n0 = by * BN;
    const int ktot = a.cin_pad;
    const int nkt = ktot / 64;
    const _Float16* x16 = reinterpret_cast<const _Float16*>(a.x);

    // per-lane source of this wave's IPW row groups at K tile 0
    const _Float16* src[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int row = 8 * (wid + NW * i) + (lane >> 3);
        const int slot = lane & 7;
        if (row < BM) {
            const int c = slot ^ ((row >> 1) & 7);
            int64_t m = m0 + row;
            if (m >= a.m) m = a.m - 1;             // rows past the end: any valid address, never stored
            src[i] = x16 + m * a.lda + c * 8;
        } else {
            const int lr = row - BM;
            const int c = slot ^ ((lr >> 1) & 7);
            int nn = n0 + lr;                      // packed weights are padded to whole tiles; a raw [n][K] matrix (the kNN bank) is not
            if (nn >= a.n) nn = a.n - 1;
            src[i] = a.w + (int64_t)nn * ktot + c * 8;
        }
    }
    auto issue = [&](int kt) {
        unsigned char* dst = ring + (kt % STAGES) * STAGE_BYTES + wid * 1024;
#ifndef RING_SKIP_LOAD
#pragma unroll
        for (int i = 0; i < IPW; ++i)
            __builtin_amdgcn_global_load_lds(src[i] + kt * 64, (__attribute__((address_space(3))) void*)(dst + i * (NW * 1024)), 16, 0, 0);
#endif
    };

    float16v acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    // fragment byte offsets inside a stage (row part; the K chunk is XORed in per k-step)
    int a_off[TM], a_sw[TM], b_off[TN], b_sw[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int lr = (wm * TM + i) * 32 + r;
        a_off[i] = lr * 128;
        a_sw[i] = (lr >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int lr = (wn * TN + j) * 32 + r;
        b_off[j] = BM * 128 + lr * 128;
        b_sw[j] = (lr >> 1) & 7;
    }

#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
        if (s < nkt) issue(s);

    for (int kt = 0; kt < nkt; ++kt) {
        // K tile kt has landed once at most the later tiles' DMAs are outstanding
        const int rem = nkt - kt;
        if (rem >= STAGES - 1) wait_vmcnt<(STAGES - 2) * IPW>();
        else if (rem == 2) wait_vmcnt<IPW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();              // every wave's part of tile kt is in LDS; tile kt-1 is no longer read
        if (kt + STAGES - 1 < nkt) issue(kt + STAGES - 1);
        const unsigned char* st = ring + (kt % STAGES) * STAGE_BYTES;
#ifndef RING_SKIP_MFMA
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8 fa[TM], fb[TN];
            const int c = ks * 2 + h;
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const half8*>(st + a_off[i] + ((c ^ a_sw[i]) << 4));
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const half8*>(st + b_off[j] + ((c ^ b_sw[j]) << 4));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
#endif
    }
    __syncthreads();                               // all fragment reads done (and no DMA outstanding): the ring becomes slab space
#ifndef RING_SKIP_EPI
#if RING_LSE
    static_assert(TN == 2 && NW * 32 * EPI_W * 4 + BM * WN * 12 <= STAGES * STAGE_BYTES, "partials behind the slabs");
    float* part = reinterpret_cast<float*>(ring + NW * 32 * EPI_W * 4);
    tile_epilogue_lse<TM, WN, BM>(a, acc, reinterpret_cast<float*>(ring), part, m0, n0, wm, wn, wid, lane);
    tile_store_lse<BM, WN>(a, part, m0, by, tid, NW * 64);
#else
    if constexpr (WN == 4 && TM == 1 && NW == 4) {
        if (a.ln_gamma) {      // block = whole output rows (n == BN): residual add + LayerNorm of the result fused in
            tile_epilogue_ln<TN>(a, acc[0], reinterpret_cast<float*>(ring), reinterpret_cast<float*>(ring + 4 * 32 * EPI_W * 4), m0, wn, wid, lane);
            return;
        }
    }
    if (a.blockmax) {
        if constexpr (TN == 2 && (WN == 2 || WN == 4) && NW * 32 * EPI_W * 4 + BM * WN * 4 <= STAGES * STAGE_BYTES) {
            float* bm_lds = reinterpret_cast<float*>(ring + NW * 32 * EPI_W * 4);      // behind the waves' slabs
            tile_epilogue_knn<TM, TN, WN>(a, acc, reinterpret_cast<float*>(ring), bm_lds, m0, n0, wm, wn, wid, lane, m0 + BM <= a.m && n0 + BN <= a.n);
            tile_store_blockmax<BM, WN>(a, bm_lds, m0, n0, tid, NW * 64);
        }
    } else {
        tile_epilogue<TM, TN>(a, acc, reinterpret_cast<float*>(ring), m0, n0, wm, wn, wid, lane, m0 + BM <= a.m && n0 + BN <= a.n);
    }
#endif
#else
    if (acc[0][0][0] == 123.0f) a.out[0] = 1.0f;
#endif
#endif
}

// ------------------------------------------------------------------------------------------
// gemm_ring8: the 256 x 256 tile of gemm_ring<4, 2, 2, 4, 8> on the CDNA guide's EIGHT-PHASE schedule (cdna_hip_programming.md, "The
// 256^2 8-phase template"): instead of one barrier, 24 fragment reads and 32 MFMAs per K tile and wave, a K tile is four PHASES of
// (fragment reads of ONE accumulator quadrant's operands + one sub-tile's LDS-DMA, barrier, 8 MFMAs, barrier), and the two wave groups
// of a SIMD (waves w and w + 4: the two row halves of the tile) run ONE BARRIER APART, so that one group's MFMAs cover the other's
// reads and DMA issue.  Same LDS image per stage as gemm_ring (512 rows of 128 B, swizzle on the DMA source and on the reads), two
// stages = 128 KB = eight sub-tile slots.
//
// Sub-tiles (16 KB = 2 DMA instructions per wave) are cut by what a PHASE reads, not by halves of the tile:
//   A0 = row tiles 0, 1 of both wave rows (rows 0-63, 128-191)    A1 = row tiles 2, 3 (rows 64-127, 192-255)
//   B0 = column tile 0 of all four wave columns (32 of every 64)   B1 = column tile 1
// and form ONE sequence S_j, j = 4 t + (0: A0, 1: B0, 2: B1, 3: A1) over the K tiles t.  Phase P = 4 t + p multiplies quadrant
//   p0: (A0, B0) after reading both    p1: (A0, B1) after reading B1    p2: (A1, B1) after reading A1    p3: (A1, B0), B0 kept in registers
// so S_j is read for the first time in phase j (A0) or j - 1 and for the LAST time no later than phase j.
//
// Depth.  The DMA runs as far ahead as the slots allow: phase P requests S_(P+6) into the slot of S_(P-2), whose last read is two
// phases back (the restaging distance the guide asks for with staggered groups) -- five sub-tiles (80 KB) in flight after the request,
// four after the wait (measured: no faster than three ahead -- the kernel is not bound by bytes in flight -- and never slower).
//
// Ordering of the LDS-DMA data (nothing but the issuing wave's counted vmcnt followed by a barrier the READER has passed orders it):
// what phase P + 1 reads first -- everything up to S_(P+2); up to S_(P+1) when P + 1 is a p3 -- is waited for by every wave before global
// barrier 2 (P + 1): the leading group at the end of its phase P, the trailing group (one barrier behind) in the read section of ITS
// phase P, with the same count in both places: vmcnt(2 x the sub-tiles requested behind the needed one).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void RING8_KERNEL(RING_ARGS a) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 256, BN = 256, STAGE_BYTES = 512 * 128, EPI_W = 32 * 2 + 4;
    static_assert(8 * 32 * EPI_W * 4 <= 2 * STAGE_BYTES, "epilogue slabs must fit in the ring");
    extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: the group branches below)
    const int wm = wid >> 2, wn = wid & 3;           // wave tile: rows [128 wm, +128), columns [64 wn, +64)
    const int r = lane & 31, h = lane >> 5;
    const int gy = (a.n + BN - 1) / BN;
    int bx, by;
    {
        const int nwg = gridDim.x, w = blockIdx.x;
        const int xcd = w & 7, q = nwg >> 3, rr = nwg & 7;
        const int L = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (w >> 3);
        ring_tile_of(L, (int)((a.m + BM - 1) / BM), gy, a.m_first ? 0 : 4, bx, by);
    }
    const int64_t m0 = (int64_t)bx * BM;
    const int n0 = by * BN;
    const int ktot = a.cin_pad;
    const int nkt = ktot / 64;
    const _Float16* x16 = reinterpret_cast<const _Float16*>(a.x);

    // ---- DMA: sub-tile s (0 A0, 1 B0, 2 B1, 3 A1) = 16 row groups of 8 rows; wave w takes groups w and w + 8.
    //   A sub-tiles: group g -> tile rows 128 (g / 8) + 64 (s == 3) + 8 (g % 8)
    //   B sub-tiles: group g -> tile columns 64 (g / 4) + 32 (s == 2) + 8 (g % 4)
    const _Float16* src[4][2];
    int dst[4][2];                                   // byte offset of the 8-row group inside a stage
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int g = wid + 8 * i;
            const bool is_a = sb == 0 || sb == 3;
            const int row0 = is_a ? 128 * (g >> 3) + (sb == 3 ? 64 : 0) + 8 * (g & 7) : 64 * (g >> 2) + (sb == 2 ? 32 : 0) + 8 * (g & 3);
            const int row = row0 + (lane >> 3);      // this lane's row of the group, 16-byte slot lane & 7
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            if (is_a) {
                int64_t m = m0 + row;
                if (m >= a.m) m = a.m - 1;
                src[sb][i] = x16 + m * a.lda + c * 8;
                dst[sb][i] = row0 * 128;
            } else {
                int nn = n0 + row;
                if (nn >= a.n) nn = a.n - 1;
                src[sb][i] = a.w + (int64_t)nn * ktot + c * 8;
                dst[sb][i] = (BM + row0) * 128;
            }
        }
    auto issue = [&](int kt, int sb) {               // (sb is a compile-time constant at every call)
        unsigned char* base = ring + (kt & 1) * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds(src[sb][i] + kt * 64, (__attribute__((address_space(3))) void*)(base + dst[sb][i]), 16, 0, 0);
    };

    float16v acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    int a_off[4], a_sw[4], b_off[2], b_sw[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lr = wm * 128 + i * 32 + r;
        a_off[i] = lr * 128;
        a_sw[i] = (lr >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int lr = wn * 64 + j * 32 + r;
        b_off[j] = BM * 128 + lr * 128;
        b_sw[j] = (lr >> 1) & 7;
    }
    half8 fa[2][4], fb[2][4];                        // two row tiles x 4 k-steps of the current A sub-tile; both column tiles x 4 k-steps
    auto read_a = [&](const unsigned char* st, int i0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                fa[i][ks] = *reinterpret_cast<const half8*>(st + a_off[i0 + i] + (((ks * 2 + h) ^ a_sw[i0 + i]) << 4));
    };
    auto read_b = [&](const unsigned char* st, int j) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) fb[j][ks] = *reinterpret_cast<const half8*>(st + b_off[j] + (((ks * 2 + h) ^ b_sw[j]) << 4));
    };
    auto mma = [&](int i0, int j) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][ks], fb[j][ks], acc[i0 + i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    // the counted wait in front of the NEXT phase's reads.  rem = sub-tiles of the sequence behind this phase's own index P
    // (4 nkt - 1 - P); requested so far: through S_(P + min(6, rem)); needed: through S_(P + min(need, rem)).
    auto wait_for = [&](int rem, int need) {
        const int left = (rem < 6 ? rem : 6) - (rem < need ? rem : need);
        if (left >= 5) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else if (left == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (left == 3) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (left == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (left == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    const bool trail = wm == 1;                      // the trailing group: one barrier behind, waits in its read section
    const int last = 4 * nkt - 1;

    // ---- prologue: S_0 .. S_5 (K tile 0 whole, A0 and B0 of K tile 1); S_0, S_1 must have landed before phase 0
    issue(0, 0);
    issue(0, 1);
    issue(0, 2);
    issue(0, 3);
    if (nkt > 1) {
        issue(1, 0);
        issue(1, 1);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                    // (global barrier 0: every wave's part of S_0, S_1 is in LDS)
    if (trail) __builtin_amdgcn_s_barrier();

#define RING8_PHASE(STEADY, P, READS, ISSUE_KT, SB, I0, J, NEED)                                              \
    do {                                                                                                      \
        const int rem = last - (4 * kt + (P));                                                                \
        READS;                                                                                                \
        if (STEADY || rem >= 6) issue(ISSUE_KT, SB);                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        if (trail) {                                                                                          \
            if (STEADY) wait_vmcnt<2 * (6 - (NEED))>();                                                       \
            else wait_for(rem, NEED);                                                                         \
        }                                                                                                     \
        __builtin_amdgcn_s_barrier();                                                                         \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        mma(I0, J);                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                    \
        if (!trail) {                                                                                         \
            if (STEADY) wait_vmcnt<2 * (6 - (NEED))>();                                                       \
            else wait_for(rem, NEED);                                                                         \
        }                                                                                                     \
        __builtin_amdgcn_s_barrier();                                                                         \
    } while (0)
#define RING8_TILE(STEADY)                                                                                                                     \
    do {                                                                                                                                       \
        const unsigned char* st = ring + (kt & 1) * STAGE_BYTES;                                                                               \
        RING8_PHASE(STEADY, 0, (read_b(st, 0), __builtin_amdgcn_sched_barrier(0), read_a(st, 0)), kt + 1, 2, 0, 0, 2); /* requests B1(kt + 1); p1 reads B1(kt) */ \
        RING8_PHASE(STEADY, 1, read_b(st, 1), kt + 1, 3, 0, 1, 2);                                  /* requests A1(kt + 1); p2 reads A1(kt) */  \
        RING8_PHASE(STEADY, 2, read_a(st, 2), kt + 2, 0, 2, 1, 1);                                  /* requests A0(kt + 2); p3 reads nothing */ \
        RING8_PHASE(STEADY, 3, (void)0, kt + 2, 1, 2, 0, 2);                                        /* requests B0(kt + 2); p0 reads A0, B0(kt + 1) */ \
    } while (0)

    int kt = 0;
    for (; kt < nkt - 2; ++kt) RING8_TILE(true);     // steady state: every phase requests, every wait is a constant
    for (; kt < nkt; ++kt) RING8_TILE(false);        // the last two K tiles: requests run out, the counts shrink
#undef RING8_TILE
#undef RING8_PHASE
    if (!trail) __builtin_amdgcn_s_barrier();        // (the barrier the trailing group took up front)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                 // all fragment reads done, no DMA outstanding: the ring becomes slab space
#if RING_LSE
    static_assert(8 * 32 * EPI_W * 4 + BM * 4 * 12 <= 2 * STAGE_BYTES, "partials behind the slabs");
    float* part = reinterpret_cast<float*>(ring + 8 * 32 * EPI_W * 4);
    tile_epilogue_lse<4, 4, BM>(a, acc, reinterpret_cast<float*>(ring), part, m0, n0, wm, wn, wid, lane);
    tile_store_lse<BM, 4>(a, part, m0, by, tid, 512);
#else
    if (a.blockmax) {
        static_assert(8 * 32 * EPI_W * 4 + BM * 4 * 4 <= 2 * STAGE_BYTES, "block maxima behind the slabs");
        float* bm_lds = reinterpret_cast<float*>(ring + 8 * 32 * EPI_W * 4);
        tile_epilogue_knn<4, 2, 4>(a, acc, reinterpret_cast<float*>(ring), bm_lds, m0, n0, wm, wn, wid, lane, m0 + BM <= a.m && n0 + BN <= a.n);
        tile_store_blockmax<BM, 4>(a, bm_lds, m0, n0, tid, 512);
    } else {
        tile_epilogue<4, 2>(a, acc, reinterpret_cast<float*>(ring), m0, n0, wm, wn, wid, lane, m0 + BM <= a.m && n0 + BN <= a.n);
    }
#endif
#endif
}

