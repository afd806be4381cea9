// gemm_plan.h -- what the GEMM launcher (ops_gemm.hip) runs for a call: the kernel family, the ring tile, the skinny kernel's split-K and
// row passes, the workgroup tile of gemm_rows.  Pure functions of a shape, plain integer arithmetic: no HIP call, no allocation, no
// lock, so that a host-only program (tests/host/gemm_plan_main.cpp) prints the plan of a list of shapes and tests/test_gemm_plan_cpu.py
// compares it with the recorded one (tests/golden/gemm_plan.txt): a changed threshold shows as the shapes that moved.
//
// launch_gemm builds a GemmShape from its arguments, asks gemm_plan() and switches on the answer; astts_op_gemm_kernel_kind and
// gemm_scan_blockmax_ok ask the same function, astts_op_gemm_rows asks gemm_rows_plan().
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/astts.h"

namespace astts {

static inline int64_t plan_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What the decision reads of a call.
// plain: taps == 1, stride == 1, pad == 0, t_in == t_out, no row lengths; x_aligned: fp16 x at a 16-byte aligned address with lda % 8 == 0
// (the LDS-DMA staging of the ring kernels); ring_mode: the ring switch in force (astts_op_gemm_set_ring_mode over ASTTS_GEMM_RING; -1: the
// rule, 0 switches the ring kernels off, above: that tile forced).
struct GemmShape {
    int64_t m = 1;               // B * t_out
    int n = 1, cin = 64, cin_pad = 64, taps = 1;
    bool plain = true, x_f16 = false, out_f16 = false, x_aligned = true;
    bool blockmax = false;       // the kNN scan's block-maximum epilogue is asked for (GemmArgs::blockmax)
    bool gather = false;         // skinny extras present: row gather, LayerNorm prologue, split-K workspace
    bool ln = false;
    bool splitk_ws = false;
    int ring_mode = -1;
    bool no_splitk = false;      // ASTTS_NO_SPLITK is set
};

// The tiles of gemm_ring / gemm_ring8: block rows x block columns, ring depth.
enum class RingTile : int {
    T128x128_S2,       // gemm_ring<2, 2, 2>: two stages
    T128x64_S2,        // gemm_ring<2, 1, 2>: two stages (wide outputs)
    T64x64_S4,         // gemm_ring<1, 1, 4>: four stages (n <= 256)
    T256x256_1B,       // gemm_ring<4, 2, 2, 4, 8>: eight waves, two stages, one barrier per K tile
    T256x256_8P,       // gemm_ring8: the same tile on the eight-phase schedule
};

// The public numbers of astts_op_gemm_set_ring_mode / ASTTS_GEMM_RING -> tile; nothing else knows them.
// (A switch above the table, which only the environment can set, has always run the 64 x 64 tile.)
static constexpr int kRingModeAuto = -1, kRingModeOff = 0, kRingModeMax = 5;
static inline RingTile ring_tile_of_mode(int mode) {
    switch (mode) {
        case 1: return RingTile::T128x128_S2;
        case 2: return RingTile::T128x64_S2;
        case 4: return RingTile::T256x256_1B;
        case 5: return RingTile::T256x256_8P;
        default: return RingTile::T64x64_S4;   // 3
    }
}

struct GemmPlan {
    int kind = ASTTS_GEMM_KIND_T64K64;          // ASTTS_GEMM_KIND_*
    RingTile tile = RingTile::T64x64_S4;        // RING: the tile that is launched
    // SKINNY: K slices, rows of x per pass (pass p takes rows [p * rows, min(m, (p + 1) * rows)) with MT = skinny_mt(its rows)), XV of
    // every pass, the K elements of a slice; fits: false = even one row's LDS image is too large (the call is invalid)
    int ksplit = 1, rows = 0, xv = 4, kslice = 0;
    bool fits = true;
};

// the skinny kernel's dynamic LDS: the fp16 image of m rows of a K slice (16-byte skew per row) + the waves' reduction buffer
static constexpr int kSkinnyWaves = 8;
static constexpr size_t kSkinnyLdsMax = 160 * 1024;
static inline int skinny_mt(int rows) { return rows <= 16 ? 1 : 2; }
static inline size_t skinny_lds_bytes(int m, int cin_pad, int mt) {
    return (((size_t)m * (cin_pad + 8) * 2 + 15) & ~(size_t)15) + (size_t)kSkinnyWaves * mt * 4 * 64 * sizeof(float);
}

// Which kernel family serves a contraction (ASTTS_GEMM_KIND_*).
static inline int gemm_kernel_kind(const GemmShape& s) {
    if (s.m <= 32 && s.plain && !s.x_f16 && !s.out_f16) return ASTTS_GEMM_KIND_SKINNY;
    // fp16 activations, plain GEMM, whole 64-wide K tiles: the LDS-DMA ring kernel
    if (s.plain && s.x_f16 && s.cin == s.cin_pad && s.x_aligned && s.m >= 64 && s.n > 32 && s.ring_mode != kRingModeOff) return ASTTS_GEMM_KIND_RING;
    auto blocks = [&](int bm, int bn) { return plan_cdiv(s.m, bm) * plan_cdiv(s.n, bn); };
    const int64_t want = 384;  // >= 1.5 blocks per CU
    // K tile: cin_pad is a multiple of 64, so 64 never straddles a tap; 128 needs cin_pad % 128 == 0
    const bool k128 = (s.cin_pad % 128) == 0 && s.taps * s.cin_pad >= 256;
    if (s.n <= 32) return ASTTS_GEMM_KIND_T32;
    if (s.n > 64 && blocks(128, 128) >= want) return ASTTS_GEMM_KIND_T128;   // measured: the 128x128 tile is fastest at BK=32 (2+ blocks/CU, small K)
    if (blocks(128, 64) >= want) return ASTTS_GEMM_KIND_T128X64;
    return k128 ? ASTTS_GEMM_KIND_T64K128 : ASTTS_GEMM_KIND_T64K64;
}

// The ring tile the rule gives a shape (no switch forced).
static inline RingTile ring_tile_by_rule(const GemmShape& s) {
    auto blocks = [&](int bm, int bn) { return plan_cdiv(s.m, bm) * plan_cdiv(s.n, bn); };
    // Tile choice, measured IN SITU (scripts/flow_only.py; the back-to-back micro-benchmark runs on L2-hot weights and ranks
    // the deep-K tiles differently).  Wide outputs (K = 256: four K tiles) take two-stage rings -- 48 KB of LDS puts three
    // blocks on a CU and the overlap of one block's epilogue with its neighbours' loads beats a deeper ring (16 -> 12 us);
    // the n <= 256 projections (K = 512 / 1024 from cold weights) keep the 4-stage 64x64 ring.
    //   1: 128x128 x2 (once there are >= 4-8 tiles per CU)   2: 128x64 x2 (wide outputs)   3: 64x64 x4 (n <= 256)   4: 256x256 x2, 8 waves
    const int64_t b128 = blocks(128, 128);
    // (deep K with enough tiles -- the kNN scan as a GEMM, K = 6144: 128 x 128 measured 727 us per 256-query search against 797 for
    // 128 x 64 and 906 for 64 x 64, profiles/r05_knn_gemm_ab.log)
    // 4: 256 x 256 with eight waves (two stages = 128 KB, one block per CU).  The ring kernels are bound by the bytes a CU can keep in
    // flight (latency x rate, against the LDS left beside the tile being multiplied): 128 x 128 holds 2 blocks x 32 KB for 2.1 MFLOP
    // each, 256 x 256 holds 64 KB for 8.4 MFLOP.  scripts/ring_shapes.py, TFLOP/s 128 x 128 -> 256 x 256: 15 360 x 3072 x 5120 (the
    // embedder's q|k|v) 807 -> 1025, 15 360 x 8192 x 3072 832 -> 1037, 23 680 x 1024 x 4096 700 -> 916, the kNN scan 256 x 6144 x 100k
    // 639 -> 796; needs more than a round of blocks (86 blocks: 349 against 548) and deep K (the flow's K = 256 projections at 44 032
    // rows: 532 against 463 back to back, but the 64-sequence flow solve measured 123.8 ms with it and 121.0 without).
    // Round 6: the rule's 256 x 256 tile runs on the eight-phase schedule (gemm_ring8: bit-identical results, +8-10 % -- alternating
    // A/B in one process, scripts/ring_ab.py, profiles/r06_ring8_ab.log: 8192^3 1066 -> 1171, 15 360 x 3072 x 5120 1005 -> 1087,
    // the kNN scan 783 -> 861 TFLOP/s on N(0, 1) operands; on zero-filled operands 1425 -> 1667, i.e. what is left is the clock the
    // chip holds under fp16 MFMA load on real data (1.71 GHz measured, GRBM_GUI_ACTIVE), not the schedule).
    // Round 6, with the eight-phase kernel and the grouped tile order (alternating A/B of tiles 1 / 2 / 5 on 17 embedder, prefill and
    // frontend shapes, profiles/r06_ring_rule_ab.log): what decides for the 256 x 256 tile is how full its LAST round of 256 blocks is
    // -- 180 or 235 blocks (one round, 0.70 / 0.92 full) win by 10-19 % at K >= 3072, 264, 300 or 516 blocks (0.52 - 0.67) lose by 7-47 % --
    // and shallow K needs a fuller round (K = 1024-1280: wins at 0.92, even at 0.87, loses at 0.70); below it 128 x 128 beats 128 x 64
    // on every deep-K shape with >= 256 tiles (the K = 256 projections of the flow keep their in-situ rule).
    const int64_t b256 = blocks(256, 256);
    const int64_t fill_pct = b256 * 100 / (plan_cdiv(b256, 256) * 256);          // how full the rounds of 256 x 256 tiles are
    // the rule's 256 x 256 tile is the eight-phase kernel; a FORCED 4 keeps the one-barrier form (A/B, tests)
    if (s.n > 128 && ((s.cin_pad >= 2048 && fill_pct >= 68) || (s.cin_pad >= 1024 && fill_pct >= 85))) return RingTile::T256x256_8P;
    if (b128 >= (s.n >= 512 ? 2048 : 1024) || (s.cin_pad >= 4096 && b128 >= 512) || (s.cin_pad >= 1024 && s.n >= 512 && b128 >= 256))
        return RingTile::T128x128_S2;
    if (s.n >= 512 && blocks(128, 64) >= 160) return RingTile::T128x64_S2;
    return RingTile::T64x64_S4;
}

// The ring tile that is LAUNCHED: the rule's or the forced one, the block-maximum override, and what a tile wider than the output
// degrades to (a forced 128 x 128 at n <= 64 runs 128 x 64; a forced 256 x 256 at n <= 128 runs 128 x 128 in the one-barrier form's
// place -- 64 x 64 at n <= 64 -- and 64 x 64 in the eight-phase form's).
static inline RingTile ring_tile_launched(const GemmShape& s) {
    RingTile t = s.ring_mode > kRingModeOff ? ring_tile_of_mode(s.ring_mode) : ring_tile_by_rule(s);
    // (the block maxima are per 64 columns of a wave: the tiles with TN = 2)
    if (s.blockmax && t != RingTile::T256x256_1B && t != RingTile::T256x256_8P) t = RingTile::T128x128_S2;
    switch (t) {
        case RingTile::T256x256_8P: return s.n > 128 ? t : RingTile::T64x64_S4;
        case RingTile::T256x256_1B: return s.n > 128 ? t : s.n > 64 ? RingTile::T128x128_S2 : RingTile::T64x64_S4;
        case RingTile::T128x128_S2: return s.n > 64 ? t : RingTile::T128x64_S2;
        default: return t;
    }
}

static inline GemmPlan gemm_plan(const GemmShape& s) {
    GemmPlan p;
    p.kind = gemm_kernel_kind(s);
    if (p.kind == ASTTS_GEMM_KIND_RING) p.tile = ring_tile_launched(s);
    if (p.kind == ASTTS_GEMM_KIND_SKINNY) {
        // the block keeps its m rows of x as an fp16 image in LDS: rows are taken in chunks that fit 160 KB
        // (only m > 16 with K > 2048 needs two passes, e.g. the FFN-out projection of a 32-row decode group)
        // split-K (workspace given): deep, narrow GEMMs (the FFN-out projection: K = 4096 onto 1024 columns = 64 column
        // blocks) are cut into 4 K slices so that 256 workgroups stream the weights instead of 64
        const int lines_tot = s.cin_pad >> 6;
        if (s.splitk_ws && !s.no_splitk && !s.gather && !s.ln && lines_tot >= 32 && lines_tot % 32 == 0 && (s.n + 15) / 16 <= 128) p.ksplit = 4;
        p.kslice = s.cin_pad / p.ksplit;
        p.rows = (int)s.m;
        while (p.rows > 1 && skinny_lds_bytes(p.rows, p.kslice, skinny_mt(p.rows)) > kSkinnyLdsMax) p.rows = p.rows > 16 ? 16 : p.rows / 2;
        p.fits = skinny_lds_bytes(p.rows, p.kslice, 1) <= kSkinnyLdsMax;
        p.xv = p.kslice <= 1024 ? 4 : 16;   // row of <= 4 float4 per lane: a quarter of the staging registers
    }
    return p;
}

// gemm_rows: PL (K lines per wave and pass: one pass when the fragments fit the registers; fp32 rows hold twice the registers) and the
// workgroup tile (16 RT) x (16 CT): the fattest one (fewest re-reads of the activation rows) that still gives every CU a workgroup
struct RowsPlan {
    int pl, rt, ct;
};

static inline RowsPlan gemm_rows_plan(int64_t m, int n, int k, bool x_f16) {
    const int per_wave = (k / 64 + 7) / 8;
    const int pl = per_wave <= 2 ? 2 : (per_wave <= 4 || !x_f16) ? 4 : 8;
    auto blocks = [&](int rt, int ct) { return plan_cdiv(m, 16 * rt) * plan_cdiv(n, 16 * ct); };
    if (pl <= 2 && blocks(4, 2) >= 256) return {pl, 4, 2};
    if (pl <= 4 && blocks(2, 2) >= 256) return {pl, 2, 2};
    return {pl, 2, 1};
}

}  // namespace astts
