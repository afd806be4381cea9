// flow_share.h -- how a joined estimator pass of a flow session (flow_engine.hip) shares the two operators whose launch used to decide
// a row's bits: the segment table of one tfm_ffn_fused launch over the rows of all batches, and the grouping of the batches whose
// astts_op_gemm may run as one launch.  Plain integer arithmetic on top of gemm_plan.h: no HIP call, no allocation, so that a host-only
// program (tests/host/flow_share_plan_main.cpp) drives it under the sanitizers.
//
// tfm_ffn_fused: a workgroup owns a 32-row tile and starts its sum over the hidden chunks at chunk (tile / 8) % chunks, the tile
// counted from the launch's first one.  A segment is one batch's rows; its tiles are counted from the segment's own first tile, the last
// one is partial, and no tile spans two segments: every row runs the instruction sequence it runs when its batch is launched alone.
//
// astts_op_gemm: gemm_plan() chooses kernel family and tile from the row count.  Consecutive batches whose plans FOR THEIR OWN ROW COUNTS
// are equal run as one launch of that plan over the rows of all of them (launch_gemm's plan_m); a row's sum does not depend on
// where its tile lies, only on the kernel.  The m <= 32 skinny family keeps its rows in LDS and never serves more than it was planned
// for: such a batch stays alone.
#pragma once
#include <cstdint>

#include "flow_session.h"
#include "gemm_plan.h"

namespace astts {

static constexpr int kFfnTileRows = 32;

// One tfm_ffn_fused launch over n row segments (passed to the kernel by value).  Segment s owns tiles [tile0[s], tile0[s + 1]) of the
// launch and rows [row0[s], row0[s] + rows[s]) of the operands.
struct FfnSegTable {
    int n = 0;
    unsigned tile0[FlowSessionPlan::kSlots] = {};
    int64_t row0[FlowSessionPlan::kSlots] = {};
    int64_t rows[FlowSessionPlan::kSlots] = {};
};

// -> the launch's tile count, or 0 when the segments are not 1 .. kSlots non-empty row ranges in ascending order without overlap (an
// in-place launch reads a tile's rows before it writes them, which is only safe while no other tile holds the same rows)
static inline int64_t ffn_seg_table(int n, const int64_t* row0, const int64_t* rows, FfnSegTable* out) {
    if (n < 1 || n > FlowSessionPlan::kSlots || !row0 || !rows) return 0;
    FfnSegTable t;
    t.n = n;
    int64_t tiles = 0, end = 0;
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 1 || row0[i] < end) return 0;
        t.tile0[i] = (unsigned)tiles;
        t.row0[i] = row0[i];
        t.rows[i] = rows[i];
        tiles += (rows[i] + kFfnTileRows - 1) / kFfnTileRows;
        end = row0[i] + rows[i];
        if (tiles > (int64_t)0x7fffffff) return 0;
    }
    if (out) *out = t;
    return tiles;
}

// what a workgroup computes from its index (the kernel's own lookup, kept here for the host test): its segment, the tile's rows
// [m0, mend) and the seed of its chunk rotation
struct FfnTile {
    int seg;
    int64_t m0, mend;
    unsigned rot_seed;
};

static inline FfnTile ffn_tile_of(const FfnSegTable& t, unsigned block) {
    int s = 0;
    for (int i = 1; i < FlowSessionPlan::kSlots; ++i)
        if (i < t.n && block >= t.tile0[i]) s = i;
    const unsigned j = block - t.tile0[s];
    const int64_t m0 = t.row0[s] + (int64_t)kFfnTileRows * j, end = t.row0[s] + t.rows[s];
    return FfnTile{s, m0, m0 + kFfnTileRows < end ? m0 + kFfnTileRows : end, j >> 3};
}

// do two plans launch the same kernel the same way?  (Skinny plans are never equal: the family cannot be shared.)
static inline bool gemm_plans_share(const GemmPlan& a, const GemmPlan& b) {
    if (a.kind != b.kind || a.kind == ASTTS_GEMM_KIND_SKINNY) return false;
    return a.kind != ASTTS_GEMM_KIND_RING || a.tile == b.tile;
}

// may the kernel planned for plan_m rows be launched over m rows?  The skinny family holds the rows it was planned for in LDS.
static inline bool gemm_plan_serves(const GemmPlan& p, int64_t m) { return p.kind != ASTTS_GEMM_KIND_SKINNY || m <= 32; }

// The launches of one astts_op_gemm over the rows of n batches laid out one after the other: group g is batches
// [first[g], first[g] + count[g]), launched once over their rows with the plan of plan_m[g] rows (a member's own row count).
struct GemmGroups {
    int n = 0;
    int first[FlowSessionPlan::kSlots] = {}, count[FlowSessionPlan::kSlots] = {};
    int64_t plan_m[FlowSessionPlan::kSlots] = {};
};

// `shape`: what gemm_plan reads of the call, m aside; rows[i]: the GEMM rows of batch i.  share == false: one group per batch.
static inline GemmGroups gemm_share_groups(GemmShape shape, int n, const int64_t* rows, bool share) {
    GemmGroups g;
    GemmPlan cur;
    for (int i = 0; i < n && i < FlowSessionPlan::kSlots; ++i) {
        shape.m = rows[i];
        const GemmPlan p = gemm_plan(shape);
        if (share && g.n > 0 && gemm_plans_share(cur, p)) {
            g.count[g.n - 1] += 1;
            continue;
        }
        g.first[g.n] = i;
        g.count[g.n] = 1;
        g.plan_m[g.n] = rows[i];
        g.n += 1;
        cur = p;
    }
    return g;
}

}  // namespace astts
