// Drives what a joined flow pass shares (autostyle-tts_amd/csrc/flow_share.h: no HIP): the segment table of the one tfm_ffn_fused
// launch and the grouping of the batches whose astts_op_gemm runs as one launch, for every slot occupancy of a session and uneven
// row counts.  Host-only: built with -fsanitize=address,undefined and run directly by tests/test_flow_share_cpu.py; every row access
// goes through a vector the sanitizer guards, every invariant through CHECK.  Exit status 0 = all held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../autostyle-tts_amd/csrc/flow_share.h"

using namespace astts;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

namespace {

struct Rng {
    uint64_t s;
    int below(int n) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((s >> 33) % (uint64_t)n);
    }
};

long g_tables = 0, g_tiles = 0, g_groupings = 0, g_shared = 0;

// the segment table of n row ranges: tiles cover every segment's rows exactly once, no tile spans two segments, and every tile has the
// rows and the rotation seed it has when its segment is launched alone from tile 0
void check_table(int n, const int64_t* row0, const int64_t* rows) {
    FfnSegTable t;
    const int64_t tiles = ffn_seg_table(n, row0, rows, &t);
    CHECK(tiles > 0 && t.n == n);
    int64_t want_tiles = 0, end = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(t.tile0[i] == (unsigned)want_tiles && t.row0[i] == row0[i] && t.rows[i] == rows[i]);
        want_tiles += (rows[i] + 31) / 32;
        end = row0[i] + rows[i];
    }
    CHECK(tiles == want_tiles);
    std::vector<int> owner((size_t)end, -1);          // -1: in no segment (a gap), else the segment
    std::vector<int> hits((size_t)end, 0);
    for (int i = 0; i < n; ++i)
        for (int64_t r = 0; r < rows[i]; ++r) owner.at((size_t)(row0[i] + r)) = i;
    for (int64_t b = 0; b < tiles; ++b) {
        const FfnTile w = ffn_tile_of(t, (unsigned)b);
        CHECK(w.seg >= 0 && w.seg < n);
        const int64_t j = b - t.tile0[w.seg];
        CHECK(j >= 0 && j < (rows[w.seg] + 31) / 32);                                  // a tile of its own segment
        CHECK(w.m0 == row0[w.seg] + 32 * j);                                           // ... at the rows it has alone: 32 j of the segment
        CHECK(w.mend > w.m0 && w.mend - w.m0 <= 32 && w.mend <= row0[w.seg] + rows[w.seg]);
        CHECK(w.mend == w.m0 + 32 || w.mend == row0[w.seg] + rows[w.seg]);             // partial only as the segment's last tile
        CHECK(w.rot_seed == (unsigned)(j >> 3));                                       // ... with the rotation it has alone
        for (int64_t r = w.m0; r < w.mend; ++r) {
            CHECK(owner.at((size_t)r) == w.seg);                                       // no tile spans two segments
            hits.at((size_t)r) += 1;
        }
        g_tiles += 1;
    }
    for (size_t r = 0; r < hits.size(); ++r) CHECK(hits[r] == (owner[r] >= 0 ? 1 : 0));     // every row exactly once, gaps never
    g_tables += 1;
}

void table_refusals() {
    FfnSegTable t;
    const int64_t r0[5] = {0, 64, 128, 192, 256}, rn[5] = {64, 64, 64, 64, 64};
    CHECK(ffn_seg_table(0, r0, rn, &t) == 0);
    CHECK(ffn_seg_table(5, r0, rn, &t) == 0);                       // more than kSlots
    CHECK(ffn_seg_table(2, nullptr, rn, &t) == 0 && ffn_seg_table(2, r0, nullptr, &t) == 0);
    const int64_t overlap0[2] = {0, 63};
    CHECK(ffn_seg_table(2, overlap0, rn, &t) == 0);                 // the second range starts inside the first
    const int64_t desc0[2] = {64, 0};
    CHECK(ffn_seg_table(2, desc0, rn, &t) == 0);
    const int64_t empty[2] = {64, 0};
    CHECK(ffn_seg_table(2, r0, empty, &t) == 0);
    const int64_t neg0[1] = {-32};
    CHECK(ffn_seg_table(1, neg0, rn, &t) == 0);
    const int64_t huge[1] = {((int64_t)1 << 36) + 1};
    CHECK(ffn_seg_table(1, r0, huge, &t) == 0);                     // more tiles than a grid has
    CHECK(ffn_seg_table(4, r0, rn, nullptr) == 8);                  // the count alone
}

// the estimator's GEMM shapes (what gemm_plan reads of them, m aside)
std::vector<GemmShape> shapes() {
    std::vector<GemmShape> v;
    GemmShape conv;                 // ResNet / resampling convolution: fp32 rows, n = 256, K = 3 x 256
    conv.n = 256; conv.cin = conv.cin_pad = 256; conv.taps = 3; conv.plain = false;
    v.push_back(conv);
    GemmShape first = conv;         // the first down block's ResNet: 320 input channels
    first.cin = 320; first.cin_pad = 320;
    v.push_back(first);
    GemmShape up = conv;            // phase-decomposed ConvTranspose1d
    up.n = 512; up.taps = 2;
    v.push_back(up);
    GemmShape fin;                  // the final projection onto the mel bins: plain fp32 rows (m <= 32 is the skinny family)
    fin.n = 80; fin.cin = fin.cin_pad = 256;
    v.push_back(fin);
    GemmShape qkv;                  // q|k|v projection of the unfused attention path: fp16 rows, the ring kernels
    qkv.n = 1536; qkv.cin = qkv.cin_pad = 256; qkv.x_f16 = true; qkv.out_f16 = true;
    v.push_back(qkv);
    GemmShape w1 = qkv;             // feed-forward W1 of the unfused path
    w1.n = 512;
    v.push_back(w1);
    GemmShape off = qkv;            // ring kernels switched off
    off.ring_mode = kRingModeOff;
    v.push_back(off);
    return v;
}

// the grouping of n batches: groups are contiguous and cover the batches in order, plans inside a group are equal (to the plan of
// plan_m, a member's own row count), neighbouring groups differ, and the planned kernel serves the group's rows
void check_groups(const GemmShape& base, int n, const int64_t* rows) {
    auto plan_of = [&](int64_t m) {
        GemmShape s = base;
        s.m = m;
        return gemm_plan(s);
    };
    const GemmGroups g = gemm_share_groups(base, n, rows, true);
    CHECK(g.n >= 1 && g.n <= n);
    int next = 0;
    for (int k = 0; k < g.n; ++k) {
        CHECK(g.first[k] == next && g.count[k] >= 1 && g.first[k] + g.count[k] <= n);
        const GemmPlan p = plan_of(g.plan_m[k]);
        bool member = false;
        int64_t total = 0;
        for (int i = 0; i < g.count[k]; ++i) {
            const int64_t m = rows[g.first[k] + i];
            member = member || m == g.plan_m[k];
            total += m;
            const GemmPlan q = plan_of(m);
            if (g.count[k] > 1) CHECK(gemm_plans_share(p, q));              // equal plans, never the skinny family
            else CHECK(p.kind == q.kind);
        }
        CHECK(member);
        CHECK(gemm_plan_serves(p, total));
        if (k + 1 < g.n) CHECK(!gemm_plans_share(p, plan_of(rows[g.first[k + 1]])));     // maximal: the next batch could not have joined
        next += g.count[k];
        g_shared += g.count[k] > 1;
    }
    CHECK(next == n);
    const GemmGroups alone = gemm_share_groups(base, n, rows, false);     // the switch off: one launch per batch, its own plan
    CHECK(alone.n == n);
    for (int i = 0; i < n; ++i) CHECK(alone.first[i] == i && alone.count[i] == 1 && alone.plan_m[i] == rows[i]);
    g_groupings += 1;
}

void serves() {
    GemmShape s;
    s.n = 256; s.cin = s.cin_pad = 256;
    s.m = 32;
    const GemmPlan sk = gemm_plan(s);
    CHECK(sk.kind == ASTTS_GEMM_KIND_SKINNY);
    CHECK(gemm_plan_serves(sk, 32) && gemm_plan_serves(sk, 7) && !gemm_plan_serves(sk, 33) && !gemm_plan_serves(sk, 64));
    CHECK(!gemm_plans_share(sk, sk));
    s.m = 33;
    const GemmPlan tile = gemm_plan(s);
    CHECK(tile.kind != ASTTS_GEMM_KIND_SKINNY && gemm_plan_serves(tile, (int64_t)1 << 30) && gemm_plans_share(tile, tile));
    // two one-row batches at one frame... (2 rows each): skinny, never grouped
    const int64_t tiny[3] = {2, 2, 2};
    const GemmGroups g = gemm_share_groups(s, 3, tiny, true);
    CHECK(g.n == 3);
    // 6 144 + 6 144 rows of the k = 3 convolution: T64K128 each, one group planned for 6 144 (the total alone would be T128X64)
    GemmShape conv = shapes()[0];
    const int64_t two[2] = {6144, 6144};
    const GemmGroups c = gemm_share_groups(conv, 2, two, true);
    CHECK(c.n == 1 && c.count[0] == 2 && c.plan_m[0] == 6144);
    conv.m = 6144;
    CHECK(gemm_plan(conv).kind == ASTTS_GEMM_KIND_T64K128);
    conv.m = 12288;
    CHECK(gemm_plan(conv).kind == ASTTS_GEMM_KIND_T128X64);
    // 6 144 | 12 288 | 12 288 | 6 144: the middle two share, the outer ones stay alone
    const int64_t four[4] = {6144, 12288, 12288, 6144};
    const GemmGroups f = gemm_share_groups(shapes()[0], 4, four, true);
    CHECK(f.n == 3 && f.count[0] == 1 && f.first[1] == 1 && f.count[1] == 2 && f.plan_m[1] == 12288 && f.first[2] == 3);
}

// every occupancy of the four slots, the batches' rows uneven: the pass the session lays out -> segment table and groupings
void occupancies(uint64_t seed) {
    Rng r{seed};
    const std::vector<GemmShape> sh = shapes();
    const int ts[] = {2, 33, 64, 97, 225, 344, 375};
    for (int t : ts)
        for (int mask = 1; mask < 1 << FlowSessionPlan::kSlots; ++mask)
            for (int rep = 0; rep < 6; ++rep) {
                FlowSessionPlan plan;
                CHECK(plan.init(t, FlowSessionPlan::kSlots, 32, 10) == FLOW_SESSION_OK);
                int left = 32;
                for (int i = 0; i < FlowSessionPlan::kSlots; ++i) {
                    if (!((mask >> i) & 1) || left < 1) continue;
                    const int b = rep == 0 ? (left < 8 ? left : 8) : 1 + r.below(left < 12 ? left : 12);
                    plan.s[i] = FlowSlot{1, b, 10, r.below(10), 0};
                    left -= b;
                }
                const int nseq = plan.layout();
                int n = 0;
                int64_t row0[FlowSessionPlan::kSlots], rows[FlowSessionPlan::kSlots], rows_half[FlowSessionPlan::kSlots];
                const int t_half = (t - 1) / 2 + 1;
                for (int i = 0; i < FlowSessionPlan::kSlots; ++i) {
                    if (!plan.s[i].active) continue;
                    row0[n] = (int64_t)plan.s[i].seq0 * t;
                    rows[n] = 2 * (int64_t)plan.s[i].b * t;
                    rows_half[n] = 2 * (int64_t)plan.s[i].b * t_half;
                    ++n;
                }
                CHECK(n >= 1 && row0[n - 1] + rows[n - 1] == (int64_t)nseq * t);       // the pass's rows, without gaps
                check_table(n, row0, rows);
                for (const GemmShape& s : sh) {
                    check_groups(s, n, rows);
                    check_groups(s, n, rows_half);
                }
            }
}

}  // namespace

int main() {
    table_refusals();
    serves();
    // the operator test's tables: 9 + 33 + 1 tiles from rows 0 / 283 / 1332, whole tiles, one segment; with gaps
    {
        const int64_t a0[3] = {0, 283, 1332}, an[3] = {283, 1049, 1};
        check_table(3, a0, an);
        const int64_t b0[2] = {0, 512}, bn[2] = {512, 640};
        check_table(2, b0, bn);
        const int64_t c0[1] = {0}, cn[1] = {970};
        check_table(1, c0, cn);
        const int64_t d0[3] = {0, 288, 1342};
        check_table(3, d0, an);
        const int64_t e0[1] = {77};
        check_table(1, e0, cn);
    }
    occupancies(0x5eedull);
    CHECK(g_shared > 0);
    std::printf("flow_share_plan: ok (%ld tables, %ld tiles, %ld groupings, %ld shared groups)\n", g_tables, g_tiles, g_groupings, g_shared);
    return 0;
}
