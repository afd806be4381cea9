// Drives the decode session's bookkeeping (autostyle-tts_amd/csrc/lm_session.h: no HIP) through admit / step / retire / rebase
// sequences against a model arena that records WHICH key of WHICH group every (position, row) cell holds.  Host-only: built with
// -fsanitize=address,undefined and run directly by tests/test_lm_session_plan_cpu.py; every cell access goes through a vector the
// sanitizer guards, every invariant through CHECK.  Exit status 0 = all sequences held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../autostyle-tts_amd/csrc/lm_session.h"

using astts::SessionGroup;
using astts::SessionPlan;

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

struct Cell { int uid, key; };

struct Model {
    SessionPlan plan;
    std::vector<Cell> arena;           // [t_arena][rows_max]
    int uid[2] = {0, 0};
    int next_uid = 1;
    long steps = 0, rebases = 0, joins = 0, two_active_rebases = 0;

    Cell& at(int t, int row) {
        CHECK(t >= 0 && t < plan.t_arena && row >= 0 && row < plan.rows_max);
        return arena.at((size_t)t * plan.rows_max + row);
    }

    void init(int rows_max, int t_arena) {
        CHECK(plan.init(rows_max, t_arena) == astts::SESSION_OK);
        arena.assign((size_t)t_arena * rows_max, Cell{0, 0});
    }

    // what lm_kv_admit does: prefix key j of every row -> arena position win_start + j
    int admit(int rows, int pos0, int n_steps) {
        const int before = plan.n_active();
        const int expect = plan.admissible(rows, pos0, n_steps);
        const int slot = plan.admit(rows, pos0, n_steps);
        CHECK(slot == expect);
        if (slot < 0) return slot;
        const SessionGroup& g = plan.g[slot];
        CHECK(g.active && g.rows == rows && g.row0 >= 0 && g.row0 + rows <= plan.rows_max && g.step == 0);
        CHECK(g.win_start >= 0 && g.win_start + pos0 == plan.pos);
        if (before == 1) {                 // side by side with the running group: no overlap, no gap
            const SessionGroup& o = plan.g[1 - slot];
            CHECK(g.row0 + g.rows == o.row0 || o.row0 + o.rows == g.row0);
            ++joins;
        } else {
            CHECK(plan.pos == plan.half() && g.row0 == 0);
        }
        uid[slot] = next_uid++;
        for (int j = 0; j < pos0; ++j)
            for (int r = 0; r < rows; ++r) at(g.win_start + j, g.row0 + r) = Cell{uid[slot], j};
        return slot;
    }

    // every live window holds its group's keys 0 .. n - 1 in order, where the attention will read them: [win_start, pos)
    void check_windows() {
        for (int i = 0; i < 2; ++i) {
            const SessionGroup& g = plan.g[i];
            if (!g.active) continue;
            CHECK(g.win_start >= 0 && plan.pos - g.win_start == g.pos0 + g.step);
            CHECK(plan.pos - g.win_start <= plan.half());
            for (int t = g.win_start; t < plan.pos; ++t)
                for (int r = 0; r < g.rows; ++r) {
                    const Cell c = at(t, g.row0 + r);
                    CHECK(c.uid == uid[i] && c.key == t - g.win_start);
                }
        }
    }

    // what astts_lm_session_step does with k
    unsigned step(int k) {
        unsigned done = 0;
        int left = k;
        while (left > 0 && plan.n_active() > 0) {
            if (plan.needs_rebase()) {
                int r0 = 0, rows = 0;
                CHECK(plan.cover(&r0, &rows));
                const int active = plan.n_active();
                const SessionPlan::Rebase rb = plan.rebase();
                CHECK(rb.n > 0 && rb.delta > 0);
                CHECK(rb.src0 - rb.delta >= 0 && rb.src0 - rb.delta + rb.n <= rb.src0);      // destination below the source, disjoint
                CHECK(plan.pos == plan.half());
                for (int t = rb.src0; t < rb.src0 + rb.n; ++t)
                    for (int r = r0; r < r0 + rows; ++r) at(t - rb.delta, r) = at(t, r);
                ++rebases;
                two_active_rebases += active == 2;
                check_windows();
            }
            const int q = plan.quantum(left);
            CHECK(q >= 1 && q <= left);
            int r0 = 0, rows = 0;
            CHECK(plan.cover(&r0, &rows) && r0 >= 0 && rows >= 1 && r0 + rows <= plan.rows_max);
            for (int s = 0; s < q; ++s) {
                // the forward pass of this step writes key (pos0 + step) of every group that goes on, at position pos + s
                for (int i = 0; i < 2; ++i) {
                    const SessionGroup& g = plan.g[i];
                    if (!g.active) continue;
                    CHECK(g.step + s < g.n_steps);                                            // a range never passes a group's end
                    if (g.step + s + 1 == g.n_steps) {
                        CHECK(s == q - 1);                                                    // a group ends only on the range's last step
                        continue;
                    }
                    for (int r = 0; r < g.rows; ++r) at(plan.pos + s, g.row0 + r) = Cell{uid[i], g.pos0 + g.step + s};
                }
                int s0 = 0, srows = 0;
                if (plan.cover(&s0, &srows, s, true)) CHECK(s0 >= r0 && s0 + srows <= r0 + rows);
            }
            const SessionPlan saved = plan;
            const unsigned fin = plan.advance(q);
            for (int i = 0; i < 2; ++i)
                CHECK(((fin >> i) & 1u) == (unsigned)(saved.g[i].active && saved.g[i].step + q == saved.g[i].n_steps));
            done |= fin;
            left -= q;
            steps += q;
            check_windows();
        }
        return done;
    }
};

void scripted() {
    // two 8-row groups of the benchmark's shape, arena at its smallest: each joins in the middle of the one before and takes the slot of the one before that
    Model m;
    const int pos0 = 180, n = 250, w = pos0 + n - 1;
    m.init(16, 2 * w);
    CHECK(m.plan.admissible(8, pos0, n + 1) == astts::SESSION_ERR_WINDOW);
    CHECK(m.plan.admissible(17, pos0, n) == astts::SESSION_ERR_ROWS);
    CHECK(m.admit(8, pos0, n) == 0);
    CHECK(m.step(125) == 0u);
    CHECK(m.admit(8, pos0, n) == 1 && m.plan.g[1].row0 == 8);
    CHECK(m.plan.admissible(8, pos0, n) == astts::SESSION_ERR_FULL);
    CHECK(m.step(125) == 1u);                     // A ends, B goes on alone in rows [8, 16)
    int r0 = 0, rows = 0;
    CHECK(m.plan.cover(&r0, &rows) && r0 == 8 && rows == 8);
    CHECK(m.admit(8, pos0, n) == 0 && m.plan.g[0].row0 == 0);
    CHECK(m.step(125) == 2u);                     // B ends; D takes its rows
    CHECK(m.admit(8, pos0, n) == 1 && m.plan.g[1].row0 == 8);
    CHECK(m.step(1000) == 3u);                    // runs to the end of both, through a rebase with two groups active
    CHECK(m.plan.n_active() == 0 && m.rebases >= 1 && m.two_active_rebases >= 1);
    // a single step with one group that ends and one that goes on
    Model t;
    t.init(8, 64);
    CHECK(t.admit(3, 5, 2) == 0 && t.admit(5, 9, 4) == 1);
    CHECK(t.plan.g[1].row0 == 3);
    CHECK(t.step(1) == 0u && t.step(1) == 1u && t.step(7) == 2u);
    // a smaller group beside a group that sits at the top: placed directly below it
    CHECK(t.admit(4, 3, 6) == 0 && t.admit(4, 3, 6) == 1 && t.step(6) == 3u);
    CHECK(t.admit(2, 3, 3) == 0);
    CHECK(t.admit(6, 3, 9) == 1 && t.plan.g[1].row0 == 2);
    CHECK(t.step(3) == 1u);
    CHECK(t.admit(1, 4, 2) == 0 && t.plan.g[0].row0 == 1);
    CHECK(t.admit(1, 4, 2) == astts::SESSION_ERR_FULL);
    CHECK(t.step(100) == 3u);
}

void random_runs(uint64_t seed, int rounds) {
    Rng rng{seed};
    for (int round = 0; round < rounds; ++round) {
        Model m;
        const int rows_max = 1 + rng.below(32);
        const int wmax = 2 + rng.below(60);
        m.init(rows_max, 2 * wmax + rng.below(2));         // the smallest legal arena (even or odd)
        for (int op = 0; op < 300; ++op) {
            if (rng.below(3) == 0) {
                const int rows = 1 + rng.below(rows_max);
                const int pos0 = 1 + rng.below(wmax);
                const int n_steps = 1 + rng.below(wmax - pos0 + 2);
                const int slot = m.admit(rows, pos0, n_steps);
                if (pos0 + n_steps - 1 > m.plan.half()) CHECK(slot == astts::SESSION_ERR_WINDOW);
                m.check_windows();
            } else {
                m.step(1 + rng.below(2 * wmax));
            }
        }
        m.step(1 << 20);
        CHECK(m.plan.n_active() == 0);
    }
}

}  // namespace

int main() {
    scripted();
    random_runs(1, 200);
    random_runs(0x9e3779b97f4a7c15ull, 200);
    std::puts("lm_session_plan: ok");
    return 0;
}
