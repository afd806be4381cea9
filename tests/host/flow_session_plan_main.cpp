// Drives the flow session's bookkeeping (autostyle-tts_amd/csrc/flow_session.h: no HIP) through admit / step / finish sequences
// against a model pass that records WHICH batch owns every sequence of every pass.  Host-only: built with -fsanitize=address,undefined
// and run directly by tests/test_flow_session_cpu.py; every sequence access goes through a vector the sanitizer guards, every
// invariant through CHECK.  Exit status 0 = all sequences held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../autostyle-tts_amd/csrc/flow_session.h"

using astts::FlowSessionPlan;
using astts::FlowSlot;

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

struct Model {
    FlowSessionPlan plan;
    int uid[FlowSessionPlan::kSlots] = {};
    int steps_done[FlowSessionPlan::kSlots] = {};
    int next_uid = 1;
    long passes = 0, joined = 0, finished = 0;

    // one pass: lay out, check that the sequence ranges tile [0, nseq) without overlap, advance
    unsigned pass() {
        const int nseq = plan.layout();
        CHECK(nseq == 2 * plan.rows_active());
        CHECK(nseq >= 2 && nseq <= 2 * plan.rows_max);
        std::vector<int> owner((size_t)nseq, 0);
        int n = 0;
        for (int i = 0; i < plan.n_slots; ++i) {
            const FlowSlot& x = plan.s[i];
            if (!x.active) continue;
            ++n;
            CHECK(x.step == steps_done[i] && x.step < x.n_steps);
            for (int j = 0; j < 2 * x.b; ++j) {
                CHECK(owner.at((size_t)(x.seq0 + j)) == 0);      // never two batches on one sequence
                owner.at((size_t)(x.seq0 + j)) = uid[i];
            }
        }
        for (int v : owner) CHECK(v != 0);                       // no gap
        passes += 1;
        joined += n > 1;
        const unsigned done = plan.advance();
        for (int i = 0; i < plan.n_slots; ++i) {
            if (uid[i] == 0) continue;
            steps_done[i] += 1;
            const bool ended = steps_done[i] >= plan.s[i].n_steps;
            CHECK(((done >> i) & 1u) == (ended ? 1u : 0u));
            if (ended) {
                CHECK(!plan.s[i].active);                        // the slot is free at once
                uid[i] = 0;
                steps_done[i] = 0;
                finished += 1;
            }
        }
        return done;
    }

    int admit(int b, int t, int n_steps) {
        const int want = plan.admissible(b, t, n_steps);
        const int rows_before = plan.rows_active();
        const int slot = plan.admit(b, t, n_steps);
        CHECK(slot == want);
        if (slot >= 0) {
            CHECK(slot < plan.n_slots && uid[slot] == 0);
            CHECK(plan.rows_active() == rows_before + b && plan.rows_active() <= plan.rows_max);
            uid[slot] = next_uid++;
            steps_done[slot] = 0;
        } else {
            CHECK(plan.rows_active() == rows_before);
        }
        return slot;
    }
};

void fixed_cases() {
    Model m;
    CHECK(m.plan.init(1, 4, 32, 10) == astts::FLOW_SESSION_ERR_ARG);
    CHECK(m.plan.init(64, 0, 32, 10) == astts::FLOW_SESSION_ERR_ARG);
    CHECK(m.plan.init(64, 5, 32, 10) == astts::FLOW_SESSION_ERR_ARG);
    CHECK(m.plan.init(64, 4, 0, 10) == astts::FLOW_SESSION_ERR_ARG);
    CHECK(m.plan.init(64, 4, 32, 10) == astts::FLOW_SESSION_OK);
    CHECK(m.plan.n_active() == 0 && m.plan.layout() == 0 && m.plan.advance() == 0u);
    // refusals: bad arguments, another frame count, too many steps, rows, slots
    CHECK(m.admit(0, 64, 4) == astts::FLOW_SESSION_ERR_ARG);
    CHECK(m.admit(8, 65, 4) == astts::FLOW_SESSION_ERR_T);
    CHECK(m.admit(8, 64, 11) == astts::FLOW_SESSION_ERR_STEPS);
    CHECK(m.admit(33, 64, 4) == astts::FLOW_SESSION_ERR_ROWS);
    CHECK(m.admit(8, 64, 4) == 0);
    CHECK(m.admit(8, 64, 4) == 1);
    CHECK(m.admit(8, 64, 2) == 2);
    CHECK(m.admit(9, 64, 4) == astts::FLOW_SESSION_ERR_ROWS);      // 24 + 9 > 32
    CHECK(m.admit(8, 64, 4) == 3);
    CHECK(m.admit(1, 64, 4) == astts::FLOW_SESSION_ERR_ROWS);      // rows are checked before slots: 32 rows are in use
    CHECK(m.pass() == 0u);
    CHECK(m.pass() == 1u << 2);                                    // the two-step batch ends: slot 2 and its rows are free at once
    CHECK(m.admit(9, 64, 4) == astts::FLOW_SESSION_ERR_ROWS);
    CHECK(m.admit(8, 64, 10) == 2);                                // a third batch takes the slot a finished one freed
    CHECK(m.admit(1, 64, 1) == astts::FLOW_SESSION_ERR_ROWS);
    CHECK(m.pass() == 0u);
    CHECK(m.pass() == (1u | 1u << 1 | 1u << 3));
    CHECK(m.plan.n_active() == 1 && m.plan.layout() == 16 && m.plan.s[2].seq0 == 0);   // the survivor's sequences start at 0 again
    // four one-row batches in 4 slots: the fifth is refused for slots, not rows
    Model f;
    CHECK(f.plan.init(33, 4, 32, 10) == astts::FLOW_SESSION_OK);
    for (int i = 0; i < 4; ++i) CHECK(f.admit(1, 33, 3) == i);
    CHECK(f.admit(1, 33, 3) == astts::FLOW_SESSION_ERR_FULL);
    // a batch admitted at another's last step
    Model l;
    CHECK(l.plan.init(40, 2, 8, 4) == astts::FLOW_SESSION_OK);
    CHECK(l.admit(3, 40, 4) == 0);
    for (int i = 0; i < 3; ++i) CHECK(l.pass() == 0u);
    CHECK(l.admit(1, 40, 4) == 1);
    CHECK(l.pass() == 1u);
    for (int i = 0; i < 2; ++i) CHECK(l.pass() == 0u);
    CHECK(l.pass() == 2u && l.plan.n_active() == 0);
}

void random_runs(uint64_t seed, int rounds) {
    Rng r{seed};
    for (int run = 0; run < rounds; ++run) {
        Model m;
        const int t = 2 + r.below(400), n_slots = 1 + r.below(FlowSessionPlan::kSlots), rows_max = 1 + r.below(64), steps_max = 1 + r.below(32);
        CHECK(m.plan.init(t, n_slots, rows_max, steps_max) == astts::FLOW_SESSION_OK);
        for (int ev = 0; ev < 400; ++ev) {
            if (r.below(3) == 0) {
                const int bt = r.below(8) == 0 ? t + 1 : t;
                m.admit(1 + r.below(rows_max + 2), bt, 1 + r.below(steps_max + 1));
            } else if (m.plan.n_active() > 0) {
                m.pass();
            }
        }
        while (m.plan.n_active() > 0) m.pass();
        CHECK(m.plan.rows_active() == 0 && m.plan.layout() == 0);
        CHECK(m.finished == (long)m.next_uid - 1);
    }
}

}  // namespace

int main() {
    fixed_cases();
    random_runs(0x5eedull, 300);
    std::puts("flow_session_plan: ok");
    return 0;
}
