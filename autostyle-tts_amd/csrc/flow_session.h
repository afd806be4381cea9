// flow_session.h -- bookkeeping of a flow session (flow_engine.hip: astts_flow_session_*): which slot a batch holds, which Euler step
// it is at, which sequences of a joined estimator pass are its own.  Plain integer arithmetic: no HIP call, no allocation, so that a
// host-only program (tests/host/flow_session_plan_main.cpp) drives it under the sanitizers.
//
// A session is ONE chain of estimator passes that up to kSlots batches of the same frame count `t` share.  The estimator keeps no
// state between Euler steps except each batch's own x, so the sequences of a pass are laid out afresh for every pass: the active slots in
// slot order, each as its 2 b sequences (guided half, then unguided half), without gaps.  A batch that ends frees its slot and its rows
// at once; nothing has to move.
#pragma once
#include <cstdint>

namespace astts {

struct FlowSlot {
    int active;
    int b;                  // guided rows of the batch (2 b sequences of a pass)
    int n_steps, step;      // Euler steps of its solve; index of the next one (0 .. n_steps)
    int seq0;               // first sequence of the batch in the pass laid out last (layout())
};

enum { FLOW_SESSION_OK = 0, FLOW_SESSION_ERR_ARG = -1, FLOW_SESSION_ERR_T = -2, FLOW_SESSION_ERR_FULL = -3, FLOW_SESSION_ERR_ROWS = -4,
       FLOW_SESSION_ERR_STEPS = -5 };

struct FlowSessionPlan {
    static constexpr int kSlots = 4;
    int t = 0, n_slots = 0, rows_max = 0, steps_max = 0;
    FlowSlot s[kSlots] = {};

    int init(int t_, int n_slots_, int rows_max_, int steps_max_) {
        if (t_ < 2 || n_slots_ < 1 || n_slots_ > kSlots || rows_max_ < 1 || steps_max_ < 1) return FLOW_SESSION_ERR_ARG;
        t = t_;
        n_slots = n_slots_;
        rows_max = rows_max_;
        steps_max = steps_max_;
        for (FlowSlot& x : s) x = FlowSlot{};
        return FLOW_SESSION_OK;
    }

    int n_active() const {
        int n = 0;
        for (int i = 0; i < n_slots; ++i) n += s[i].active;
        return n;
    }
    int rows_active() const {
        int n = 0;
        for (int i = 0; i < n_slots; ++i) n += s[i].active ? s[i].b : 0;
        return n;
    }

    // can a batch of `b` rows and `bt` frames be admitted now?  -> the slot it would take, or FLOW_SESSION_ERR_*
    int admissible(int b, int bt, int n_steps) const {
        if (b < 1 || bt < 2 || n_steps < 1) return FLOW_SESSION_ERR_ARG;
        if (bt != t) return FLOW_SESSION_ERR_T;
        if (n_steps > steps_max) return FLOW_SESSION_ERR_STEPS;
        if (b > rows_max - rows_active()) return FLOW_SESSION_ERR_ROWS;
        for (int i = 0; i < n_slots; ++i)
            if (!s[i].active) return i;
        return FLOW_SESSION_ERR_FULL;
    }

    int admit(int b, int bt, int n_steps) {
        const int slot = admissible(b, bt, n_steps);
        if (slot < 0) return slot;
        s[slot] = FlowSlot{1, b, n_steps, 0, 0};
        return slot;
    }

    // lay out the next pass: every active slot gets its sequence range, in slot order, without gaps -> sequences of the pass
    int layout() {
        int seq = 0;
        for (int i = 0; i < n_slots; ++i) {
            if (!s[i].active) continue;
            s[i].seq0 = seq;
            seq += 2 * s[i].b;
        }
        return seq;
    }

    // after one issued pass: -> bit mask of the slots whose solve is complete (they are retired: slot and rows are free)
    unsigned advance() {
        unsigned done = 0;
        for (int i = 0; i < n_slots; ++i) {
            if (!s[i].active) continue;
            if (++s[i].step >= s[i].n_steps) {
                s[i].active = 0;
                done |= 1u << i;
            }
        }
        return done;
    }
};

}  // namespace astts
