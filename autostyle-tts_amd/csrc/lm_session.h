// lm_session.h -- bookkeeping of a decode session (lm_engine.hip: astts_lm_session_*): which rows and which arena positions a
// group of rows owns, how many steps may run before something changes, when the arena is rebased.  Plain integer arithmetic: no HIP
// call, no allocation, so that a host-only program (tests/host/lm_session_plan_main.cpp) drives it under the sanitizers.
//
// A session is ONE decode chain that up to two groups of rows share.  All rows of the chain are at the same ABSOLUTE position `pos` (the
// arena row the next forward pass writes); a group that joins a running chain has its prefix keys placed at [pos - pos0, pos) and its
// first valid key raised by the same shift, which changes none of its sums (lm_step.hip: lm_attn addresses keys and position rows
// relative to the query and splits the key range from the row's first valid key).
//
// Arena rule: no group's window (prefix + steps - 1 keys) is longer than half() = t_arena / 2.  The chain starts at pos = half() and is
// rebased back to pos = half() when it reaches t_arena: every live window [pos - w, pos), w <= half(), then moves to [half() - w,
// half()), which cannot overlap its source, and a joiner's prefix (<= half() keys) always fits below the chain position.
#pragma once
#include <cstdint>

namespace astts {

struct SessionGroup {
    int active;
    int row0, rows;         // rows [row0, row0 + rows) of the arena and the workspace
    int pos0, n_steps;      // prefix length; steps of its decode
    int step;               // index of the next token it samples (0 .. n_steps)
    int win_start;          // arena position of its prefix key 0 (= shift of its positions and of its key_start)
};

enum { SESSION_OK = 0, SESSION_ERR_ARG = -1, SESSION_ERR_WINDOW = -2, SESSION_ERR_FULL = -3, SESSION_ERR_ROWS = -4 };

struct SessionPlan {
    static constexpr int kGroups = 2;
    int rows_max = 0, t_arena = 0;
    int pos = 0;            // absolute position of the chain (meaningful while a group is active)
    SessionGroup g[kGroups] = {};

    int half() const { return t_arena / 2; }
    int n_active() const { return g[0].active + g[1].active; }

    int init(int rows_max_, int t_arena_) {
        if (rows_max_ < 1 || rows_max_ > 32 || t_arena_ < 4) return SESSION_ERR_ARG;
        rows_max = rows_max_;
        t_arena = t_arena_;
        pos = 0;
        g[0] = g[1] = SessionGroup{};
        return SESSION_OK;
    }

    // can a group of `rows` rows with this window be admitted now?  -> the slot it would take, or SESSION_ERR_*
    int admissible(int rows, int pos0, int n_steps, int* row0_out = nullptr) const {
        if (rows < 1 || pos0 < 1 || n_steps < 1) return SESSION_ERR_ARG;
        if (rows > rows_max) return SESSION_ERR_ROWS;
        if ((int64_t)pos0 + n_steps - 1 > half()) return SESSION_ERR_WINDOW;
        const int slot = !g[0].active ? 0 : (!g[1].active ? 1 : -1);
        if (slot < 0) return SESSION_ERR_FULL;
        int row0 = 0;
        if (n_active() == 1) {            // beside the running group, without a gap: above it, else below it
            const SessionGroup& o = g[1 - slot];
            if (o.row0 + o.rows + rows <= rows_max) row0 = o.row0 + o.rows;
            else if (rows <= o.row0) row0 = o.row0 - rows;
            else return SESSION_ERR_ROWS;
        }
        if (row0_out) *row0_out = row0;
        return slot;
    }

    // -> slot (0 / 1) or SESSION_ERR_*.  The group's prefix key j then lives at arena position win_start + j.
    int admit(int rows, int pos0, int n_steps) {
        int row0 = 0;
        const int slot = admissible(rows, pos0, n_steps, &row0);
        if (slot < 0) return slot;
        if (n_active() == 0) pos = half();
        g[slot] = SessionGroup{1, row0, rows, pos0, n_steps, 0, pos - pos0};
        return slot;
    }

    // the rows one launch set covers: from the lowest active row to the highest (admissible() puts a joiner directly against the
    // running group, so two active groups never leave a gap).  With `survivors_only` only the groups that still run a forward pass
    // after sampling at their step index `step + ahead`.
    bool cover(int* row0, int* rows, int ahead = 0, bool survivors_only = false) const {
        int lo = rows_max, hi = 0;
        for (const SessionGroup& x : g) {
            if (!x.active || (survivors_only && x.step + ahead + 1 >= x.n_steps)) continue;
            lo = x.row0 < lo ? x.row0 : lo;
            hi = x.row0 + x.rows > hi ? x.row0 + x.rows : hi;
        }
        if (hi <= lo) return false;
        *row0 = lo;
        *rows = hi - lo;
        return true;
    }

    bool needs_rebase() const { return n_active() > 0 && pos >= t_arena; }

    // steps that can be issued as one range: no group ends before the last of them and no position passes the arena
    int quantum(int k) const {
        if (n_active() == 0 || k < 1) return 0;
        int q = k;
        for (const SessionGroup& x : g)
            if (x.active && x.n_steps - x.step < q) q = x.n_steps - x.step;
        if (t_arena - pos < q) q = t_arena - pos;
        return q < 0 ? 0 : q;
    }

    // after `q` issued steps: -> bit mask of the slots whose decode is complete (they are retired)
    unsigned advance(int q) {
        unsigned done = 0;
        for (int i = 0; i < kGroups; ++i) {
            if (!g[i].active) continue;
            g[i].step += q;
            if (g[i].step >= g[i].n_steps) {
                g[i].active = 0;
                done |= 1u << i;
            }
        }
        pos += q;
        return done;
    }

    struct Rebase { int src0, n, delta; };     // arena positions [src0, src0 + n) move down by delta
    // the chain goes back to pos = half(); source and destination are disjoint (checked: n == 0 and delta == 0 when they would not be)
    Rebase rebase() {
        Rebase r{0, 0, 0};
        if (n_active() == 0) return r;
        int lo = pos;
        for (const SessionGroup& x : g)
            if (x.active && x.win_start < lo) lo = x.win_start;
        const int delta = pos - half();
        if (delta <= 0 || lo - delta < 0 || pos - delta > lo) return r;      // would leave the arena / overlap: not a legal state
        r = Rebase{lo, pos - lo, delta};
        for (SessionGroup& x : g)
            if (x.active) x.win_start -= delta;
        pos -= delta;
        return r;
    }
};

}  // namespace astts
