// CPU harness for the step start of a lane that knows its call site's trace interval (abr_lane_jump.h: lanej_begin_step_at,
// lanej_site_next, lanej_site_reached; abr_tick_tables.h: avail_j) against the search that defines the result
// (lanej_begin_step).
//
// Every lane runs its decisions twice, side by side:
//   * the GENERAL lane takes lanej_begin_step at every decision and nothing else.  It alone says which call sites
//     buffer_full moved: those that are not max(completing tick + 1, avail_tick[chunk + 1]);
//   * the FAST lane takes lanej_begin_step_at, told its call site's interval the way the role-split kernels' download side is
//     (abr_env_roles.h: role_d_pre forms the next call site and its interval, role_d_validate gives it up where the player or
//     lanej_predict_next_call says another tick), with launches of `fuse` decisions whose first one searches.  The
//     one-thread-per-lane kernels' classification (lanej_site_reached on lanej_wait_call's word) is computed next to it
//     and must agree.
// At every decision the fast lane's StepStart and cursor are compared, field by field, with lanej_begin_step on a copy of the
// cursor, and the two lanes' player state with each other.
// Built two ways by tests/test_step_start_cpu.py: as a shared library (helpers.native_harness), and with -DSTEP_START_MAIN as
// a stand-alone program (the sanitizer build) that replays a built-in set of configurations.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

using namespace abrx;

enum {
    kDecisions = 0,    // decisions taken (each by both lanes)
    kMismatch,         // fields that differ between the fast path and the search, or between the two lanes' states
    kSearched,         // decisions the fast lane sent to the search
    kFirst,            // first decisions of a launch
    kMoved,            // decisions, not first of a launch, whose call site buffer_full moved (the general lane's word)
    kDisagree,         // decisions the download side and the one-thread classification would start differently
    kAvailJBad,        // entries of avail_j that break its definition
    kTimedOut,         // lanes that ran into max_ticks
    kRearms,           // episodes re-armed under auto_reset
    kCaseA,            // decisions started from "the tick after the completing one"
    kCaseB,            // decisions started from "the chunk became available"
    kFarBehind,        // decisions at which the search found the cursor more than kCatch intervals behind
    kWrapMod,          // decisions at which the trace position took the `%` branch of trace_wrap
    kStats
};

template <class TB>
static void fill(TB &t, const TickTables &tt, double L, double max_buffer, double start_up_length, int32_t V, int32_t max_ticks) {
    t.G = tt.G.data(); t.interval_tick = tt.interval_tick.data(); t.avail_tick = tt.avail_tick.data();
    t.avail_j = tt.avail_j.data();
    t.L = L; t.sd = tt.sd; t.max_buffer = max_buffer; t.start_up_length = start_up_length;
    t.V = V; t.max_ticks = max_ticks;
    t.drain = make_drain_tab(tt.sd, max_buffer + L);     // as abr_env_create does
}

// avail_j against its definition: the j with interval_tick[j] <= avail_tick[c] < interval_tick[j + 1]; -1 exactly where
// avail_tick holds INT_MAX (or the two interval ends after j would lie outside interval_tick: never in these tables)
static int64_t check_avail_j(const TickTables &tt) {
    int64_t bad = 0;
    if (tt.avail_j.size() != tt.avail_tick.size()) return 1 + (int64_t)tt.avail_tick.size();
    for (size_t c = 0; c < tt.avail_tick.size(); c++) {
        const int32_t k = tt.avail_tick[c], j = tt.avail_j[c];
        if (k == INT_MAX) { bad += j != -1; continue; }
        if (j < 0 || (size_t)j + 2 >= tt.interval_tick.size()) { bad++; continue; }
        bad += !(tt.interval_tick[j] <= k && k < tt.interval_tick[j + 1]);
    }
    return bad;
}

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

struct LaneRun {
    const double *traces; const int64_t *trace_off; const int32_t *trace_len;
    int32_t n_traces, tid0, offset0, resample;
};

static void arm(LaneJ &s, const LaneRun &r, int32_t episode) {
    // a re-arm may move the lane to another trace and offset, as the episode sampler does
    const int32_t tid = r.resample ? (r.tid0 + 7 * episode) % r.n_traces : r.tid0;
    const int32_t off = r.resample ? r.offset0 + 13 * episode : r.offset0;
    s.cur.trace = r.traces + r.trace_off[tid]; s.cur.tlen = r.trace_len[tid];
    cursor_init(s.cur, off);
}

template <class TB>
static void lane(const TB &t, const LaneRun &r, const double *ladder, const int32_t *actions, int32_t n_steps, int32_t fuse,
                 int32_t auto_reset, int64_t *st_out) {
    LaneJ g, f;                               // the general lane and the fast one
    for (LaneJ *s : {&g, &f}) {
        s->sd = t.sd; s->pt = 0.0; s->pl_left = 0; s->play_id = 0; s->pt_sum = 0.0; s->lane = 0;
        lanej_init_player(*s, t);
        arm(*s, r, 0);
    }
    if (!lanej_wait_call(g, t) | !lanej_wait_call(f, t)) { st_out[kTimedOut]++; return; }
    int32_t episode = 0;
    int32_t d_k = f.k, d_site = kSiteSearch;  // the download side's next call site and its interval
    int32_t p_site = kSiteSearch;             // the one-thread kernels' classification of the same call site
    bool moved = false;                       // the general lane's word on the call site it stands at
    for (int32_t step = 0; step < n_steps; step++) {
        const bool first = step % fuse == 0;
        // ---- role_d_begin / role_d_validate: a launch's first decision, and a call site that is not the one formed ----
        if (first || d_k != f.k) d_site = kSiteSearch;
        if (first) p_site = kSiteSearch;
        st_out[kDisagree] += (d_site < 0) != (p_site < 0) || (d_site >= 0 && d_site != p_site);
        st_out[kDecisions]++;
        st_out[kFirst] += first;
        st_out[kMoved] += !first && moved;
        st_out[kSearched] += d_site < 0;
        // ---- the general lane ----
        const int32_t gk0 = g.k;
        const StepStart gs = lanej_begin_step(g.cur, t, g.k, g.chunk_id);
        // ---- the fast lane, against the search on a copy of its cursor ----
        Cursor cc = f.cur;
        {
            st_out[kFarBehind] += f.k >= t.interval_tick[cc.j + 1 + kCatch];
            st_out[kWrapMod] += d_site >= 0 && f.cur.tpos + (d_site - f.cur.j) >= 2 * f.cur.tlen;
        }
        const StepStart ref = lanej_begin_step(cc, t, f.k, f.chunk_id);
        const StepStart fs = lanej_begin_step_at(f.cur, t, f.k, f.chunk_id, d_site);
        const int32_t avail_j_next = t.avail_j[f.chunk_id + 1];
        int64_t mm = 0;
        mm += bits(fs.c) != bits(ref.c); mm += bits(fs.bw_next) != bits(ref.bw_next);
        mm += fs.ke != ref.ke; mm += fs.ke_next != ref.ke_next; mm += fs.tn != ref.tn;
        mm += fs.avail_next != ref.avail_next; mm += f.cur.j != cc.j; mm += f.cur.tpos != cc.tpos;
        // ... and against the general lane, which never took the fast path
        mm += f.cur.j != g.cur.j; mm += f.cur.tpos != g.cur.tpos; mm += f.k != g.k; mm += bits(f.buf) != bits(g.buf);
        mm += bits(fs.c) != bits(gs.c); mm += fs.ke != gs.ke;
        st_out[kMismatch] += mm;

        const int a = actions[step];
        const double target = ladder[a] * t.L;
        const Download gd = lanej_download(g.cur, t, gs, g.k, target);
        const StepResult gr = lanej_after_download(g, t, gd, gs.avail_next, a);
        const double buf0 = f.buf; const bool su0 = f.su, be0 = f.be; const int32_t k0 = f.k;
        const Download fd = lanej_download(f.cur, t, fs, f.k, target);
        int32_t how;
        const StepResult fr = lanej_after_download(f, t, fd, fs.avail_next, a, &how);
        st_out[kMismatch] += bits(fd.dl) != bits(gd.dl) || fd.n_dl != gd.n_dl || fd.hit != gd.hit || fr.ended != gr.ended ||
                             fr.timeout != gr.timeout || bits(fr.bw) != bits(gr.bw);
        if (gr.timeout || fr.timeout) { st_out[kTimedOut]++; return; }
        // the general lane alone: did buffer_full move the call site it now stands at?
        moved = !gr.ended && g.k != (gk0 + gd.n_dl > gs.avail_next ? gk0 + gd.n_dl : gs.avail_next);
        // ---- role_d_pre: where the next download starts if nothing gates it, and the interval of that tick ----
        const int32_t k_done = k0 + fd.n_dl;
        d_k = k_done > fs.avail_next ? k_done : fs.avail_next;
        d_site = k_done >= fs.avail_next ? lanej_site_next(f.cur, fd) : avail_j_next;
        st_out[kCaseA] += !fr.ended && k_done >= fs.avail_next;
        st_out[kCaseB] += !fr.ended && k_done < fs.avail_next;
        // ---- the one-thread kernels: from the tick the player stopped at ----
        p_site = lanej_site_reached(how, f.cur, fd, t.avail_j[f.chunk_id]);      // (lanej_download_and_wait_site)
        if (fr.ended) {
            if (!auto_reset) return;
            episode++;
            st_out[kRearms]++;
            for (LaneJ *s : {&g, &f}) { lanej_init_player(*s, t); arm(*s, r, episode); }
            d_k = t.avail_tick[0]; d_site = t.avail_j[0];                      // role_d_pre's re-arm
            if (!lanej_wait_call(g, t) | !lanej_wait_call(f, t)) { st_out[kTimedOut]++; return; }
            p_site = f.k == t.avail_tick[0] ? t.avail_j[0] : kSiteSearch;      // env_jump_kernel's re-arm
            moved = g.k != t.avail_tick[0];
        } else if (f.chunk_id > 0 && lanej_gate_possible(buf0, su0, be0, fd.n_dl, t)) {
            // ---- role_d_validate: buffer_full in reach at the completing tick -> the exact call site instead ----
            int32_t kn;
            if (lanej_predict_next_call(buf0, k0, fd.n_dl, fs.avail_next, t, kn)) {
                if (kn != d_k) d_site = kSiteSearch;
                d_k = kn;
            }
        }
    }
}

extern "C" {

// n_lanes lanes of n_steps decisions each in launches of `fuse`; actions [n_lanes][n_steps].  proven: the no-speeds tables
// (TablesT<false>, whose download does not wait for the look-ahead's last load) instead of the general ones.
// Returns 0, or -1 on bad arguments; stats[kStats] as the enum above.
int64_t ss_run(double interval, double L, double speed, int32_t V, double max_buffer, double start_up_length, int32_t max_ticks,
               const double *ladder, int32_t n_rates, int32_t auto_reset, int32_t resample, const double *traces,
               const int64_t *trace_off, const int32_t *trace_len, int32_t n_traces, const int32_t *trace_id, const int32_t *offset,
               const int32_t *actions, int32_t n_lanes, int32_t n_steps, int32_t fuse, int32_t proven, int64_t *stats) {
    if (fuse < 1 || n_rates < 1 || n_traces < 1) return -1;
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    const TickTables tt = build_tick_tables(interval, L, speed, V, max_ticks, n_iv);
    for (int i = 0; i < kStats; i++) stats[i] = 0;
    stats[kAvailJBad] = check_avail_j(tt);
    if (proven && !chains_proven(tt.interval_tick.data(), tt.interval_tick.size(), max_ticks, tt.sd, L, max_buffer, ladder, n_rates))
        return -1;
    TablesT<false> tp;
    Tables tc;
    fill(tp, tt, L, max_buffer, start_up_length, V, max_ticks);
    fill(tc, tt, L, max_buffer, start_up_length, V, max_ticks);
    tc.per_lane_speed = false; tc.speed_rows = 0; tc.speed_stride = 0; tc.speeds = nullptr;
    for (int32_t i = 0; i < n_lanes; i++) {
        if (trace_id[i] < 0 || trace_id[i] >= n_traces || offset[i] < 0) return -1;
        const LaneRun r{traces, trace_off, trace_len, n_traces, trace_id[i], offset[i], resample};
        if (proven) lane(tp, r, ladder, actions + (size_t)i * n_steps, n_steps, fuse, auto_reset, stats);
        else lane(tc, r, ladder, actions + (size_t)i * n_steps, n_steps, fuse, auto_reset, stats);
    }
    return 0;
}
int32_t ss_n_stats() { return kStats; }
int32_t ss_catch() { return kCatch; }
}

#ifdef STEP_START_MAIN
// A built-in replay: seeded traces and actions over the configurations of tests/test_step_start_cpu.py in small.  Prints
// "ok <decisions> <searched>" and exits 0 when nothing differs and the search took exactly the decisions it must.
int main() {
    const double ladder[6] = {0.3, 0.75, 1.2, 1.85, 2.85, 4.3};
    uint64_t lcg = 2024;
    auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33); };
    struct Cfg { double interval, max_buffer, lo, hi; int32_t V, max_ticks, tlen_lo, tlen_hi, fuse, proven; };
    const Cfg cfgs[] = {
        {1.0, 20.0, 0.2, 6.0, 48, 0, 200, 400, 48, 1},        // the bench shape in small
        {0.3, 20.0, 0.05, 0.4, 8, 0, 40, 300, 11, 1},         // starved: many intervals per wait
        {0.5, 5.0, 3.0, 9.0, 8, 0, 40, 300, 11, 0},           // buffer_full gates often
        {0.7, 4.5, 3.0, 9.0, 8, 0, 40, 300, 5, 1},
        {0.3, 20.0, 0.3, 6.0, 8, 0, 1, 3, 11, 0},             // traces shorter than the look-ahead
        {1.0, 20.0, 0.2, 6.0, 8, 0, 1, 90, 7, 1},             // mixed lengths
        {1.0, 20.0, 0.05, 0.3, 8, 3600, 30, 90, 11, 0},       // lanes time out
    };
    int64_t decisions = 0, searched = 0;
    for (const Cfg &c : cfgs) {
        const int32_t n_traces = 5, n_lanes = 60, n_steps = 3 * c.V + 5;
        const int32_t mt = c.max_ticks ? c.max_ticks : 32 * c.V * 400;
        std::vector<double> tr;
        std::vector<int64_t> toff;
        std::vector<int32_t> tlen;
        for (int q = 0; q < n_traces; q++) {
            const int32_t n = c.tlen_lo + (int32_t)(rnd() % (uint32_t)(c.tlen_hi - c.tlen_lo + 1));
            toff.push_back((int64_t)tr.size()); tlen.push_back(n);
            for (int i = 0; i < n; i++) tr.push_back(c.lo + (c.hi - c.lo) * (double)(rnd() % 10000) / 10000.0);
        }
        std::vector<int32_t> tid(n_lanes), off(n_lanes), act((size_t)n_lanes * n_steps);
        for (int i = 0; i < n_lanes; i++) { tid[i] = (int32_t)(rnd() % n_traces); off[i] = (int32_t)(rnd() % 1000); }
        for (auto &v : act) v = (int32_t)(rnd() % 6);
        int64_t st[kStats];
        const int64_t rc = ss_run(c.interval, 4.0, 1.0, c.V, c.max_buffer, 4.0, mt, ladder, 6, 1, 1, tr.data(), toff.data(),
                                  tlen.data(), n_traces, tid.data(), off.data(), act.data(), n_lanes, n_steps, c.fuse, c.proven, st);
        if (rc != 0 || st[kMismatch] || st[kDisagree] || st[kAvailJBad] || st[kSearched] != st[kFirst] + st[kMoved] ||
            st[kDecisions] == 0) {
            printf("interval %g max_buffer %g: rc %lld, %lld decisions, %lld mismatches, %lld disagreements, %lld bad avail_j, "
                   "searched %lld, first %lld, moved %lld\n", c.interval, c.max_buffer, (long long)rc, (long long)st[kDecisions],
                   (long long)st[kMismatch], (long long)st[kDisagree], (long long)st[kAvailJBad], (long long)st[kSearched],
                   (long long)st[kFirst], (long long)st[kMoved]);
            return 1;
        }
        decisions += st[kDecisions]; searched += st[kSearched];
    }
    printf("ok %lld %lld\n", (long long)decisions, (long long)searched);
    return 0;
}
#endif
