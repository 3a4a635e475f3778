// abr_lane_jump.h -- one lane of the event-driven environment step (host + device).
//
// The same tick semantics as the reference's Simulator.run() loop
// (Simulator.py:135-208 under R1-R3) without visiting every tick.  A step (ABR
// call site -> next call site) is a handful of runs in which one float64
// variable receives the same constant every tick:
//   phase A  downloaded_size += bandwidth*dt, one run per trace interval, until it
//            reaches target_size at tick k_hit            (chain<STOP_GE>, :160-163)
//            meanwhile buffer_level -= speed*dt while playing, until 0
//                                                          (chain<STOP_LE>, :184,:194)
//   hit tick buffer_level = (buffer_level + L) - speed*dt, flags, start-up exit
//                                                          (:170,:184,:190-202)
//   phase B  wait for the next chunk to become available (:143): buffer_level drains
//            for avail_tick - k ticks, then until buffer_level < max_buffer when
//            buffer_full gates the download               (chain<STOP_LT>, :144,:190)
// abrx::chain executes each run in O(binades crossed) and returns the bit-identical
// float64 value of the tick-by-tick loop (abr_exact_jump.h); the integer counters
// (ticks in start-up / rebuffering / playing, and the latency integral: sum of k
// over playing ticks) have exact closed forms over a run.
//
// State between the pieces is always "post-head": T1-T3 (:137-149) of tick s.k are
// done.  A download cannot pause inside phase A: buffer_full only turns on in a tick
// that completes a chunk (buffer_level grows nowhere else), availability is
// monotone in time.
//
// Plain C++ so that tests/native can run it on the CPU against the oracle; the
// product only ever runs it inside the HIP kernels of abr_env.hip.
#ifndef ABR_LANE_JUMP_H
#define ABR_LANE_JUMP_H

#include <math.h>

#include "abr_exact_jump.h"

#ifndef ABR_STAMP
#define ABR_STAMP(n)               // cycle stamps exist only in the diagnostic build of abr_env.hip
#endif

namespace abrx {

constexpr double kTickDt = 0.01;   // Simulator.py:133
#ifndef ABR_K_DRAIN_TAIL
#define ABR_K_DRAIN_TAIL 16
#endif
constexpr int kPrologue = 16;               // (the asynchronous pipeline's own prologue: diagnostic build only)
#ifndef ABR_PCHUNKS
#define ABR_PCHUNKS 12
#endif
#ifndef ABR_PCHECK
#define ABR_PCHECK 0x892
#endif
constexpr int kPChunks = ABR_PCHUNKS;       // prologue of a download: up to 7 single additions + this many chunks of 8
constexpr int kPCheck = ABR_PCHECK;         // bit q: a checkpoint after chunk q (the last chunk's bit must be set)

// The stateless speed rule, field for field the layout of include/abr_env.h: abr_speed_rule (abr_env.hip asserts it).
struct SpeedRule {
    int32_t n_lat, n_buf;          // 0..4
    double lat_thr[4], buf_thr[4]; // strictly ascending [s]
    double speed[5][5];            // speed[i][j], i in 0..n_lat, j in 0..n_buf
};

// i = thresholds of lat reached, j = thresholds of buf reached; comparisons only, so the host, the device and a numpy twin
// give the same answer for the same inputs
ABR_HD double speed_rule_eval(const SpeedRule &r, double lat, double buf) {
    int32_t i = 0, j = 0;
    for (int32_t q = 0; q < r.n_lat; q++) i += lat >= r.lat_thr[q] ? 1 : 0;
    for (int32_t q = 0; q < r.n_buf; q++) j += buf >= r.buf_thr[q] ? 1 : 0;
    return r.speed[i][j];
}

// Tables::speed_rows of a speed rule: a "schedule" whose every row is computed (sched_begin_chunk)
constexpr int32_t kSpeedRowsRule = 0x7fffffff;

// A speed rule's block: the rule, and where its answers go (speed p of lane i to log[p * stride + i] for p < log_rows).
// In the kernels it lies in the parameter block, at byte ABR_RULE_KERNARG_OFFSET of the kernarg segment, and is read there
// only when a played chunk begins: held in Tables its pointers would be live scalars across every kernel's loop.
struct SpeedRuleBlock {
    SpeedRule rule;
    double *log;
    int32_t log_rows, reserved_;
};

// SPEEDS: whether the per-lane play-speed features (per-lane speeds, speed schedules, the speed rule) can be on at all.
// TablesT<true> is the table every caller has always filled in (`Tables`); TablesT<false> carries the tag of a build that
// has none of them: the speed fields are compile-time constants, and every lane function selects its one-speed path at
// compile time (`if constexpr` on kSpeeds), so neither the tests nor the state they guard exist in the caller's code.
template <bool SPEEDS = true>
struct TablesT;

template <>
struct TablesT<true> {
    static constexpr bool kSpeeds = true;
    static constexpr int kSettle = SETTLE_REMAINDER;   // how the chains settle a jump (abr_exact_jump.h: SettleKind)
    static constexpr int kGuards = GUARDS_CHECKED;     // who establishes the segments' guards (abr_exact_jump.h: GuardKind)
    const double *G;               // G[n] = dt added n times to 0.0 (global_time, download_time, ...)
    const int32_t *interval_tick;  // first tick k with int(G[k]/interval) >= j          (:158)
    const int32_t *avail_tick;     // first tick k with int(G[k]/chunk_length) - 1 >= c  (:143)
    const int32_t *avail_j = nullptr;   // the trace interval avail_tick[c] lies in, -1 where not known; only lanej_begin_step_at reads it
    double L, sd, max_buffer, start_up_length;
    int32_t V, max_ticks;
    bool per_lane_speed;           // each lane carries its own speed*dt and play_time (8f rank 3)
    // speed schedule (8f rank 3, second half): speed_rows >= 2 means the lane's play speed is
    // re-read at the first playing tick of every played chunk (play_length == 0, :176-177):
    // played chunk p of lane i plays at speeds[min(p, speed_rows - 1) * speed_stride + i]
    int32_t speed_rows;
    int64_t speed_stride;
    const double *speeds;
    // speed_rows == kSpeedRowsRule: the played chunk's speed is computed by a speed rule (include/abr_env.h:
    // abr_speed_rule) from the lane's state at that tick; the host harness points `rule` at its block, the kernels read
    // theirs from the kernarg segment (SpeedRuleBlock)
    const SpeedRuleBlock *rule = nullptr;
    // the per-binade cascade of buffer_level -= sd at THE one play speed (abr_exact_jump.h: drain_cascade); n == 0 with
    // per-lane speeds or when the speed / buffer range is not covered: the general chains then do the drains
    DrainTab drain;
};

template <>
struct TablesT<false> {
    static constexpr bool kSpeeds = false;
    static constexpr int kSettle = SETTLE_REMAINDER;
    // The chains of these tables run without their per-segment guards: whoever fills one in for a handle has checked
    // chains_proven() for it (below); a handle that fails runs the TablesT<true> instances, which accept the no-speed case.
    static constexpr int kGuards = GUARDS_PROVEN;
    const double *G;
    const int32_t *interval_tick;
    const int32_t *avail_tick;
    const int32_t *avail_j = nullptr;
    double L, sd, max_buffer, start_up_length;
    int32_t V, max_ticks;
    static constexpr bool per_lane_speed = false;
    static constexpr int32_t speed_rows = 0;
    static constexpr int64_t speed_stride = 0;
    static constexpr const double *speeds = nullptr;
    static constexpr const SpeedRuleBlock *rule = nullptr;
    DrainTab drain;
};

using Tables = TablesT<true>;

// The table of the three-wave kernel's speed instances: the same fields, the chains settled by three candidates
// (abr_exact_jump.h: SettleKind says why those kernels keep that form).
struct TablesCandidates : TablesT<true> {
    static constexpr int kSettle = SETTLE_CANDIDATES;
};

// The no-speeds table with the checked chains: for code that runs on ANY handle and has no TablesT<true> form to fall back
// to (the tree walks of lookahead_kernel and plan_kernel).
struct TablesChecked : TablesT<false> {
    static constexpr int kGuards = GUARDS_CHECKED;
};

// The handle's side of GUARDS_PROVEN (abr_exact_jump.h: P1-P3), checked ONCE on the host where the tick tables are built.
// With it, every chain loop of the lane functions hands chain_segment a budget in 1..kJumpCap:
//   * lanej_drain, lanej_wait_call, lanej_predict_next_call: budgets are tick counts of one episode, m <= max_ticks, and
//     the loops run while `a < m` (chain(), drain_to_zero), so each segment's budget m - a is in 1..max_ticks;
//   * lanej_download: the loop runs while kk < mt and hands over ke - kk, where ke = min(end of the cursor's interval, mt).
//     kk <= ke always (a segment performs at most its budget), and when kk == ke the trip first moves to the next interval,
//     whose end is strictly later because every interval up to the sentinel spans at least one tick: 1 <= ke - kk; and
//     ke - kk <= mt - 0.
// So: max_ticks <= kJumpCap, and interval_tick strictly increasing up to its first sentinel (the spans then are below
// 2^20 as well; the test is kept because it is what the download loop's argument reads).  P3 (finite values) for what the
// handle itself contributes: chunk_length, sd, max_buffer and ladder x chunk_length finite and below 2^960 -- buffer_level
// stays below max_buffer + chunk_length, downloaded_size below target + one tick's bytes; trace samples, a per-chunk
// bitrate table and a size table (abr_env_set_size_table: finite, > 0 and below 2^960, never read on the host) are the
// caller's finite inputs.  A handle with a size table runs the TablesT<true> instances in any case.
inline bool chains_proven(const int32_t *interval_tick, size_t n_interval_tick, int32_t max_ticks, double sd,
                          double chunk_length, double max_buffer, const double *ladder, int32_t n_rates) {
    if (max_ticks < 1 || max_ticks > kJumpCap) return false;
    for (size_t j = 0; j + 1 < n_interval_tick && interval_tick[j] != 0x7fffffff; j++) {
        if (interval_tick[j + 1] == 0x7fffffff) break;
        const int64_t span = (int64_t)interval_tick[j + 1] - interval_tick[j];
        if (span < 1 || span >= kJumpCap) return false;
    }
    const auto bounded = [](double v) { return v == v && v > -0x1p960 && v < 0x1p960; };
    if (!bounded(sd) || !bounded(chunk_length) || !bounded(max_buffer)) return false;
    for (int32_t r = 0; r < n_rates; r++)
        if (!bounded(ladder[r] * chunk_length)) return false;
    return true;
}

// Where a lane is in its bandwidth trace.  Only the download side (phase A) reads it.
struct Cursor {
    int32_t j;                     // interval index of the clock, int(global_time / interval) (:158)
    int32_t tpos;                  // (offset0 + j) mod tlen: bandwidths[idx] of that interval (:159)
    int32_t tlen;
    const double *trace;
};

struct LaneJ {
    double buf;                    // buffer_level
    double sd;                     // this lane's speed*dt (== Tables::sd unless per_lane_speed)
    double pt;                     // play_time, carried only when per_lane_speed (else GP[n_play])
    long long sumk;                // sum of tick indices of playing ticks (latency integral)
    int32_t k, chunk_id, n_su, n_rb, n_play, avail_k, last_action;
    bool su, be, bf;               // start_up, buffer_empty, buffer_full
    Cursor cur;
    // speed schedule only: playing ticks left in the current played chunk (0: the next playing
    // tick starts one and asks for its speed), chunks played so far (play_id), the sum of
    // play_time over the playing ticks (latency integral), and the lane's column in `speeds`
    int32_t pl_left, play_id;
    double pt_sum;
    int64_t lane;
};

ABR_HD void cursor_init(Cursor &c, int32_t offset0) {
    c.j = 0;                       // int(0.0 / interval)
    c.tpos = offset0 % c.tlen;
}

// Simulator.py:95-130, then T1-T3 of tick 0 (start_up_time += dt); everything but the cursor
template <class TB>
ABR_HD void lanej_init_player(LaneJ &s, const TB &t) {
    s.buf = 0.0; s.sumk = 0;
    s.k = 0; s.chunk_id = 0; s.n_su = 1; s.n_rb = 0; s.n_play = 0;
    s.last_action = -1;
    s.su = true; s.be = true; s.bf = false;
    s.avail_k = t.avail_tick[0];
    if constexpr (TB::kSpeeds) {
        s.pt = 0.0;                    // play_time = 0 (:115); s.sd is set by the caller
        s.pl_left = 0; s.play_id = 0; s.pt_sum = 0.0;      // play_length = 0, play_id = 0 (:113-114)
    }
}

template <class TB>
ABR_HD void lanej_init(LaneJ &s, const TB &t, int32_t offset0) {
    lanej_init_player(s, t);
    cursor_init(s.cur, offset0);
}

// play_time += speed*dt for `a` playing ticks (:182).  With one speed for all lanes
// play_time is the table value GP[n_play]; with per-lane speeds it is carried, advanced by
// the same exact chain machinery.
template <class TB>
ABR_HD void lanej_play(LaneJ &s, const TB &t, int32_t a) {
    if (!t.per_lane_speed || a <= 0) return;
    int32_t done = 0;
    double x = s.pt;
    // an unreachable threshold: the chain only counts
    chain<STOP_GE, 0, TB::kSettle, TB::kGuards>(x, s.sd, 1.0e300, a, done);
    s.pt = x;
}

// buffer_level -= speed*dt per playing tick (:184) for up to m ticks, stopping right after the
// first result <= 0 (:194).  Same contract as chain<STOP_LE>(b, -sd, 0.0, m, a).  Far from
// zero the exact jumps do the work; within kDrainTail ticks of zero a binade lasts only a
// few ticks (8, 4, 2, 1: one segment each), so the last stretch is plain subtractions -- the
// reference's own sequence.  The switch point affects speed only, never a result; measured
// on one MI355X box at 65 536 lanes (profiles/r02_ab_drain_tail.txt): 8-32 ticks are
// equivalent (7.3-7.4e9 env-steps/s), 64 costs 5 %, 128 costs 20 %.
// (A buffer that runs dry is the player wave's slowest case -- six segments and the whole tail, one lane in 25, so 86 % of a
// wave's decisions have one -- and only the tick it ends at is needed, not its values; but that tick cannot be had from
// real arithmetic: buffer levels are sums of chunk lengths and tick-sized subtractions, so b / sd sits within rounding of
// a whole number exactly when it matters, and which side of zero the k-th result falls on is decided by the roundings
// themselves.  Built and measured in round 5, profiles/r05_experiments_not_kept.txt.)
constexpr int kDrainTail = ABR_K_DRAIN_TAIL;
template <int SETTLE = SETTLE_REMAINDER, int GUARDS = GUARDS_CHECKED>
ABR_HD bool drain_to_zero(double &b_io, double sd, int32_t m, int32_t &a_out) {
    ChainState cs;
    cs.x = b_io; cs.eb = -1;
    const double tail = (double)kDrainTail * sd;
    int32_t a = 0;
    bool below = false;
    while (a < m && !below) a += chain_segment<STOP_LE, 0, SETTLE, GUARDS>(cs, -sd, tail, m - a, below);
    double b = cs.x;
    ABR_STAMP(24);
#ifdef ABR_DRAIN_HOOK
    const int32_t a_seg = a;
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    while (a < m && b > 0.0) { b = b - sd; a++; }
    ABR_STAMP(25);
#ifdef ABR_DRAIN_HOOK
    ABR_DRAIN_HOOK(a > 0 && b <= 0.0, a - a_seg);   // host-side analysis builds: did it run dry, ticks of the plain tail
#endif
    b_io = b; a_out = a;
    return a > 0 && b <= 0.0;
}

// The drain of the common case -- one play speed for every lane -- goes through the per-binade cascade (round 6: a stage
// is ~25 vector instructions against the ~58 of a chain segment plus its loop, and a buffer that runs dry is one pass over
// the binades instead of six segments and a 16-tick tail).  Wave-uniform choice: a lane above the cascade (never seen: it
// covers max_buffer + chunk_length) sends the whole wave through the chains.
template <class TB>
ABR_HD bool lanej_drain(const TB &t, double &b_io, double sd, int32_t m, int32_t &a_out) {
    if (t.drain.n > 0 && !wave_any(!(b_io < t.drain.top))) {
        const bool zero = drain_cascade(t.drain, sd, b_io, m, a_out);
        ABR_STAMP(24);
        return zero;
    }
    return drain_to_zero<TB::kSettle, TB::kGuards>(b_io, sd, m, a_out);
}

// ---- speed schedule: the play speed changes at played-chunk boundaries ----
// The first playing tick of a played chunk (play_length == 0) takes the chunk's speed
// (:176-177); the chunk then lasts until play_length, `speed*dt` added per tick from 0, is
// >= chunk_length (:183,:185-187): that many ticks, by the same exact chain.
// k: the tick, b: buffer_level at that point of it (after :170, before :184) -- what a speed rule reads.
template <class TB>
ABR_HD void sched_begin_chunk(LaneJ &s, const TB &t, int32_t k, double b) {
    double v;
    if (t.speed_rows == kSpeedRowsRule) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(ABR_RULE_KERNARG_OFFSET)
        // behind a compiler-only fence, so that the rule's loads stay here instead of being hoisted out of the kernel's
        // loops as live scalars (abr_env_roles.h: fresh_params)
        auto kp = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const SpeedRuleBlock &rb = *(const SpeedRuleBlock *)((const char *)kp + ABR_RULE_KERNARG_OFFSET);
#else
        const SpeedRuleBlock &rb = *t.rule;
#endif
        v = speed_rule_eval(rb.rule, t.G[k] - s.pt, b);                       // lat = instant_latency (:179)
        if (s.play_id < rb.log_rows) rb.log[(int64_t)s.play_id * t.speed_stride + s.lane] = v;
    } else {
        const int32_t row = s.play_id < t.speed_rows ? s.play_id : t.speed_rows - 1;
        v = t.speeds[(int64_t)row * t.speed_stride + s.lane];
    }
    s.sd = v * kTickDt;                                                      // play_speed * dt (:182)
    double x = 0.0;
    int32_t a = 0;
    chain<STOP_GE, 0, TB::kSettle, TB::kGuards>(x, s.sd, t.L, t.max_ticks + 1, a);
    s.pl_left = a > 0 ? a : 1;
}

// bookkeeping of `a` playing ticks inside one played chunk: play_time (exact chain), the sum of
// play_time over those ticks (real arithmetic: it only feeds average_latency), chunk boundary
template <class TB>
ABR_HD void sched_played(LaneJ &s, const TB &t, int32_t a) {
    if (a <= 0) return;
    s.pt_sum += (double)a * s.pt + s.sd * (double)(((long long)a * (a - 1)) / 2);
    int32_t done = 0;
    double x = s.pt;
    chain<STOP_GE, 0, TB::kSettle, TB::kGuards>(x, s.sd, 1.0e300, a, done);
    s.pt = x;
    s.pl_left -= a;
    if (s.pl_left == 0) s.play_id++;                                       // :185-187
}

// buffer_level -= speed*dt for up to m playing ticks, stopping right after the first result that
// is <= 0 (STOP_LE, :194) or < thr (STOP_LT, :190), one played chunk at a time
template <int STOP, class TB>
ABR_HD bool sched_drain(LaneJ &s, const TB &t, double &b, double thr, int32_t m, int32_t &a_out) {
    int32_t a_tot = 0;
    bool hit = false;
    while (a_tot < m && !hit) {
        if (s.pl_left == 0) sched_begin_chunk(s, t, s.k + a_tot, b);
        const int32_t run = (m - a_tot < s.pl_left) ? m - a_tot : s.pl_left;
        int32_t a = 0;
        if (STOP == STOP_LE) hit = drain_to_zero<TB::kSettle, TB::kGuards>(b, s.sd, run, a);
        else hit = chain<STOP_LT, 0, TB::kSettle, TB::kGuards>(b, -s.sd, thr, run, a);
        sched_played(s, t, a);
        a_tot += a;
    }
    a_out = a_tot;
    return hit;
}

// m full iterations: T4-T9 of a tick in which no chunk completes, then T1-T3 of the next
template <class TB>
ABR_HD void lanej_idle(LaneJ &s, const TB &t, int32_t m) {
    if (m <= 0) return;
    // :201-202 at the end of the first of these ticks.  A no-op everywhere (start_up implies
    // buffer_level < start_up_length once any tick has run) except right after init when
    // start_up_length <= 0: tick 0 itself counts as start-up, every later one does not.
    if (s.su && s.buf >= t.start_up_length) s.su = false;
    ABR_STAMP(23);
    if (s.su) {
        s.n_su += m;                                   // :137-138; nothing plays, buffer untouched
    } else if (s.be) {
        s.n_rb += m;                                   // :139-140; buffer stays 0
    } else {
        int32_t a = 0;
        double b = s.buf;
        bool zero;
        if constexpr (TB::kSpeeds) {
            if (t.speed_rows >= 2) zero = sched_drain<STOP_LE>(s, t, b, 0.0, m, a);
            else { zero = lanej_drain(t, b, s.sd, m, a); lanej_play(s, t, a); }   // :184,:194
        } else {
            zero = lanej_drain(t, b, t.sd, m, a);          // one speed for all lanes: play_time is GP[n_play]
        }
        s.n_play += a;
        s.sumk += (long long)a * s.k + ((long long)a * (a - 1)) / 2;
        if (zero) { b = 0.0; s.be = true; s.n_rb += (m - a + 1); }             // :195-196, then :140
        s.buf = b;
        s.bf = b >= t.max_buffer;                      // :190, as of the last tick executed
    }
    s.k += m;
}

// From a post-head state that is not downloading: advance to the next call site
// (returns true) or to max_ticks (returns false).
// how: which of lanej_begin_step_at's cases the call site is -- reached without a wait (kWaitNone), by waiting for the
// chunk to become available and for nothing else (kWaitAvail: s.k == s.avail_k), or moved by buffer_full (kWaitGated, also
// when no call site is reached)
enum { kWaitNone = 0, kWaitAvail = 1, kWaitGated = 2 };
template <class TB>
ABR_HD bool lanej_wait_call(LaneJ &s, const TB &t, int32_t *how = nullptr) {
    const int32_t mt = t.max_ticks;
    if (how) *how = kWaitNone;
    if (s.k >= s.avail_k && !s.bf) return true;
    if (how) *how = kWaitGated;
    int32_t w = s.avail_k - s.k;
    if (w < 0) w = 0;
    if (w > mt - s.k) w = mt - s.k;
    lanej_idle(s, t, w);
    if (s.k >= mt) return false;
    if (how) *how = s.bf ? kWaitGated : kWaitAvail;     // (buffer_full only ever clears during the wait: not full means w > 0)
    if (s.bf) {
        // buffer_full gates the next download (:144): drain until buffer_level < max_buffer
        if (s.su || s.be) {
            // nothing drains the buffer: the reference spins forever; run out the clock
            if (s.su) s.n_su += mt - s.k; else s.n_rb += mt - s.k;
            s.k = mt;
            return false;
        }
        int32_t a = 0;
        double b = s.buf;
        bool cleared;
        if constexpr (TB::kSpeeds) {
            if (t.speed_rows >= 2) cleared = sched_drain<STOP_LT>(s, t, b, t.max_buffer, mt - s.k, a);
            else { cleared = chain<STOP_LT, 0, TB::kSettle, TB::kGuards>(b, -s.sd, t.max_buffer, mt - s.k, a); lanej_play(s, t, a); }
        } else {
            cleared = chain<STOP_LT, 0, TB::kSettle, TB::kGuards>(b, -t.sd, t.max_buffer, mt - s.k, a);
        }
        s.n_play += a;
        s.sumk += (long long)a * s.k + ((long long)a * (a - 1)) / 2;
        s.k += a;
        s.be = b <= 0.0;
        if (s.be) { b = 0.0; s.n_rb += 1; }
        s.buf = b;
        s.bf = !cleared;
        if (!cleared) return false;
    }
    return true;
}

struct StepResult {
    double bw;        // downloaded_size / download_time of the chunk (:164), valid when hit
    bool hit;         // the chunk completed
    bool ended;       // chunk_id >= video_length (:207-208)
    bool timeout;     // ran into max_ticks
};

// Everything a step needs from memory before it can start, fetched in ONE burst of
// independent loads (a lane alone on its SIMD cannot hide a chain of dependent loads):
// phase B moved k only, so the trace cursor (j, tpos) may be up to kCatch intervals
// behind; the candidates for all those cases are loaded at once and selected in
// registers.  The caller can issue this before it computes the action.
constexpr int kCatch = 4;
constexpr int32_t kSiteSearch = -1;         // lanej_begin_step_at: the call site's interval is not known
struct StepStart {
    double c;          // bandwidth * dt of the interval the call site is in (:160)
    double bw_next;    // bandwidth of the next interval
    int32_t ke;        // end tick of the current interval
    int32_t ke_next;   // end tick of the next one
    int32_t tn;        // trace position of the next interval
    int32_t avail_next;// avail_tick[chunk_id + 1]: when the chunk after this one can start (:143)
};

ABR_HD int32_t trace_wrap(int32_t pos, int32_t tlen) {
    if (pos >= tlen) pos -= tlen;
    if (pos >= tlen) pos %= tlen;             // traces shorter than the look-ahead
    return pos;
}

// The loads of lanej_begin_step on their own, so that a caller can issue them well before it
// needs the values (the role-split kernel issues them before its workgroup barrier).
struct StepLoads {
    int32_t ke[kCatch + 2];
    double bw[kCatch + 2];
    int32_t avail_next;
};

template <class TB>
ABR_HD StepLoads lanej_begin_load(const Cursor &s, const TB &t, int32_t chunk_id) {
    StepLoads ld;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < kCatch + 2; i++) {
        ld.ke[i] = t.interval_tick[s.j + 1 + i];
        ld.bw[i] = s.trace[trace_wrap(s.tpos + i, s.tlen)];
    }
    ld.avail_next = t.avail_tick[chunk_id + 1];
    return ld;
}

// ... and the selection among them once the call-site tick k is known.  The cursor must be the
// one the loads were issued for.
template <class TB>
ABR_HD StepStart lanej_begin_select(Cursor &s, const TB &t, const StepLoads &ld, int32_t k) {
    const int32_t *ke = ld.ke;
    const double *bw = ld.bw;
    StepStart st;
    st.avail_next = ld.avail_next;
    // intervals the cursor is behind: ke[] is non-decreasing
    int32_t adv = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < kCatch; i++) adv += (k >= ke[i]) ? 1 : 0;
    if (adv == kCatch && k >= ke[kCatch]) {
        // more than kCatch intervals behind (a long buffer_full wait): walk, then reload
        s.j += kCatch; s.tpos = trace_wrap(s.tpos + kCatch, s.tlen);
        int32_t e = t.interval_tick[s.j + 1];
        while (k >= e && e != 0x7fffffff) {       // the table ends in INT_MAX sentinels
            s.j++;
            s.tpos = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
            e = t.interval_tick[s.j + 1];
        }
        st.ke = e; st.ke_next = t.interval_tick[s.j + 2];
        st.tn = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
        st.c = s.trace[s.tpos] * kTickDt; st.bw_next = s.trace[st.tn];
        return st;
    }
    // select candidate `adv` (static indices only: the arrays stay in registers)
    double c_bw = bw[0], n_bw = bw[1];
    int32_t c_ke = ke[0], n_ke = ke[1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 1; i <= kCatch; i++) {
        const bool pick = adv == i;
        c_bw = pick ? bw[i] : c_bw; n_bw = pick ? bw[i + 1] : n_bw;
        c_ke = pick ? ke[i] : c_ke; n_ke = pick ? ke[i + 1] : n_ke;
    }
    s.j += adv;
    s.tpos = trace_wrap(s.tpos + adv, s.tlen);
    st.c = c_bw * kTickDt; st.bw_next = n_bw; st.ke = c_ke; st.ke_next = n_ke;
    st.tn = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
    return st;
}

template <class TB>
ABR_HD StepStart lanej_begin_step(Cursor &s, const TB &t, int32_t k, int32_t chunk_id) {
    const StepLoads ld = lanej_begin_load(s, t, chunk_id);
    return lanej_begin_select(s, t, ld, k);
}

// The step start of a lane that KNOWS which interval its call site k lies in.  Inside a rollout that is nearly every
// decision, because a call site is reached in one of three ways:
//   A  no wait: k is the tick after the completing one.  The cursor is in k's interval already, or exactly one behind when
//      the completing tick was the last of its interval -- the download knows which (Download::j_next);
//   B  the lane waited for the chunk to become available (:143) and nothing else: k = avail_tick[c], whose interval depends
//      on the chunk alone (Tables::avail_j, abr_tick_tables.h);
//   C  anything else -- buffer_full moved the call site (:144), the first decision after the state was loaded, a call site
//      the download side took from the player or predicted: not known.
// j_site >= 0 says "interval_tick[j_site] <= k < interval_tick[j_site + 1]" (the cursor's invariant, and the caller's
// promise); the trace position follows from the cursor's, which is never ahead of k.  Then the two interval ends and the
// two samples the step uses are loaded directly: five loads with per-lane addresses in one burst, against the thirteen of
// lanej_begin_load, no candidate arrays and no select chain.  j_site < 0 (case C) is the search of lanej_begin_step, which
// defines the result; one such lane sends only itself there, behind a wave-uniform branch that the others skip.
template <class TB>
ABR_HD StepStart lanej_begin_step_at(Cursor &s, const TB &t, int32_t k, int32_t chunk_id, int32_t j_site) {
    const bool search = j_site < 0;
    const int32_t j = search ? s.j : j_site;                  // (a searching lane loads from its own cursor: in bounds, unused)
    const int32_t tp = trace_wrap(s.tpos + (j - s.j), s.tlen);
    const int32_t tn = (tp + 1 == s.tlen) ? 0 : tp + 1;
    StepStart st;
    st.ke = t.interval_tick[j + 1];
    st.ke_next = t.interval_tick[j + 2];
    st.c = s.trace[tp] * kTickDt;
    st.bw_next = s.trace[tn];
    st.tn = tn;
    st.avail_next = t.avail_tick[chunk_id + 1];
    if (wave_any(search)) {
        if (search) return lanej_begin_step(s, t, k, chunk_id);
    }
    s.j = j; s.tpos = tp;
    return st;
}

// Phase A of one decision: the download side.  Needs nothing of the player state but
// the call-site tick k: the download cannot pause before it completes, so it is a pure
// function of (k, cursor, target) -- which is what lets a second thread run the player
// side of the SAME lane concurrently (abr_env.hip: env_split_kernel).
struct Download {
    double dl;        // downloaded_size at the completing tick (:160-163)
    int32_t n_dl;     // ticks it took: download_time = G[n_dl] (:161)
    bool hit;         // false: max_ticks reached first
    // where the tick after the completing one lies, for lanej_begin_step_at: in the cursor's interval or (closed) in the
    // next one; next_known == false: in neither for sure (an interval shorter than a tick; no completing tick at all)
    bool closed, next_known;
};
// ... as an interval index
ABR_HD int32_t lanej_site_next(const Cursor &s, const Download &d) {
    return d.next_known ? s.j + (d.closed ? 1 : 0) : kSiteSearch;
}

template <class TB>
ABR_HD Download lanej_download(Cursor &s, const TB &t, const StepStart &st, int32_t k,
                               double target) {
    // One flat loop over chain SEGMENTS (abr_exact_jump.h); a lane moves on to its next
    // trace interval between two segments.  The next interval's bandwidth and end tick
    // are loaded one interval ahead so the loads overlap the arithmetic.  kk is the tick the
    // next addition belongs to: download_time is G[kk - k] (:161); interval ends are clamped to
    // max_ticks, so "ticks left in the interval" is also "ticks left at all".
    const int32_t mt = t.max_ticks;
    int32_t ke = st.ke < mt ? st.ke : mt, ke_next = st.ke_next, tn = st.tn;
    double c = st.c, bw_next = st.bw_next;
    ChainState cs;
    cs.x = 0.0; cs.eb = -1;                   // downloaded_size = 0 at a call site
    int32_t kk = k;
    bool hit = false;
    {
        // Prologue: downloaded_size starts at 0, so its first additions cross a binade every 1, 2, 4, 8, ... steps,
        // where a jump buys nothing (a 95-instruction trip for a handful of ticks).  The first up to 7 + 8 kPChunks additions are
        // therefore PLAIN additions -- that IS the reference's sequence -- and they have to work for every lane: a
        // wave pays its slowest lane, and with 64 lanes some call site always sits just before an interval end
        // (rounds 2-3 kept the prologue only when it fitted the current interval: 16 % of downloads got none).
        // The additions are n1 = ticks left in the current interval at c, then c2 = the next interval's constant.
        // To keep the code straight-line the first a = n1 mod 8 additions are single predicated ones, which
        // aligns the interval boundary with a chunk boundary; then kPChunks chunks of 8 with one constant each.
        // Checkpoints (bit q of kPCheck: after chunk q) are kept while they stay below the target (the sequence
        // increases, so nothing before a kept checkpoint reached it), within max_ticks, and inside the NEXT interval.
        const int32_t left = ke - kk;                                  // ticks of the current interval, >= 1
        const int32_t n1 = left > 0 ? left : 0;
        const int32_t a = n1 & 7, q1 = n1 >> 3;                        // singles, then q1 whole chunks at c
        const double c2 = bw_next * kTickDt;
        const int32_t room2 = (ke_next < mt ? ke_next : mt) - ke;      // ticks of the next interval (clamped to max_ticks)
        double x = 0.0, xb = 0.0;
        int32_t T = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 7; i++) x = (i < a) ? x + c : x;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int q = 0; q < kPChunks; q++) {
            const double cq = (q < q1) ? c : c2;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 8; i++) x = x + cq;
            if ((kPCheck >> q) & 1) {
                // a checkpoint after Tq ticks is usable if it is below the target and either all in the current
                // interval (Tq <= n1: then also within max_ticks, ke being clamped) or its part beyond n1 ends
                // strictly inside the next interval.  Usability only ever turns off as q grows.
                const int32_t Tq = a + 8 * (q + 1);
                const bool ok = (x < target) & ((Tq <= n1) | (Tq - n1 < room2));
                xb = ok ? x : xb;
                T = ok ? Tq : T;
            }
        }
        cs.x = xb;
        // past the interval boundary?  then the cursor moves on here (the loop reloads the look-ahead from it)
        const bool crossed = T > n1;
        kk += T;
        c = crossed ? c2 : c;
        ke = crossed ? (ke_next < mt ? ke_next : mt) : ke;
        s.j += crossed ? 1 : 0;
        s.tpos = crossed ? tn : s.tpos;
    }
    while (!hit && kk < mt) {
        // Interval over?  Its successor was prefetched.  Branch-free on purpose, and the
        // prefetch of the interval after that is (re)issued in EVERY trip: a load inside
        // a divergent `if` must be waited for at the end of that `if` (the loaded
        // registers merge with the not-taken path), exposing its full latency; issued
        // unconditionally it is only needed one trip later.
        const bool adv = kk >= ke;
        c = adv ? bw_next * kTickDt : c;
        ke = adv ? (ke_next < mt ? ke_next : mt) : ke;
        s.j += adv ? 1 : 0;
        s.tpos = adv ? tn : s.tpos;
        cs.eb = adv ? -1 : cs.eb;             // new constant: the steady state is void
        tn = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
        bw_next = s.trace[(uint32_t)tn];
        ke_next = t.interval_tick[(uint32_t)(s.j + 2)];
        kk += chain_segment<STOP_GE, 0, TB::kSettle, TB::kGuards>(cs, c, target, ke - kk, hit);                // :160-163
    }
    Download d;
    d.dl = cs.x; d.n_dl = kk - k; d.hit = hit;
    // Where the tick after the completing one lies: in the cursor's interval, or -- the completing tick was the last of its
    // interval -- in the next one, provided that one is not empty (an interval shorter than a tick: the search then).  The
    // proven tables' intervals span at least a tick each (chains_proven), so they do not wait for the look-ahead's last load.
    // ke is clamped to max_ticks: a download that ends there has no next call site.
    d.closed = kk >= ke;
    d.next_known = hit && (TB::kGuards == GUARDS_PROVEN || !d.closed || kk < ke_next);
    return d;
}

// The rest of the decision: the player side of the download's ticks, the completing tick,
// then phase B up to the next call site.  `action` only labels the step (last_action);
// avail_next = avail_tick[chunk_id + 1].
template <class TB>
ABR_HD StepResult lanej_after_download(LaneJ &s, const TB &t, const Download &d,
                                       int32_t avail_next, int32_t action, int32_t *how = nullptr) {
    if (how) *how = kWaitGated;               // (lanej_wait_call's, when it runs)
    StepResult r;
    r.bw = 0.0; r.hit = false; r.ended = false; r.timeout = false;
    const int32_t mt = t.max_ticks;
    const bool hit = d.hit;
    const int32_t n_dl = d.n_dl;
    const double g_ndl = t.G[n_dl];           // download_time; loaded now, divided by much later
    // ---- buffer side of the ticks before the completing one ----
    lanej_idle(s, t, hit ? n_dl - 1 : n_dl);
    ABR_STAMP(10);
    if (!hit) { r.timeout = true; return r; }
    // ---- the completing tick (:163-170, then :174-202) ----
    const bool playing = !(s.be || s.su);
    double b = s.buf + t.L;                                                  // :170
    if (playing) {                                                            // :176-184
        s.sumk += s.k; s.n_play++;
        if constexpr (TB::kSpeeds) {
            if (t.speed_rows >= 2) {
                if (s.pl_left == 0) sched_begin_chunk(s, t, s.k, b);
                b = b - s.sd;
                sched_played(s, t, 1);
            } else { b = b - s.sd; lanej_play(s, t, 1); }
        } else {
            b = b - t.sd;
        }
    }
    s.bf = b >= t.max_buffer;                                                // :190
    s.be = b <= 0.0;                                                         // :194
    if (s.be) b = 0.0;
    s.buf = b;
    s.su = s.su && !(b >= t.start_up_length);                                // :201-202
    s.k++;                                                                   // :205
    r.hit = true;
    r.bw = d.dl / g_ndl;                                                     // :164
    s.last_action = action;
    s.chunk_id++;                                                            // :166
    s.avail_k = avail_next;
    r.ended = s.chunk_id >= t.V;                                             // :207-208
    r.timeout = !r.ended && s.k >= mt;
    ABR_STAMP(11);
    if (!r.ended && !r.timeout) {
        s.n_su += s.su ? 1 : 0;                                              // T1 of the next tick
        s.n_rb += (!s.su && s.be) ? 1 : 0;
        r.timeout = !lanej_wait_call(s, t, how);                             // phase B
    }
    ABR_STAMP(12);
    return r;
}

// Where the NEXT download of a lane starts, from the player's state at THIS download's call site (buffer_level and the
// start_up / buffer_empty flags at tick k) and the download's length -- for the download side of the role-split kernels,
// which otherwise speculates "max(completing tick + 1, avail_next): not gated by buffer_full" (Simulator.py:143-145) and
// repeats the download when the player says otherwise.  A lane whose buffer sits near max_buffer is gated at almost every
// decision, and a workgroup is as slow as its slowest lane (round 5: ONE such lane made its workgroup, and with it the whole
// launch, 30 % longer).  Covers the steady playing state at one play speed for all lanes -- the only state in which
// buffer_level can reach max_buffer -- by running exactly what lanej_after_download and lanej_wait_call do to
// (buffer_level, buffer_full, k): the same chains on the same values, hence the same tick.  Returns false when the state is
// not covered (start-up, empty buffer, the buffer running dry, max_ticks in reach, per-lane speeds): the caller keeps its
// speculation, and the player's validation of the download's start tick stays the arbiter either way.
template <class TB>
ABR_HD bool lanej_gate_possible(double buf, bool su, bool be, int32_t n_dl, const TB &t) {
    // buffer_full at the completing tick needs buffer_level - (n_dl - 1) * sd + L - sd >= max_buffer; real arithmetic with a
    // margin far above the chains' rounding (<= 1e-9 over an episode), far below one tick's sd
    return !su && !be && !t.per_lane_speed && (buf + t.L) - (double)n_dl * t.sd >= t.max_buffer - 1.0e-6;
}
template <class TB>
ABR_HD bool lanej_predict_next_call(double buf, int32_t k, int32_t n_dl, int32_t avail_next, const TB &t,
                                    int32_t &k_next, double *buf_next = nullptr) {
    const int32_t mt = t.max_ticks;
    double b = buf;
    int32_t a = 0;
    // the ticks before the completing one (lanej_idle, playing branch)
    if (n_dl > 1 && lanej_drain(t, b, t.sd, n_dl - 1, a)) return false;
    // the completing tick (lanej_after_download): :170, :184, :190, :194
    b = b + t.L;
    b = b - t.sd;
    if (b <= 0.0) return false;
    bool bf = b >= t.max_buffer;
    k += n_dl;
    if (k >= mt) return false;
    // lanej_wait_call
    if (!(k >= avail_next && !bf)) {
        int32_t w = avail_next - k;
        if (w < 0) w = 0;
        if (w > mt - k) w = mt - k;
        if (w > 0) {
            if (lanej_drain(t, b, t.sd, w, a)) return false;
            bf = b >= t.max_buffer;
            k += w;
        }
        if (k >= mt) return false;
        if (bf) {
            a = 0;
            if (!chain<STOP_LT, 0, TB::kSettle, TB::kGuards>(b, -t.sd, t.max_buffer, mt - k, a)) return false;
            k += a;
            if (b <= 0.0) return false;
        }
    }
    k_next = k;
    if (buf_next) *buf_next = b;               // buffer_level at that call site (the lane is still playing: b > 0)
    return true;
}

// One decision in one thread, after lanej_begin_step: download a chunk of target_size, then
// run to the next call site.
template <class TB>
ABR_HD StepResult lanej_download_and_wait(LaneJ &s, const TB &t, const StepStart &st,
                                          double target, int32_t action) {
    const Download d = lanej_download(s.cur, t, st, s.k, target);
    return lanej_after_download(s, t, d, st.avail_next, action);
}
// The interval of the call site a step stopped at, for lanej_begin_step_at: how = lanej_wait_call's word, the cursor and the
// download as the step left them, avail_j_here = avail_j[s.chunk_id] of the chunk that call site downloads.
ABR_HD int32_t lanej_site_reached(int32_t how, const Cursor &cur, const Download &d, int32_t avail_j_here) {
    return how == kWaitNone ? lanej_site_next(cur, d) : (how == kWaitAvail ? avail_j_here : kSiteSearch);
}
// lanej_download_and_wait that also says which interval the call site it stops at lies in.  avail_j is loaded here, after
// the chains: one step ahead of its use, and in no register while they run.
template <class TB>
ABR_HD StepResult lanej_download_and_wait_site(LaneJ &s, const TB &t, const StepStart &st, double target, int32_t action,
                                               int32_t &j_site) {
    const Download d = lanej_download(s.cur, t, st, s.k, target);
    int32_t how;
    const StepResult r = lanej_after_download(s, t, d, st.avail_next, action, &how);
    j_site = lanej_site_reached(how, s.cur, d, t.avail_j[s.chunk_id]);
    return r;
}

// begin + download + wait in one call (host harness)
template <class TB>
ABR_HD StepResult lanej_step(LaneJ &s, const TB &t, double target, int32_t action) {
    const StepStart st = lanej_begin_step(s.cur, t, s.k, s.chunk_id);
    return lanej_download_and_wait(s, t, st, target, action);
}

// ---- the standard bitrate rules, evaluated at a call site (include/abr_env.h: abr_rule_config) ----
// Inputs are the arguments of get_next_bitrate (Simulator.py:155): c = chunk_id, B = buffer_level, h[0..c) =
// previous_bandwidths oldest first, and br(m) = chunk c's bitrate m (per-chunk table or the ladder).  Everything is
// float64 in a fixed operation order (the library builds with -ffp-contract=off), so a numpy twin written in the same
// order reproduces every answer bit for bit.  `br` and `hist` are accessors, so that the kernels read the ladder and the
// history rows straight from where they live (no copy into a local array, which would cost scratch).
// kRuleFastMpc is internal: the FastMPC lookup (include/abr_env.h: abr_fastmpc), reached through abr_env_step_fastmpc only
enum { kRuleBuffer = 1, kRuleRate = 2, kRuleBola = 3, kRuleFastMpc = 4 };

struct RuleParams {
    int32_t kind, window;                    // kRule*; RATE, FastMPC: W >= 1
    double reservoir, cushion;               // BUFFER: r >= 0, k > 0 [s]
    double safety;                           // RATE: s > 0
    double bola_v, bola_gp;                  // BOLA: V > 0, gp
    const double *utility;                   // BOLA: [video_length][n_rates]
    // FastMPC (appended, so that every field above keeps its offset): the blob -- uint8 entries [fm_rows][M][fm_nb][fm_nq],
    // padded to 8 bytes, then the fm_nb - 1 buffer edges and the fm_nq - 1 throughput edges, float64
    const uint8_t *fm_table;
    int32_t fm_uniform;                      // 0: row = c; 1: row = min(V - c, fm_horizon) - 1
    int32_t fm_horizon, fm_nb, fm_nq;
};

// the highest index m in 1..M-1 with br(m) <= X, else 0 (on an ascending ladder: the highest rate not above X)
template <class BR>
ABR_HD int32_t rule_hi(const BR &br, int32_t M, double X) {
    int32_t a = 0;
    for (int32_t m = 1; m < M; m++) a = br(m) <= X ? m : a;
    return a;
}

// BBA-0 rate map (Huang et al. 2014) without hysteresis
template <class BR>
ABR_HD int32_t rule_buffer(const RuleParams &r, const BR &br, int32_t M, double B) {
    if (B <= r.reservoir) return 0;
    if (B >= r.reservoir + r.cushion) return M - 1;
    const double lo = br(0);
    return rule_hi(br, M, lo + ((B - r.reservoir) / r.cushion) * (br(M - 1) - lo));
}

// harmonic mean of the n > 0 throughputs h[c-n .. c-1]: S = sum of 1.0 / h[j] oldest first, then n / S (RATE, RobustMPC)
template <class HIST>
ABR_HD double harmonic_tail(const HIST &hist, int32_t c, int32_t n) {
    double S = 0.0;
    for (int32_t j = c - n; j < c; j++) S = S + 1.0 / hist(j);
    return (double)n / S;
}

// safety * harmonic mean of the last min(W, c) throughputs, summed oldest first
template <class BR, class HIST>
ABR_HD int32_t rule_rate(const RuleParams &r, const BR &br, const HIST &hist, int32_t M, int32_t c) {
    const int32_t n = r.window < c ? r.window : c;
    if (n <= 0) return 0;
    return rule_hi(br, M, r.safety * harmonic_tail(hist, c, n));
}

// BOLA-BASIC (Spiteri et al. 2016): argmax_m (V (u[c][m] + gp) - B) / br(m), the FIRST index of the maximum
template <class BR>
ABR_HD int32_t rule_bola(const RuleParams &r, const BR &br, int32_t M, int32_t c, double B) {
    const double *u = r.utility + (int64_t)c * M;
    double best = (r.bola_v * (u[0] + r.bola_gp) - B) / br(0);
    int32_t a = 0;
    for (int32_t m = 1; m < M; m++) {
        const double sc = (r.bola_v * (u[m] + r.bola_gp) - B) / br(m);
        a = sc > best ? m : a;
        best = sc > best ? sc : best;
    }
    return a;
}

template <class BR, class HIST>
ABR_HD int32_t rule_select(const RuleParams &r, const BR &br, const HIST &hist, int32_t M, int32_t c, double B) {
    if (r.kind == kRuleBuffer) return rule_buffer(r, br, M, B);
    if (r.kind == kRuleRate) return rule_rate(r, br, hist, M, c);
    return rule_bola(r, br, M, c, B);
}

// ---- FastMPC's lookup (include/abr_env.h: abr_fastmpc) ----
// the number of the n ascending edges e[0..n) that are <= x, by bisection (NaN: 0; +inf: n)
ABR_HD int32_t fastmpc_cell(const double *e, int32_t n, double x) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// bytes of the blob's entries before the edges: n_rows * M * Nb * Nq, rounded up to 8
ABR_HD int64_t fastmpc_entry_bytes(int32_t n_rows, int32_t M, int32_t nb, int32_t nq) {
    return (((int64_t)n_rows * M * nb * nq) + 7) & ~(int64_t)7;
}

// The decision at a call site: chunk c, previous bitrate pv (Python's -M..-1 wrap), buffer B, history h[0..c).  -1 for a
// chunk outside [0, V) or a previous bitrate outside [-M, M), which no environment lane presents.
template <class HIST>
ABR_HD int32_t fastmpc_lookup(const RuleParams &r, const HIST &hist, int32_t M, int32_t V, int32_t c, int32_t pv,
                              double B) {
    if (c < 0 || c >= V || pv < -M || pv >= M) return -1;
    const int32_t n = r.window < c ? r.window : c;
    if (n <= 0) return 0;
    const double P = harmonic_tail(hist, c, n);
    if (pv < 0) pv += M;
    const int32_t row = r.fm_uniform ? ((V - c < r.fm_horizon ? V - c : r.fm_horizon) - 1) : c;
    const int32_t rows = r.fm_uniform ? r.fm_horizon : V;
    const double *be = (const double *)(r.fm_table + fastmpc_entry_bytes(rows, M, r.fm_nb, r.fm_nq));
    const double *te = be + (r.fm_nb - 1);
    const int32_t bi = fastmpc_cell(be, r.fm_nb - 1, B);
    const int32_t qi = fastmpc_cell(te, r.fm_nq - 1, P);
    return r.fm_table[(((int64_t)row * M + pv) * r.fm_nb + bi) * r.fm_nq + qi];
}

// Under the environment's size table (include/abr_env.h: abr_env_set_size_table) RATE and BOLA compare and divide by what
// a rung costs to fetch: their br(m) is the effective bitrate e[m] = sz[c][m] / chunk_length, one float64 division.  BBA-0's
// map lives on the nominal ladder, and FastMPC reads no br at all.
ABR_HD bool rule_reads_cost(int32_t kind) { return kind == kRuleRate || kind == kRuleBola; }
ABR_HD double rule_cost(const double *sz_row, double L, int32_t m) { return sz_row[m] / L; }

// rule_select with the call-site arguments only FastMPC reads (V, the previous bitrate)
template <class BR, class HIST>
ABR_HD int32_t rule_select_at(const RuleParams &r, const BR &br, const HIST &hist, int32_t M, int32_t V, int32_t c,
                              int32_t pv, double B) {
    if (r.kind == kRuleFastMpc) return fastmpc_lookup(r, hist, M, V, c, pv, B);
    return rule_select(r, br, hist, M, c, B);
}

// ---- RobustMPC's throughput estimate (Yin et al. 2015; include/abr_env.h: abr_mpc_robust) ----
// One lane at a decision: c = chunk_number (also the history length), h[0..c) = previous_bandwidths oldest first, window
// W in 1..16.  The lane's state (include/abr_env.h: ABR_ROBUST_* layout): cs1 = c* + 1 of the last estimate p* (0 = none),
// cnt = number of stored relative errors, err(0 .. cnt) = those errors oldest first (entries at or past cnt hold no
// meaning; a count outside 0..W is read as 0).  `err` is an accessor returning a double& so that the kernel updates the state rows in place.  Returns the
// estimate P the search divides by, or 0.0 for "no decision"; every operation is float64 in the order written.
template <class HIST, class ERR>
ABR_HD double robust_estimate(int32_t W, int32_t c, const HIST &hist, int32_t &cs1, int32_t &cnt, double &ps,
                              const ERR &err) {
    if (cnt < 0 || cnt > W) cnt = 0;
    // 1. the error of the previous estimate against the throughput it predicted
    if (cs1 > 0 && (int64_t)cs1 == (int64_t)c) {
        const double hc = hist(c - 1);
        const double e = fabs(ps - hc) / hc;
        if (cnt < W) {
            err(cnt) = e;
            cnt = cnt + 1;
        } else {
            for (int32_t k = 1; k < W; k++) err(k - 1) = err(k);
            err(W - 1) = e;
        }
    } else if (!(cs1 > 0 && (int64_t)cs1 == (int64_t)c + 1)) {
        cnt = 0;                                   // none, a gap, a new episode or a rewind
    }
    // 2. the window
    const int32_t n = W < c ? W : c;
    if (n <= 0) {
        cs1 = 0; cnt = 0; ps = 0.0;
        return 0.0;
    }
    // 3. harmonic mean of the last n throughputs (RATE's arithmetic)
    const double hm = harmonic_tail(hist, c, n);
    // 4. discount by the largest recent relative error
    double E = 0.0;
    if (cnt > 0) {
        E = err(0);
        for (int32_t k = 1; k < cnt; k++) E = err(k) > E ? err(k) : E;
    }
    const double P = hm / (1.0 + E);
    // 5. / 6.  (hm <= DBL_MAX: finite; NaN fails both comparisons)
    if (!(hm > 0.0 && hm <= 1.79769313486231570815e+308)) {
        cs1 = 0; cnt = 0; ps = 0.0;
        return 0.0;
    }
    ps = hm;
    cs1 = c + 1;
    return P > 0.0 ? P : 0.0;
}

// robust_estimate on lane `lane` of an N-lane state in the ABR_ROBUST_* layout (int32 [2][N], then float64 [1 + W][N]),
// updated in place: what the predictor kernels run per thread
template <class HIST>
ABR_HD double robust_estimate_rows(int32_t W, int32_t c, const HIST &hist, uint8_t *state, int64_t N, int64_t lane) {
    int32_t *cs1_row = (int32_t *)state, *cnt_row = cs1_row + N;
    double *ps_row = (double *)(state + 2 * sizeof(int32_t) * N), *err_rows = ps_row + N;
    int32_t cs1 = cs1_row[lane], cnt = cnt_row[lane];
    double ps = ps_row[lane];
    const auto ef = [&](int32_t k) -> double & { return err_rows[(int64_t)k * N + lane]; };
    const double P = robust_estimate(W, c, hist, cs1, cnt, ps, ef);
    cs1_row[lane] = cs1; cnt_row[lane] = cnt; ps_row[lane] = ps;
    return P;
}


// ---------------------------------------------------------------------------
// Learned policy (include/abr_env.h: abr_policy): features, the MLP forward pass as k-ordered fmaf chains, the decision.
// The widths are runtime values, so every register array is indexed by an unrolled loop with a uniform early exit: no
// array is ever indexed by a runtime value (0 B of scratch on the device).
// ---------------------------------------------------------------------------
constexpr int kPolicyMaxWindow = 16, kPolicyMaxWidth = 64, kPolicyMaxRates = 16;
constexpr int kPolicyMaxF = 4 + kPolicyMaxWindow + kPolicyMaxRates;

struct PolicyNet {
    int32_t window, n_hidden, w0, w1, M, F;   // F = 4 + window + M; w0 / w1 the hidden widths (0 when absent)
    const double *norm;                       // [2][F] shift, scale; nullptr: 0 and 1
    uint64_t seed, thr;                       // philox key, explore threshold (0 .. 2^32)
};

// philox4x32-10, all four output words; the same rounds as abr_env.hip: philox_action, whose action is
// ((uint64)word0 * n_rates) >> 32
ABR_HD void philox4(uint64_t seed, uint64_t lane, uint32_t step, uint32_t episode, uint32_t out[4]) {
    uint32_t c0 = (uint32_t)lane, c1 = (uint32_t)(lane >> 32), c2 = step, c3 = episode;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The features of one lane at a call site: chunk c (0 <= c < V), buffer B, previous bitrate a, latency G - P,
// h(j) = previous_bandwidths[j], br(r, m) = chunk r's bitrate m.  x[i] = (float)((raw_i - shift_i) * scale_i).
// nx(r, m) = what features 4 + W + m hold of chunk r: its bitrates, or -- while the environment has a size table
// (include/abr_env.h: abr_env_set_size_table) -- its sizes, Pensieve's next_chunk_sizes.
template <class Hist, class Br, class Nx>
ABR_HD void policy_features(const PolicyNet &n, const Hist &h, const Br &br, const Nx &nx, int32_t V, int32_t c, int32_t a,
                            double B, double G, double P, float x[kPolicyMaxF]) {
    const int32_t W = n.window;
#pragma unroll
    for (int i = 0; i < kPolicyMaxF; i++) {
        if (i < n.F) {
            double raw;
            if (i == 0) raw = B;
            else if (i == 1) raw = (a >= 0 && a < n.M && c >= 1) ? br(c - 1, a) : 0.0;
            else if (i == 2) raw = (double)(V - c);
            else if (i == 3) raw = G - P;
            else if (i < 4 + W) { const int32_t j = c - W + (i - 4); raw = j >= 0 ? h(j) : 0.0; }
            else raw = nx(c, i - 4 - W);
            const double sh = n.norm ? n.norm[i] : 0.0, sc = n.norm ? n.norm[n.F + i] : 1.0;
            x[i] = (float)((raw - sh) * sc);
        } else {
            x[i] = 0.0f;
        }
    }
}

// without a size table: features 4 + W + m are chunk c's bitrates
template <class Hist, class Br>
ABR_HD void policy_features(const PolicyNet &n, const Hist &h, const Br &br, int32_t V, int32_t c, int32_t a, double B,
                            double G, double P, float x[kPolicyMaxF]) {
    policy_features(n, h, br, br, V, c, a, B, G, P, x);
}

ABR_HD float relu_f32(float v) { return v > 0.0f ? v : 0.0f; }   // NaN and -0 -> +0

// The padded layout the forward pass reads (the kernel stages it in LDS).  Every row has a fixed length -- 36 for the
// features, 64 for a hidden layer, 16 for the outputs -- so that the inner loops are fully unrolled and branch-free (one
// wave can issue all the loads of a row before it waits).  A padded weight is -0.0f and a padded input +0.0f:
// fmaf(-0, +0, acc) == acc for every acc (NaN, infinities and both zeros included), so padding leaves each chain's bits
// as the contract's.  The layer-1 and single-hidden-layer output weights are stored transposed ([k][j]), the order in which
// hidden unit k adds its term into every accumulator j.
constexpr int kPolicyRowF = kPolicyMaxF, kPolicyRowH = kPolicyMaxWidth, kPolicyRowM = kPolicyMaxRates;
// VALUE (include/abr_env.h: abr_policy_value): one more row after everything else, the value head's weights padded to the
// width of its input (kPolicyRowH after a hidden layer, kPolicyRowF without one) and then its bias.  The offsets of the
// policy's own rows do not move.
struct PolicyLayout { int32_t W0, b0, W1, b1, Wo, bo, total, Wv, bv; };

ABR_HD int32_t policy_align4(int32_t x) { return (x + 3) & ~3; }

template <bool VALUE = false>
ABR_HD PolicyLayout policy_layout(const PolicyNet &n) {
    PolicyLayout L{};
    int32_t o = 0;
    if (n.n_hidden >= 1) { L.W0 = o; o += n.w0 * kPolicyRowF; L.b0 = o; o = policy_align4(o + n.w0); }
    if (n.n_hidden == 2) { L.W1 = o; o += n.w0 * kPolicyRowH; L.b1 = o; o += kPolicyRowH; }
    if (n.n_hidden == 1) {
        L.Wo = o; o += n.w0 * kPolicyRowM; L.bo = o; o += kPolicyRowM;
    } else {
        L.Wo = o; o += n.M * (n.n_hidden == 0 ? kPolicyRowF : kPolicyRowH); L.bo = o; o = policy_align4(o + n.M);
    }
    if (VALUE) { L.Wv = o; o += n.n_hidden == 0 ? kPolicyRowF : kPolicyRowH; L.bv = o; o += 4; }
    L.total = o;
    return L;
}

// Slot d of the padded layout, read from the packed blob (per layer Wt[out][in] row-major, then b[out]); VALUE: the last
// row from `head` (Wv[0..in) then bv, in = the width of the last hidden layer, or F without one)
template <bool VALUE = false>
ABR_HD float policy_padded(const PolicyNet &n, const PolicyLayout &L, const float *__restrict__ blob, int32_t d,
                           const float *__restrict__ head = nullptr) {
    const float pw = -0.0f, pb = 0.0f;
    const int32_t F = n.F, H0 = n.w0, H1 = n.w1, M = n.M;
    if (VALUE) {
        if (d >= L.Wv) {
            const int32_t in = n.n_hidden == 0 ? F : n.n_hidden == 1 ? H0 : H1, k = d - L.Wv;
            if (d < L.bv) return k < in ? head[k] : pw;
            return d == L.bv ? head[in] : pb;
        }
    }
    int32_t o = 0;                                            // packed offset of the current layer
    if (n.n_hidden >= 1) {
        if (d >= L.W0 && d < L.b0) { const int32_t k = (d - L.W0) / kPolicyRowF, i = (d - L.W0) % kPolicyRowF;
                                     return i < F ? blob[o + k * F + i] : pw; }
        if (d >= L.b0 && d < L.b0 + H0) return blob[o + H0 * F + (d - L.b0)];
        o += H0 * F + H0;
    }
    if (n.n_hidden == 2) {
        if (d >= L.W1 && d < L.b1) { const int32_t k = (d - L.W1) / kPolicyRowH, j = (d - L.W1) % kPolicyRowH;
                                     return j < H1 ? blob[o + j * H0 + k] : pw; }
        if (d >= L.b1 && d < L.b1 + kPolicyRowH) { const int32_t j = d - L.b1; return j < H1 ? blob[o + H1 * H0 + j] : pb; }
        o += H1 * H0 + H1;
    }
    if (n.n_hidden == 1) {
        if (d >= L.Wo && d < L.bo) { const int32_t k = (d - L.Wo) / kPolicyRowM, j = (d - L.Wo) % kPolicyRowM;
                                     return j < M ? blob[o + j * H0 + k] : pw; }
        if (d >= L.bo && d < L.bo + kPolicyRowM) { const int32_t j = d - L.bo; return j < M ? blob[o + M * H0 + j] : pb; }
    } else {
        const int32_t row = n.n_hidden == 0 ? kPolicyRowF : kPolicyRowH, in = n.n_hidden == 0 ? F : H1;
        if (d >= L.Wo && d < L.bo) { const int32_t j = (d - L.Wo) / row, k = (d - L.Wo) % row;
                                     return k < in ? blob[o + j * in + k] : pw; }
        if (d >= L.bo && d < L.bo + M) return blob[o + M * in + (d - L.bo)];
    }
    return pb;
}

// acc = b, then fmaf(row[k], in[k], acc) for k = 0 .. CAP-1: the contract's chain over the real inputs, the padded
// terms being exact no-ops
template <int CAP>
ABR_HD float dot_row(const float *__restrict__ row, float b, const float *in) {
    float acc = b;
#pragma unroll
    for (int k = 0; k < CAP; k++) acc = fmaf(row[k], in[k], acc);
    return acc;
}

// The forward pass and the first argmax over the padded layout `w` (policy_layout / policy_padded); x[i] = +0 for
// i >= F.  emit(j, score_j) is called once per output j in order.  Returns g.
// VALUE: *value = bv, then fmaf(Wv[k], y[k], v) over the last hidden layer's post-ReLU outputs y (x without a hidden layer)
// in k order -- one more chain of the same kind, which reads what the scores read and feeds nothing back into them.
template <bool VALUE = false, class Emit>
ABR_HD int32_t policy_forward(const PolicyNet &n, const float *__restrict__ w, const float x[kPolicyMaxF], const Emit &emit,
                              float *value = nullptr) {
    const PolicyLayout L = policy_layout<VALUE>(n);
    const int32_t M = n.M;
    int32_t g = 0;
    float best = 0.0f;
    const auto take = [&](int32_t j, float s) {
        emit(j, s);
        if (j == 0) best = s;
        else if (s > best) { best = s; g = j; }
    };
    if (n.n_hidden == 0) {
        for (int32_t j = 0; j < M; j++) take(j, dot_row<kPolicyRowF>(w + L.Wo + j * kPolicyRowF, w[L.bo + j], x));
        if (VALUE) *value = dot_row<kPolicyRowF>(w + L.Wv, w[L.bv], x);
    } else if (n.n_hidden == 1) {
        // hidden unit k, then its term in every output accumulator: each output stays a k-ordered chain
        float acc[kPolicyRowM];
#pragma unroll
        for (int j = 0; j < kPolicyRowM; j++) acc[j] = w[L.bo + j];
        float accv = VALUE ? w[L.bv] : 0.0f;
        for (int32_t k = 0; k < n.w0; k++) {
            const float hk = relu_f32(dot_row<kPolicyRowF>(w + L.W0 + k * kPolicyRowF, w[L.b0 + k], x));
            const float *wk = w + L.Wo + k * kPolicyRowM;
#pragma unroll
            for (int j = 0; j < kPolicyRowM; j++) acc[j] = fmaf(wk[j], hk, acc[j]);
            if (VALUE) accv = fmaf(w[L.Wv + k], hk, accv);
        }
#pragma unroll
        for (int j = 0; j < kPolicyRowM; j++)
            if (j < M) take(j, acc[j]);
        if (VALUE) *value = accv;
    } else {
        // layer-0 unit k, then its term in every layer-1 accumulator; then the output layer unit by unit
        float acc[kPolicyRowH];
#pragma unroll
        for (int j = 0; j < kPolicyRowH; j++) acc[j] = w[L.b1 + j];
        for (int32_t k = 0; k < n.w0; k++) {
            const float hk = relu_f32(dot_row<kPolicyRowF>(w + L.W0 + k * kPolicyRowF, w[L.b0 + k], x));
            const float *wk = w + L.W1 + k * kPolicyRowH;
#pragma unroll
            for (int j = 0; j < kPolicyRowH; j++) acc[j] = fmaf(wk[j], hk, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kPolicyRowH; j++) acc[j] = relu_f32(acc[j]);
        for (int32_t j = 0; j < M; j++) take(j, dot_row<kPolicyRowH>(w + L.Wo + j * kPolicyRowH, w[L.bo + j], acc));
        if (VALUE) *value = dot_row<kPolicyRowH>(w + L.Wv, w[L.bv], acc);
    }
    return g;
}

// The decision: the random policy's action from the same philox block when word 1 < thr, else g.
ABR_HD int32_t policy_explore(const PolicyNet &n, uint64_t lane, int32_t c, int32_t episode, int32_t g) {
    if (n.thr == 0) return g;
    uint32_t r[4];
    philox4(n.seed, lane, (uint32_t)c, (uint32_t)episode, r);
    return (uint64_t)r[1] < n.thr ? (int32_t)(((uint64_t)r[0] * (uint32_t)n.M) >> 32) : g;
}

// The sampled decision (include/abr_env.h: abr_policy_sampling).  exp_c is the contract's float32 exp for x <= 0: a
// Cody-Waite reduction by ln 2 (Cephes' split), a degree-6 fmaf Horner chain, an exact scaling by 2^k (k >= -116 keeps
// the result normal).  No device expf: its bits are not numpy's.
constexpr float kExpLog2e = 0x1.715476p+0f, kExpLn2Hi = 0x1.63p-1f, kExpLn2Lo = -0x1.bd0106p-13f;
constexpr float kExpC3 = 0x1.55549cp-3f, kExpC4 = 0x1.555694p-5f, kExpC5 = 0x1.1234fcp-7f, kExpC6 = 0x1.6b69e0p-10f;

ABR_HD float exp_c(float x) {
    if (!(x >= -80.0f)) return 0.0f;                          // -inf and NaN too
    const float k = rintf(x * kExpLog2e);
    float r = fmaf(-k, kExpLn2Hi, x);
    r = fmaf(-k, kExpLn2Lo, r);
    float p = kExpC6;
    p = fmaf(p, r, kExpC5);
    p = fmaf(p, r, kExpC4);
    p = fmaf(p, r, kExpC3);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return ldexpf(p, (int)k);
}

// The draw from softmax(s * iT) given the first argmax g and philox word 2 w2.  buf(m) is a float& that holds s_m on
// entry and e_m on return; prob(m, v) receives probs[m] in order.  Two passes over m: e_m and S, then cum_m, the first
// cum_m > t and e_m / S.  A non-finite s_g answers g with a one-hot distribution.
template <class Buf, class Prob>
ABR_HD int32_t policy_softmax_sample(int32_t M, int32_t g, float iT, uint32_t w2, const Buf &buf, const Prob &prob) {
    const float sg = buf(g);
    if (!(sg >= -0x1.fffffep127f && sg <= 0x1.fffffep127f)) {
        for (int32_t m = 0; m < M; m++) prob(m, m == g ? 1.0f : 0.0f);
        return g;
    }
    float S = 0.0f;
    for (int32_t m = 0; m < M; m++) {
        const float d = buf(m) - sg;
        const float e = exp_c(d * iT);
        buf(m) = e;
        S += e;
    }
    const float t = (float)(w2 >> 8) * 0x1p-24f * S;
    float cum = 0.0f;
    int32_t pick = -1;
    for (int32_t m = 0; m < M; m++) {
        const float e = buf(m);
        cum += e;
        if (pick < 0 && cum > t) pick = m;
        prob(m, e / S);
    }
    return pick < 0 ? g : pick;
}

// The decision of a sampling mode: argmax (0) is policy_explore with probs one-hot at g; softmax (1) draws with word 2 of
// the exploration's philox block, and word 1 < thr still takes the random policy's action from word 0.
template <class Buf, class Prob>
ABR_HD int32_t policy_decide(const PolicyNet &n, uint64_t lane, int32_t c, int32_t episode, int32_t g, int32_t mode,
                             float iT, const Buf &buf, const Prob &prob) {
    if (mode == 0) {
        for (int32_t m = 0; m < n.M; m++) prob(m, m == g ? 1.0f : 0.0f);
        return policy_explore(n, lane, c, episode, g);
    }
    uint32_t r[4];
    philox4(n.seed, lane, (uint32_t)c, (uint32_t)episode, r);
    const int32_t s = policy_softmax_sample(n.M, g, iT, r[2], buf, prob);
    return (uint64_t)r[1] < n.thr ? (int32_t)(((uint64_t)r[0] * (uint32_t)n.M) >> 32) : s;
}

// ---------------------------------------------------------------------------
// The recurrent policy (include/abr_env.h: abr_policy_gru; abr_env.hip: policy_gru_kernel): one GRU cell of H units over
// the features and the lane's hidden state, then Linear(H, M) over the new state.  The net is a PolicyNet with n_hidden = 1
// and w0 = H (window, M, F, norm, seed and thr mean what they mean above).
// ---------------------------------------------------------------------------
// The gate activations on exp_c (whose argument is never positive here).  Both are exact in the order written: one
// rounding per operation, a correctly rounded division.
ABR_HD float sig_c(float v) {
    if (v != v) return v;
    const float e = exp_c(-fabsf(v));
    const float q = 1.0f + e;
    return (v >= 0.0f ? 1.0f : e) / q;
}

ABR_HD float tanh_c(float v) {
    if (v != v) return v;
    const float e = exp_c(-2.0f * fabsf(v));
    const float t = (1.0f - e) / (1.0f + e);
    return copysignf(t, v);
}

// The padded layout the forward pass reads (the kernel stages it in LDS), by the conventions of policy_layout: rows of fixed
// length, padded weights -0.0f against padded inputs +0.0f.
//   G   H x 3 gate rows (unit j's r, z, n rows are adjacent), each kPolicyRowF input weights then kPolicyRowH recurrent ones
//   B   H x 8: b_ih[r, z, n][j], b_hh[r, z, n][j], two pads -- the six chains' first terms in one 32-byte read
//   Wo  H x kPolicyRowM, transposed ([k][m]): the order in which unit k adds its term into every output accumulator
//   bo  kPolicyRowM
//   VALUE: Wv kPolicyRowH, then bv (4 floats)
constexpr int kGruRow = kPolicyRowF + kPolicyRowH, kGruBias = 8;
struct PolicyGruLayout { int32_t G, B, Wo, bo, total, Wv, bv; };

template <bool VALUE = false>
ABR_HD PolicyGruLayout policy_gru_layout(const PolicyNet &n) {
    PolicyGruLayout L{};
    const int32_t H = n.w0;
    int32_t o = 0;
    L.G = o; o += H * 3 * kGruRow;
    L.B = o; o += H * kGruBias;
    L.Wo = o; o += H * kPolicyRowM;
    L.bo = o; o += kPolicyRowM;
    if (VALUE) { L.Wv = o; o += kPolicyRowH; L.bv = o; o += 4; }
    L.total = o;
    return L;
}

// Slot d of the padded layout, read from the packed blob in torch.nn.GRUCell's layout (W_ih [3H][F], W_hh [3H][H], b_ih [3H],
// b_hh [3H], gates r, z, n; then W_out [M][H], b_out [M]); VALUE: the last row from `head` (Wv[0..H) then bv)
template <bool VALUE = false>
ABR_HD float policy_gru_padded(const PolicyNet &n, const PolicyGruLayout &L, const float *__restrict__ blob, int32_t d,
                               const float *__restrict__ head = nullptr) {
    const float pw = -0.0f, pb = 0.0f;
    const int32_t F = n.F, H = n.w0, M = n.M;
    const int32_t Wih = 0, Whh = Wih + 3 * H * F, bih = Whh + 3 * H * H, bhh = bih + 3 * H, Wout = bhh + 3 * H,
                  bout = Wout + M * H;
    if (VALUE) {
        if (d >= L.Wv) {
            const int32_t k = d - L.Wv;
            if (d < L.bv) return k < H ? head[k] : pw;
            return d == L.bv ? head[H] : pb;
        }
    }
    if (d < L.B) {
        const int32_t row = (d - L.G) / kGruRow, i = (d - L.G) % kGruRow, j = row / 3, g = row % 3;
        if (i < kPolicyRowF) return i < F ? blob[Wih + (g * H + j) * F + i] : pw;
        const int32_t k = i - kPolicyRowF;
        return k < H ? blob[Whh + (g * H + j) * H + k] : pw;
    }
    if (d < L.Wo) {
        const int32_t j = (d - L.B) / kGruBias, s = (d - L.B) % kGruBias;
        return s < 3 ? blob[bih + s * H + j] : s < 6 ? blob[bhh + (s - 3) * H + j] : pb;
    }
    if (d < L.bo) {
        const int32_t k = (d - L.Wo) / kPolicyRowM, m = (d - L.Wo) % kPolicyRowM;
        return m < M ? blob[Wout + m * H + k] : pw;
    }
    if (d < L.bo + kPolicyRowM) { const int32_t m = d - L.bo; return m < M ? blob[bout + m] : pb; }
    return pb;
}

// Four adjacent weights of a padded row (rows start on 16-byte boundaries: one 128-bit LDS read on the device).
struct alignas(16) PolicyGruQuad { float v[4]; };
ABR_HD PolicyGruQuad policy_gru_quad(const float *__restrict__ p) {
    PolicyGruQuad q;
    __builtin_memcpy(&q, __builtin_assume_aligned(p, 16), sizeof q);
    return q;
}
// Pins the six accumulators in the device's instruction stream: the fmafs written before it are issued before it and the
// ones written after it after it (an empty statement the compiler may not move values across, then a scheduling fence).
// No effect on any value; nothing on the host.
ABR_HD void policy_gru_pin(float (&gi)[3], float (&gh)[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(gi[0]), "+v"(gi[1]), "+v"(gi[2]), "+v"(gh[0]), "+v"(gh[1]), "+v"(gh[2]));
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// The cell, the output layer and the first argmax over the padded layout `w` (16-byte aligned).  x[i] = +0 for i >= F and
// h[k] = +0 for k >= H; hin(j) is h[j] again for a runtime j (the register array is only ever indexed by an unrolled loop,
// so the caller answers it from where h came from).
// A unit is 300 weight reads and 300 fmafs, and no read depends on anything: left alone, the device compiler issues the reads
// far ahead of the fmafs and needs a register for each (346 registers, or scratch under a tighter budget).  So the unit is
// written as a software pipeline over its 25 groups of four k: the three gate rows' quads of group q + kGruAhead are read,
// a pin (policy_gru_pin), then group q's twelve fmafs -- the six chains (gi and gh of r, z, n) advance side by side, and the reads in
// flight are bounded at (kGruAhead + 1) x 12 weights.
// h'[j] is handed to store(j, v) the moment it exists and folded at once into every output accumulator (and the value's),
// each of which therefore stays a k-ordered chain; no second array of H registers is held.  emit(m, score_m) once per
// output m in order.  Returns g.
constexpr int kGruGroups = kGruRow / 4, kGruGroupsX = kPolicyRowF / 4, kGruAhead = 4;
static_assert(kGruRow % 4 == 0 && kPolicyRowF % 4 == 0 && kPolicyRowM == 16, "quads");

template <bool VALUE = false, class Hin, class Store, class Emit>
ABR_HD int32_t policy_gru_forward(const PolicyNet &n, const float *__restrict__ w, const float x[kPolicyMaxF],
                                  const float h[kPolicyRowH], const Hin &hin, const Store &store, const Emit &emit,
                                  float *value = nullptr) {
    const PolicyGruLayout L = policy_gru_layout<VALUE>(n);
    const int32_t M = n.M, H = n.w0;
    float acc[kPolicyRowM];
#pragma unroll
    for (int m = 0; m < kPolicyRowM; m++) acc[m] = w[L.bo + m];
    float accv = VALUE ? w[L.bv] : 0.0f;
    for (int32_t j = 0; j < H; j++) {
        const float *__restrict__ row = w + L.G + j * (3 * kGruRow);
        const float *__restrict__ wk = w + L.Wo + j * kPolicyRowM;
        PolicyGruQuad q[kGruGroups][3], o[4];
        const PolicyGruQuad b0 = policy_gru_quad(w + L.B + j * kGruBias), b1 = policy_gru_quad(w + L.B + j * kGruBias + 4);
#pragma unroll
        for (int t = 0; t < kGruAhead; t++) {
#pragma unroll
            for (int g = 0; g < 3; g++) q[t][g] = policy_gru_quad(row + g * kGruRow + 4 * t);
        }
        const float hj = hin(j);
        float gi[3] = {b0.v[0], b0.v[1], b0.v[2]}, gh[3] = {b0.v[3], b1.v[0], b1.v[1]};
#pragma unroll
        for (int t = 0; t < kGruGroups; t++) {
            if (t + kGruAhead < kGruGroups) {
#pragma unroll
                for (int g = 0; g < 3; g++) q[t + kGruAhead][g] = policy_gru_quad(row + g * kGruRow + 4 * (t + kGruAhead));
            } else if (t + kGruAhead < kGruGroups + 4) {
                o[t + kGruAhead - kGruGroups] = policy_gru_quad(wk + 4 * (t + kGruAhead - kGruGroups));
            }
            policy_gru_pin(gi, gh);
#pragma unroll
            for (int e = 0; e < 4; e++) {
#pragma unroll
                for (int g = 0; g < 3; g++) {
                    if (t < kGruGroupsX) gi[g] = fmaf(q[t][g].v[e], x[4 * t + e], gi[g]);
                    else gh[g] = fmaf(q[t][g].v[e], h[4 * (t - kGruGroupsX) + e], gh[g]);
                }
            }
        }
        policy_gru_pin(gi, gh);
        const float r = sig_c(gi[0] + gh[0]);
        const float z = sig_c(gi[1] + gh[1]);
        const float c = tanh_c(fmaf(r, gh[2], gi[2]));
        const float d = hj - c;
        const float hp = fmaf(z, d, c);
        store(j, hp);
#pragma unroll
        for (int m = 0; m < kPolicyRowM; m++) acc[m] = fmaf(o[m / 4].v[m % 4], hp, acc[m]);
        if (VALUE) accv = fmaf(w[L.Wv + j], hp, accv);
    }
    int32_t g = 0;
    float best = 0.0f;
#pragma unroll
    for (int m = 0; m < kPolicyRowM; m++) {
        if (m < M) {
            emit(m, acc[m]);
            if (m == 0) best = acc[m];
            else if (acc[m] > best) { best = acc[m]; g = m; }
        }
    }
    if (VALUE) *value = accv;
    return g;
}

// ---------------------------------------------------------------------------
// The matrix engine of the learned policy (include/abr_env.h: abr_policy_mx; abr_env.hip: policy_mx_kernel): the same
// chains issued as v_mfma_f32_32x32x2_f32, the units of a layer as the rows of the product and 32 env lanes as its
// columns.  Everything here is index arithmetic, compiled for the host by tests/native/policy_matrix_harness.cpp.
//
// The instruction, for wave lane l (0..63): its A register is A[row l & 31][k = l >> 5], its B register is
// B[k = l >> 5][column l & 31], and register r (0..15) of its accumulator is D[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)]
// [column l & 31]; D = fma(A[.][1], B[1][.], fma(A[.][0], B[0][.], C)): k = 0 first.  Steps are issued with k
// ascending, so input k of a layer is k-slot k & 1 of step k >> 1.
//
// Unit u = 2 s + h of a 32-unit tile sits in row (s & 3) + 8 (s >> 2) + 4 h: accumulator register s of lane half h then
// holds unit 2 s + h, which after the ReLU is exactly that lane's B register of step s of the next layer -- the
// activations never leave the registers.  Rows past the layer's width and k-slots past its input are padded with
// -0.0f weights and biases against +0.0f inputs (the ReLU of a padded unit, whatever its chain made of -0 * x, is +0).
// ---------------------------------------------------------------------------
constexpr int kMxMaxWidth = 128, kMxMaxHidden = 3, kMxTile = 32, kMxWave = 64, kMxRegs = 16;
constexpr int kMxValueUnit = kPolicyMaxRates;             // the value head's row of the output tile (scores: 0..M-1)

ABR_HD int32_t mx_a_row(int32_t l) { return l & 31; }
ABR_HD int32_t mx_a_k(int32_t l) { return l >> 5; }
ABR_HD int32_t mx_b_k(int32_t l) { return l >> 5; }
ABR_HD int32_t mx_b_col(int32_t l) { return l & 31; }
ABR_HD int32_t mx_d_row(int32_t l, int32_t r) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }
ABR_HD int32_t mx_d_col(int32_t l) { return l & 31; }
// unit (within its tile) <-> row of the product
ABR_HD int32_t mx_unit_row(int32_t u) { const int32_t s = u >> 1, h = u & 1; return (s & 3) + 8 * (s >> 2) + 4 * h; }
ABR_HD int32_t mx_row_unit(int32_t i) { const int32_t h = (i >> 2) & 1, s = (i & 3) + 4 * (i >> 3); return 2 * s + h; }
// the unit (within its tile) that accumulator register r of lane l holds, and the next layer's step it feeds
ABR_HD int32_t mx_acc_unit(int32_t l, int32_t r) { return mx_row_unit(mx_d_row(l, r)); }
// where unit u (within its tile) of a column ends up: the accumulator register and the lane half that hold it
constexpr int32_t mx_unit_reg(int32_t u) { return u >> 1; }
constexpr int32_t mx_unit_half(int32_t u) { return u & 1; }

// One layer as the engine sees it: Wt [out][in] and b [out] in the blob; `extra` (the value head: Wv [in] then bv) is
// one more unit at row kMxValueUnit of the (only) tile, nullptr without one.
struct MxLayer { const float *W, *b; int32_t in, out; const float *extra; };

ABR_HD int32_t mx_steps(int32_t in) { return (in + 1) >> 1; }
ABR_HD int32_t mx_tiles(const MxLayer &y) { return ((y.extra ? kMxValueUnit + 1 : y.out) + kMxTile - 1) / kMxTile; }
// floats of the staged A operands: [tile][step][lane]
ABR_HD int32_t mx_staged_floats(const MxLayer &y) { return mx_tiles(y) * mx_steps(y.in) * kMxWave; }

ABR_HD float mx_weight(const MxLayer &y, int32_t unit, int32_t k) {
    if (k >= y.in) return -0.0f;
    if (unit < y.out) return y.W[(int64_t)unit * y.in + k];
    if (y.extra && unit == kMxValueUnit) return y.extra[k];
    return -0.0f;
}
ABR_HD float mx_bias(const MxLayer &y, int32_t unit) {
    if (unit < y.out) return y.b[unit];
    if (y.extra && unit == kMxValueUnit) return y.extra[y.in];
    return -0.0f;
}
// the A register of lane l at (tile T, step s), and its slot in the staged operands
ABR_HD float mx_staged_at(const MxLayer &y, int32_t T, int32_t s, int32_t l) {
    return mx_weight(y, kMxTile * T + mx_row_unit(mx_a_row(l)), 2 * s + mx_a_k(l));
}
ABR_HD int32_t mx_staged_slot(const MxLayer &y, int32_t T, int32_t s, int32_t l) {
    return (T * mx_steps(y.in) + s) * kMxWave + l;
}
// slot d of the staged operands: the A register of lane d & 63 at (tile, step) = divmod(d >> 6, steps)
ABR_HD float mx_staged(const MxLayer &y, int32_t d) {
    const int32_t l = d & (kMxWave - 1), q = d >> 6, steps = mx_steps(y.in), T = q / steps, s = q - T * steps;
    return mx_staged_at(y, T, s, l);
}

// layer li (0 .. n_hidden; n_hidden is the output layer) of a blob of hidden widths w[0..n_hidden) over F inputs and M
// outputs; head = the value head or nullptr
ABR_HD MxLayer mx_layer(const float *blob, const float *head, int32_t F, int32_t M, int32_t n_hidden, const int32_t *w,
                        int32_t li) {
    int64_t o = 0;
    int32_t in = F;
    for (int32_t l = 0; l < li; l++) { o += (int64_t)w[l] * in + w[l]; in = w[l]; }
    const int32_t out = li < n_hidden ? w[li] : M;
    return MxLayer{blob + o, blob + o + (int64_t)out * in, in, out, li == n_hidden ? head : nullptr};
}

// LDS floats of a launch: the largest staged layer; the SAMPLED instance's score columns ([M][block] floats) lie behind
// the output layer's operands (what lay there belonged to a layer every wave has left: a barrier precedes each staging)
ABR_HD int32_t mx_score_offset(int32_t F, int32_t n_hidden, const int32_t *w) {
    return mx_steps(n_hidden ? w[n_hidden - 1] : F) * kMxWave;
}
ABR_HD int32_t mx_lds_floats(int32_t F, int32_t M, int32_t n_hidden, const int32_t *w, bool sampled, int32_t block) {
    int32_t cap = mx_score_offset(F, n_hidden, w) + (sampled ? M * block : 0), in = F;
    for (int32_t l = 0; l < n_hidden; l++) {
        const int32_t need = ((w[l] + kMxTile - 1) / kMxTile) * mx_steps(in) * kMxWave;
        cap = need > cap ? need : cap;
        in = w[l];
    }
    return cap;
}

// ---------------------------------------------------------------------------
// The matrix engine of the recurrent policy (include/abr_env.h: abr_policy_gru_mx; abr_env.hip: policy_gru_mx_kernel):
// abr_policy_gru's chains on the same instruction.  The 3H gate rows are the rows of the product, a tile of 32 units at a
// time: unit j = 32 U + u of EVERY gate sits in row mx_unit_row(u) of its gate's product, so the six accumulators of a
// tile (gi and gh of r, z, n) hold unit 32 U + mx_acc_unit(l, r) in register r of lane l, and the gate arithmetic is
// element-wise on registers.  That unit is also input 2 (16 U + r) + (l >> 5) of the recurrent chains: register r of
// tile U sits where B register 16 U + r of h_in sits (d = h_in[j] - n needs no shuffle), and a tile's h' is, as it
// stands, the B operand of steps 16 U .. 16 U + 15 of the output layer.
//
// The staged operands of one unit tile are gru_mx_rows() rows of 64 floats (the A registers of one step): per gate the
// steps of W_ih then of W_hh, each rounded up to whole groups of kGruMxGroup steps (the kernel issues a group at a time
// and asks nothing of a step but its number: the rows past a chain's last step are pads), then the kMxRegs steps of the
// output layer (and the value head, row kMxValueUnit) that the tile's units feed.  Pads are -0.0f against +0.0f as
// above; a unit past H has -0.0f weights and biases and its h' is forced to +0.0f before it is folded into the outputs.
// ---------------------------------------------------------------------------
constexpr int kGruMxMaxHidden = 128, kGruMxMaxTiles = kGruMxMaxHidden / kMxTile, kGruMxGroup = 4;

// the blob of abr_policy_gru, by matrix; out is the output layer as the MLP's engine sees one (extra: the value head)
struct GruMx { const float *Wih, *Whh, *bih, *bhh; MxLayer out; int32_t F, H; };

ABR_HD GruMx gru_mx(const float *blob, const float *head, int32_t F, int32_t H, int32_t M) {
    const float *Wih = blob, *Whh = Wih + (int64_t)3 * H * F, *bih = Whh + (int64_t)3 * H * H, *bhh = bih + 3 * H,
                *Wout = bhh + 3 * H;
    return GruMx{Wih, Whh, bih, bhh, MxLayer{Wout, Wout + (int64_t)M * H, H, M, head}, F, H};
}

ABR_HD int32_t gru_mx_tiles(int32_t H) { return (H + kMxTile - 1) / kMxTile; }
// rows of one gate's staged operands (its W_ih steps, then its W_hh steps), and of a whole unit tile
ABR_HD int32_t gru_mx_chain_rows(int32_t in) { return (mx_steps(in) + kGruMxGroup - 1) / kGruMxGroup * kGruMxGroup; }
ABR_HD int32_t gru_mx_gate_rows(int32_t F, int32_t H) { return gru_mx_chain_rows(F) + gru_mx_chain_rows(H); }
ABR_HD int32_t gru_mx_rows(int32_t F, int32_t H) { return 3 * gru_mx_gate_rows(F, H) + kMxRegs; }
// the first row of gate g's W_ih steps, of its W_hh steps, and of the output steps
ABR_HD int32_t gru_mx_ih_row(int32_t F, int32_t H, int32_t g) { return g * gru_mx_gate_rows(F, H); }
ABR_HD int32_t gru_mx_hh_row(int32_t F, int32_t H, int32_t g) { return g * gru_mx_gate_rows(F, H) + gru_mx_chain_rows(F); }
ABR_HD int32_t gru_mx_out_row(int32_t F, int32_t H) { return 3 * gru_mx_gate_rows(F, H); }

// Gate g's weights and first terms for unit j (j >= H: a padded unit).  Every read is unconditional, from a clamped index,
// and the pad is selected afterwards: no branch on the device, where a wave's lanes straddle the last unit and the last k.
ABR_HD int32_t gru_mx_clamp(int32_t v, int32_t n) { return v < n ? v : n - 1; }
ABR_HD float gru_mx_w_ih(const GruMx &y, int32_t g, int32_t j, int32_t k) {
    const float w = y.Wih[((int64_t)g * y.H + gru_mx_clamp(j, y.H)) * y.F + gru_mx_clamp(k, y.F)];
    return j < y.H && k < y.F ? w : -0.0f;
}
ABR_HD float gru_mx_w_hh(const GruMx &y, int32_t g, int32_t j, int32_t k) {
    const float w = y.Whh[((int64_t)g * y.H + gru_mx_clamp(j, y.H)) * y.H + gru_mx_clamp(k, y.H)];
    return j < y.H && k < y.H ? w : -0.0f;
}
ABR_HD float gru_mx_b_ih(const GruMx &y, int32_t g, int32_t j) {
    const float b = y.bih[g * y.H + gru_mx_clamp(j, y.H)];
    return j < y.H ? b : -0.0f;
}
ABR_HD float gru_mx_b_hh(const GruMx &y, int32_t g, int32_t j) {
    const float b = y.bhh[g * y.H + gru_mx_clamp(j, y.H)];
    return j < y.H ? b : -0.0f;
}
// the output tile's weight (mx_weight's) and first term (mx_bias's) for row unit u: scores 0 .. M-1, the value head at
// kMxValueUnit, pads elsewhere
ABR_HD float gru_mx_w_out(const GruMx &y, int32_t u, int32_t k) {
    const bool score = u < y.out.out, value = y.out.extra && u == kMxValueUnit;
    const float *row = value ? y.out.extra : y.out.W + (int64_t)gru_mx_clamp(u, y.out.out) * y.H;
    const float w = row[gru_mx_clamp(k, y.H)];
    return (score || value) && k < y.H ? w : -0.0f;
}
ABR_HD float gru_mx_b_out(const GruMx &y, int32_t u) {
    const bool score = u < y.out.out, value = y.out.extra && u == kMxValueUnit;
    const float *at = value ? y.out.extra + y.H : y.out.b + gru_mx_clamp(u, y.out.out);
    const float b = *at;
    return score || value ? b : -0.0f;
}

// the A register of lane l in row q (0 .. gru_mx_rows) of unit tile U's staged operands
ABR_HD float gru_mx_staged_at(const GruMx &y, int32_t U, int32_t q, int32_t l) {
    const int32_t P = gru_mx_gate_rows(y.F, y.H), sF = gru_mx_chain_rows(y.F);   // a pad row: k past F or H
    const int32_t u = mx_row_unit(mx_a_row(l)), kk = mx_a_k(l);
    if (q >= 3 * P) return gru_mx_w_out(y, u, 2 * (kMxRegs * U + (q - 3 * P)) + kk);
    const int32_t g = (q >= P) + (q >= 2 * P), s = q - g * P, j = kMxTile * U + u;
    return s < sF ? gru_mx_w_ih(y, g, j, 2 * s + kk) : gru_mx_w_hh(y, g, j, 2 * (s - sF) + kk);
}

// LDS floats of a launch: one unit tile's staged operands, then the SAMPLED instances' score columns ([M][block])
ABR_HD int32_t gru_mx_score_offset(int32_t F, int32_t H) { return gru_mx_rows(F, H) * kMxWave; }
ABR_HD int32_t gru_mx_lds_floats(int32_t F, int32_t H, int32_t M, bool sampled, int32_t block) {
    return gru_mx_score_offset(F, H) + (sampled ? M * block : 0);
}

// The gates of one unit, in the order the engine retires its chains: r and z from their two chains each, then h' from
// the n gate's two, r, z and h_in[j].  live = false (a unit past H): +0.0f whatever the chains made of their pads, so
// that its term in every output chain is fmaf(-0, +0, acc) == acc.
ABR_HD float gru_mx_gate(float gi, float gh) { return sig_c(gi + gh); }
ABR_HD float gru_mx_unit(float r, float z, float gi_n, float gh_n, float hj, bool live) {
    const float n = tanh_c(fmaf(r, gh_n, gi_n));
    const float d = hj - n;
    const float hp = fmaf(z, d, n);
    return live ? hp : 0.0f;
}

// Policy populations (include/abr_env.h: abr_policy_pop): the member a workgroup serves and where its weights lie.
// block_first_lane is the LOCAL index of the workgroup's first lane (blockIdx.x * 256); group is a multiple of the
// workgroup size, so every lane of the workgroup has the same member.  Offsets are in floats from member 0.
ABR_HD int64_t pop_member(int64_t block_first_lane, int32_t group) { return block_first_lane / group; }
ABR_HD int64_t pop_blob_offset(int64_t member, int32_t blob_words) { return member * blob_words; }
ABR_HD int64_t pop_head_offset(int64_t member, int32_t head_words) { return member * head_words; }

// Generalised advantage estimation over [T][N] rollout slabs (include/abr_env.h: abr_gae), one lane.  Every operation is
// float32 with one rounding; q and w are selects, so a non-finite value behind an episode end never reaches the sum.
// rew(t), val(t) -> float; term(t) -> bool (any done bit); dead(t) -> bool (a step that took no decision);
// out(t, adv, ret).  Rows are taken in blocks of U, newest block first: a block's reads are all issued before its
// dependent chain starts (on the device U rows of loads are in flight while the previous block's arithmetic retires).
struct GaeCarry { float A, nv; };

template <int U, bool FULL, class Rew, class Val, class Term, class Dead, class Out>
ABR_HD void gae_block(GaeCarry &s, float gamma, float gl, int32_t lo, int32_t cnt, const Rew &rew, const Val &val,
                      const Term &term, const Dead &dead, const Out &out) {
    float r[U], v[U];
    bool tm[U], dd[U];
#if defined(__clang__)
#pragma unroll
#endif
    for (int u = 0; u < U; u++) {
        if (FULL || u < cnt) { r[u] = rew(lo + u); v[u] = val(lo + u); tm[u] = term(lo + u); dd[u] = dead(lo + u); }
    }
#if defined(__clang__)
#pragma unroll
#endif
    for (int u = U - 1; u >= 0; u--) {
        if (FULL || u < cnt) {
            if (dd[u]) {
                s.A = 0.0f; s.nv = 0.0f;
                out(lo + u, 0.0f, 0.0f);
            } else {
                const float q = tm[u] ? 0.0f : gamma * s.nv;
                const float delta = (r[u] + q) - v[u];
                const float w = tm[u] ? 0.0f : gl * s.A;
                s.A = delta + w;
                out(lo + u, s.A, s.A + v[u]);
                s.nv = v[u];
            }
        }
    }
}

template <int U, class Rew, class Val, class Term, class Dead, class Out>
ABR_HD void gae_lane(int32_t T, float gamma, float lam, float last_value, const Rew &rew, const Val &val,
                     const Term &term, const Dead &dead, const Out &out) {
    const float gl = gamma * lam;
    GaeCarry s{0.0f, last_value};
    int32_t hi = T;
    const int32_t part = T % U;                                // the newest rows that do not fill a block
    if (part) { hi -= part; gae_block<U, false>(s, gamma, gl, hi, part, rew, val, term, dead, out); }
    for (; hi > 0; hi -= U) gae_block<U, true>(s, gamma, gl, hi - U, U, rew, val, term, dead, out);
}

// The episode sampler (include/abr_env.h: abr_episode_sampler, the same layout): which (trace, start offset) episode e of
// global lane g runs when it was armed by the sampler.  A pure function of (seed, g, e), so every role of the split kernels
// computes it where it needs it.  Step 0xFFFFFFFF is never a chunk id: the draw shares no counter with the random policy
// or the policy's exploration, even under the same seed.
struct EpisodeSampler {
    uint64_t seed;
    const int32_t *pool;           // nullptr: the whole corpus
    int32_t n_pool;
    int32_t offset_span;           // 0: the whole trace
};
constexpr uint32_t kEpisodeStep = 0xFFFFFFFFu;

// trace_len: lengths of the n_traces traces (device memory in the kernels, host memory in tests/native)
ABR_HD void episode_assign(const EpisodeSampler &s, uint64_t g, uint32_t e, int32_t n_traces,
                           const int32_t *__restrict__ trace_len, int32_t &t_out, int32_t &off_out) {
    uint32_t w[4];
    philox4(s.seed, g, kEpisodeStep, e, w);
    const uint32_t n = s.pool ? (uint32_t)s.n_pool : (uint32_t)n_traces;
    const uint32_t u = (uint32_t)(((uint64_t)w[0] * n) >> 32);
    const int32_t t = s.pool ? s.pool[u] : (int32_t)u;
    const int32_t len = trace_len[t];
    const int32_t span = (s.offset_span > 0 && s.offset_span < len) ? s.offset_span : len;
    t_out = t;
    off_out = (int32_t)(((uint64_t)w[1] * (uint32_t)span) >> 32);
}

// The episode ledger (include/abr_env.h: abr_episode_ledger, the same layout): one record per finished episode, appended
// where the kernels write ep_qoe_terms.  The blob is struct-of-arrays with row stride n_lanes, every region 256-B aligned:
// count[N] int32 | total[5][N] float64 | rec_f64[rows][5][N] float64 | rec_i32[rows][5][N] int32.
struct EpisodeLedger {
    void *base;                    // nullptr: no ledger installed, ledger_append is never called
    int32_t rows;
    int32_t reserved_;
};
constexpr int kLedgerFields = 5;   // float64: rebuffer, start-up, latency, variance, qoe; int32: episode, trace, offset, chunks, done
struct LedgerLayout { size_t count, total, rec_f64, rec_i32, bytes; };   // byte offsets of the regions, and the blob's size
ABR_HD size_t ledger_align(size_t b) { return (b + 255) & ~(size_t)255; }
ABR_HD LedgerLayout ledger_layout(int64_t n_lanes, int32_t rows) {
    const size_t n = (size_t)n_lanes, r = (size_t)rows;
    LedgerLayout lo;
    lo.count = 0;
    lo.total = ledger_align(n * sizeof(int32_t));
    lo.rec_f64 = lo.total + ledger_align(kLedgerFields * n * sizeof(double));
    lo.rec_i32 = lo.rec_f64 + ledger_align(r * kLedgerFields * n * sizeof(double));
    lo.bytes = lo.rec_i32 + ledger_align(r * kLedgerFields * n * sizeof(int32_t));
    return lo;
}

// Append lane i's finished episode: the record goes to slot count % rows, the totals grow in episode order, count goes up
// by one.  qoe is calculate_qoe's sum in episode_qoe_kernel's order, so the newest record equals abr_env_episode_qoe.
ABR_HD void ledger_append(const EpisodeLedger &L, int64_t n_lanes, int64_t i, double wr, double wv, double ws, double wl,
                          double rebuffer, double start_up, double latency, double variance, int32_t episode,
                          int32_t trace_id, int32_t offset0, int32_t chunks, int32_t done) {
    const LedgerLayout lo = ledger_layout(n_lanes, L.rows);
    char *b = (char *)L.base;
    int32_t *count = (int32_t *)(b + lo.count);
    double *total = (double *)(b + lo.total), *rf = (double *)(b + lo.rec_f64);
    int32_t *ri = (int32_t *)(b + lo.rec_i32);
    const double qoe = wr * rebuffer + wv * variance + ws * start_up + wl * latency;
    const int32_t c = count[i];
    const int64_t slot = (int64_t)((uint32_t)c % (uint32_t)L.rows) * kLedgerFields;
    count[i] = c + 1;
    const double f[kLedgerFields] = {rebuffer, start_up, latency, variance, qoe};
    const int32_t w[kLedgerFields] = {episode, trace_id, offset0, chunks, done};
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < kLedgerFields; q++) {
        total[q * n_lanes + i] = total[q * n_lanes + i] + f[q];
        rf[(slot + q) * n_lanes + i] = f[q];
        ri[(slot + q) * n_lanes + i] = w[q];
    }
}

// The quality model (include/abr_env.h: abr_episode_quality, the same layout): a video-quality term of the QoE.  A step
// whose download completed takes u[chunk][action] off the reward, weighted, and adds it to the lane's running sum; the sum
// is recorded where the kernels write ep_qoe_terms.  The blob is struct-of-arrays with row stride n_lanes, every region
// 256-B aligned: count[N] int32 | q_run[N] | q_last[N] | total_q[N] | rec_q[rows][N], float64.
struct EpisodeQuality {
    double wq;
    const double *u;               // [video_length][n_rates], the caller's table
    void *base;                    // nullptr: no quality model installed, quality_step / quality_close are never called
    int32_t rows;
    int32_t reserved_;
};
struct QualityLayout { size_t count, q_run, q_last, total_q, rec_q, bytes; };   // byte offsets of the regions, and the blob's size
ABR_HD QualityLayout quality_layout(int64_t n_lanes, int32_t rows) {
    const size_t n = (size_t)n_lanes, r = (size_t)rows;
    QualityLayout lo;
    lo.count = 0;
    lo.q_run = ledger_align(n * sizeof(int32_t));
    lo.q_last = lo.q_run + ledger_align(n * sizeof(double));
    lo.total_q = lo.q_last + ledger_align(n * sizeof(double));
    lo.rec_q = lo.total_q + ledger_align(n * sizeof(double));
    lo.bytes = lo.rec_q + ledger_align(r * n * sizeof(double));
    return lo;
}

// Lane i has completed the download of `chunk` at rate `action`: its running sum grows by the table's entry (a read-modify-
// write of the lane's own element: the same thread serves the lane throughout).  Returns the weighted entry wq * q, which
// the caller takes off the step's float64 reward: one multiply here, one subtract there.  The kernels call this inside the
// branch that records the download and subtract outside it (a step without a download subtracts 0.0, which changes no
// bit of any reward), so that the QUALITY instances have no divergent branch the others lack.
ABR_HD double quality_step(const EpisodeQuality &Q, int64_t n_lanes, int32_t n_rates, int64_t i, int32_t chunk,
                           int32_t action) {
    double *q_run = (double *)((char *)Q.base + quality_layout(n_lanes, 1).q_run);      // in front of the ring: no rows in it
    const double q = Q.u[(int64_t)chunk * n_rates + action];
    q_run[i] = q_run[i] + q;
    return Q.wq * q;
}

// Lane i's episode has ended (called where ledger_append is): the running sum becomes the lane's last one, goes to slot
// count % rows and into the total, count goes up by one.  rearm: the lane starts its next episode in this same step.
ABR_HD void quality_close(const EpisodeQuality &Q, int64_t n_lanes, int64_t i, bool rearm) {
    const QualityLayout lo = quality_layout(n_lanes, Q.rows);
    char *b = (char *)Q.base;
    int32_t *count = (int32_t *)(b + lo.count);
    double *q_run = (double *)(b + lo.q_run), *q_last = (double *)(b + lo.q_last), *total_q = (double *)(b + lo.total_q),
           *rec_q = (double *)(b + lo.rec_q);
    const double q = q_run[i];
    const int32_t c = count[i];
    const int64_t slot = (int64_t)((uint32_t)c % (uint32_t)Q.rows);
    count[i] = c + 1;
    q_last[i] = q;
    rec_q[slot * n_lanes + i] = q;
    total_q[i] = total_q[i] + q;
    if (rearm) q_run[i] = 0.0;
}

// abr_env_reset abandons lane i's episode: its running sum starts again at zero; nothing else of the blob moves
ABR_HD void quality_reset(const EpisodeQuality &Q, int64_t n_lanes, int64_t i) {
    double *q_run = (double *)((char *)Q.base + quality_layout(n_lanes, 1).q_run);
    q_run[i] = 0.0;
}

// The trace generator (include/abr_env.h: abr_trace_synth; abr_trace_model has the same layout, abr_env.hip asserts it): a
// Markov chain over K <= 8 bandwidth regimes.  A sample's philox word w0 fixes where EVERY state would go next, so the
// sample is a map of the 8 states onto themselves, packed 3 bits per source state, and the chain over a trace is the
// composition of its samples' maps: an associative operation, which a wave scans (abr_env.hip: trace_synth_kernel).  The
// model reaches the kernel by value, so nothing here indexes one of its arrays by a runtime value outside a fully unrolled
// loop: every access is a static one (kernel-argument loads, no scratch copy).
constexpr int kTraceMaxStates = 8;
constexpr uint64_t kTraceKey = 0x5452414345535953ull;      // xor-ed into the seed: no counter shared with another philox user
constexpr uint32_t kTraceInitStep = 0xFFFFFFFFu;           // the step word of the initial-state block: never a sample index
constexpr uint32_t kTraceIdentity = 0xFAC688u;             // the map s -> s: sum of s << 3 s
struct TraceModel {
    int32_t n_states, reserved_;
    double level[kTraceMaxStates], spread[kTraceMaxStates];
    uint64_t outage_thr[kTraceMaxStates], init_cum[kTraceMaxStates], cum[kTraceMaxStates][kTraceMaxStates];
};

// #{ j < K - 1 : w0 >= row[j] }: the state a cumulative row sends w0 to
ABR_HD uint32_t trace_pick(const uint64_t (&row)[kTraceMaxStates], int32_t K, uint32_t w0) {
    uint32_t n = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 0; j < kTraceMaxStates - 1; j++) n += (j < K - 1 && (uint64_t)w0 >= row[j]) ? 1u : 0u;
    return n;
}

// the sample's state map; a source state >= K (never reached) maps to itself
ABR_HD uint32_t trace_map(const TraceModel &m, uint32_t w0) {
    uint32_t F = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int s = 0; s < kTraceMaxStates; s++) F |= (s < m.n_states ? trace_pick(m.cum[s], m.n_states, w0) : (uint32_t)s) << (3 * s);
    return F;
}

ABR_HD uint32_t trace_apply(uint32_t F, uint32_t s) { return (F >> (3 * s)) & 7u; }

// g after f
ABR_HD uint32_t trace_compose(uint32_t g, uint32_t f) {
    uint32_t r = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int s = 0; s < kTraceMaxStates; s++) r |= trace_apply(g, trace_apply(f, (uint32_t)s)) << (3 * s);
    return r;
}

ABR_HD uint32_t trace_initial(const TraceModel &m, uint32_t w0) { return trace_pick(m.init_cum, m.n_states, w0); }

// the sample of state s: a select chain over the states, so that s never indexes the model
ABR_HD double trace_value(const TraceModel &m, uint32_t s, uint32_t w1, uint32_t w2) {
    double level = m.level[0], spread = m.spread[0];
    uint64_t thr = m.outage_thr[0];
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 1; j < kTraceMaxStates; j++) {
        level = s == (uint32_t)j ? m.level[j] : level;
        spread = s == (uint32_t)j ? m.spread[j] : spread;
        thr = s == (uint32_t)j ? m.outage_thr[j] : thr;
    }
    const double u = (double)(w1 >> 8) * 0x1p-24;
    const double r = 2.0 * u - 1.0;
    const double x = level * (1.0 + spread * r);
    return (uint64_t)w2 < thr ? 0.0 : x;
}

// Lane fork (include/abr_env.h: abr_env_fork): lane dst[i] becomes a copy of lane src[i] as it was before the call.  All
// lane state is struct-of-arrays with row stride n_lanes, so a lane is one COLUMN of every region below, and the fork is a
// column gather into the caller's scratch ([row][pair]: adjacent pairs write adjacent elements) followed by a column scatter
// -- two launches, so that src and dst may overlap in any way.  The row table is this one definition: abr_env.hip fills it
// from the handle, tests/native/fork_harness.cpp from a host byte array, and both run fork_move below.
constexpr int kForkRegions = 10;
enum ForkRegionId { kForkF64 = 0, kForkI64, kForkI32, kForkU8, kForkActionHist, kForkBwHist, kForkEpTerms, kForkMpcAction,
                    kForkQRun, kForkObs };
constexpr int kForkRowsPerThread = 8;      // a thread moves up to this many rows of one region for one pair
struct ForkRegion {
    char *base;                    // element (row, lane) at base + (row * stride + lane) * elem; nullptr: region absent
    int32_t elem;                  // 8, 4 or 1 bytes: the region's own element, the widest access its alignment allows (a u8
                                   // row starts at a multiple of n_lanes, which is odd for an odd lane count)
    int32_t rows;
    int64_t stride;                // elements between two rows: n_lanes for every region
    int64_t scratch;               // byte offset of the region's [rows][count] image in the scratch
};
struct ForkTable {
    ForkRegion r[kForkRegions];
    int64_t n_lanes, count;
    int32_t chunks;                // row chunks over all regions: the y extent of the launch
    int32_t reserved_;
};
// elem and rows of every region for episodes of V chunks; q_run and obs are reserved in the scratch whether present or not
ABR_HD void fork_region_shape(int id, int32_t V, int32_t &elem, int32_t &rows) {
    switch (id) {
    case kForkF64: elem = 8; rows = 8; break;
    case kForkI64: elem = 8; rows = 1; break;
    case kForkI32: elem = 4; rows = 15; break;
    case kForkU8: elem = 1; rows = 2; break;
    case kForkActionHist: elem = 1; rows = V; break;
    case kForkBwHist: elem = 8; rows = V; break;
    case kForkEpTerms: elem = 8; rows = 4; break;
    case kForkMpcAction: elem = 4; rows = 1; break;
    case kForkQRun: elem = 8; rows = 1; break;
    default: elem = 4; rows = 8; break;          // kForkObs: float32 [ABR_OBS_DIM][n_lanes]
    }
}
// Shapes, scratch offsets (each region at the next multiple of 256 bytes) and the chunk count; bases are the caller's to
// set.  Returns the scratch bytes `count` pairs need.
ABR_HD size_t fork_table_init(ForkTable &T, int32_t V, int64_t n_lanes, int64_t count) {
    size_t o = 0;
    int32_t chunks = 0;
    for (int id = 0; id < kForkRegions; id++) {
        ForkRegion &g = T.r[id];
        fork_region_shape(id, V, g.elem, g.rows);
        g.base = nullptr; g.stride = n_lanes; g.scratch = (int64_t)o;
        o = ledger_align(o + (size_t)g.rows * (size_t)count * (size_t)g.elem);
        chunks += (g.rows + kForkRowsPerThread - 1) / kForkRowsPerThread;
    }
    T.n_lanes = n_lanes; T.count = count; T.chunks = chunks; T.reserved_ = 0;
    return o;
}
// the index guard: a pair moves only when both of its lanes exist (src -1 is the documented "leave dst alone")
ABR_HD bool fork_pair_ok(int64_t s, int64_t d, int64_t n_lanes) { return s >= 0 && s < n_lanes && d >= 0 && d < n_lanes; }

// E: the element in memory; R: what a thread holds it in (a byte rides in a 32-bit register, so that the loads of a chunk
// need no packing between them and stay in flight together)
template <typename E, typename R>
ABR_HD void fork_rows(const ForkRegion &g, int32_t r0, int32_t r1, int64_t lane, int64_t i, int64_t count, char *scratch,
                      bool scatter) {
    E *col = (E *)g.base + lane;
    E *img = (E *)(scratch + g.scratch) + i;
    R v[kForkRowsPerThread];
    // all loads of the chunk first, then all stores: up to kForkRowsPerThread independent accesses in flight per thread
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < kForkRowsPerThread; q++)
        if (r0 + q < r1) v[q] = scatter ? img[(int64_t)(r0 + q) * count] : col[(int64_t)(r0 + q) * g.stride];
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < kForkRowsPerThread; q++)
        if (r0 + q < r1) {
            if (scatter) col[(int64_t)(r0 + q) * g.stride] = (E)v[q]; else img[(int64_t)(r0 + q) * count] = (E)v[q];
        }
}
// One thread's work: pair i, row chunk `chunk` (the same for a whole workgroup, so the region search is wave-uniform).
// scatter == false: the source lane's elements go to the scratch; true: the scratch's go to the destination lane.
ABR_HD void fork_move(const ForkTable &T, int32_t chunk, int64_t i, const int32_t *__restrict__ src,
                      const int32_t *__restrict__ dst, char *scratch, bool scatter) {
    if (i < 0 || i >= T.count || chunk < 0 || chunk >= T.chunks) return;
    const int64_t s = src[i], d = dst ? (int64_t)dst[i] : i;
    if (!fork_pair_ok(s, d, T.n_lanes)) return;
    // the region of this chunk, by a select chain over a fully unrolled loop: the table arrives by value (kernel
    // arguments), and indexing it with a run-time value would copy it to scratch memory first
    ForkRegion g = T.r[0];
    int32_t c = chunk;
    bool found = false;
#if defined(__clang__)
#pragma unroll
#endif
    for (int id = 0; id < kForkRegions; id++) {
        const int32_t n = (T.r[id].rows + kForkRowsPerThread - 1) / kForkRowsPerThread;
        const bool here = !found && c < n;
        g.base = here ? T.r[id].base : g.base; g.elem = here ? T.r[id].elem : g.elem; g.rows = here ? T.r[id].rows : g.rows;
        g.stride = here ? T.r[id].stride : g.stride; g.scratch = here ? T.r[id].scratch : g.scratch;
        c = (found || here) ? c : c - n;
        found = found || here;
    }
    if (!found || !g.base) return;
    const int32_t r0 = c * kForkRowsPerThread;
    const int32_t r1 = r0 + kForkRowsPerThread < g.rows ? r0 + kForkRowsPerThread : g.rows;
    const int64_t lane = scatter ? d : s;
    if (g.elem == 8) fork_rows<uint64_t, uint64_t>(g, r0, r1, lane, i, T.count, scratch, scatter);
    else if (g.elem == 4) fork_rows<uint32_t, uint32_t>(g, r0, r1, lane, i, T.count, scratch, scatter);
    else fork_rows<uint8_t, uint32_t>(g, r0, r1, lane, i, T.count, scratch, scatter);
}

// Beam selection (include/abr_env.h: abr_beam_select): the score of one candidate slot and the order of two of them.  All
// float64, unfused.  R_new is the running sum of the float32 step rewards in step order; the key adds the latency term the
// step reward leaves out, or is the caller's.
constexpr uint8_t kBeamDoneEpisode = 0x1;  // ABR_DONE_EPISODE: the one done bit a live candidate may carry
ABR_HD double beam_r_new(double R_in, float reward) { return R_in + (double)reward; }
ABR_HD double beam_key(double R_new, double wl, double lat) { return R_new + wl * lat; }
ABR_HD bool beam_valid(uint8_t valid_in, uint8_t done, double key) {
    return valid_in != 0 && !(done & (uint8_t)~kBeamDoneEpisode) && key == key;
}
// candidate t ranks before candidate s: the smaller key, ties (-0.0 and +0.0 among them) by the smaller slot
ABR_HD bool beam_before(double key_t, int32_t t, double key_s, int32_t s) {
    return key_t < key_s || (key_t == key_s && t < s);
}

// ---- the lookahead expert (include/abr_env.h: abr_env_lookahead_select) ----
// The quality term of a step without quality_step's side effect: the weighted table entry a completed download of `chunk`
// at rate `action` takes off the reward -- the same multiply on the same operands -- and q_run is left alone.
ABR_HD double quality_peek(const EpisodeQuality &Q, int32_t n_rates, int32_t chunk, int32_t action) {
    return Q.wq * Q.u[(int64_t)chunk * n_rates + action];
}

// Tree sizes.  M <= 16 and h <= 8: 16^8 fits an int64 with room to spare.
constexpr int64_t kLookMaxLeaves = 65536;            // one launch walks one decision's tree; larger trees are a beam search's
// Tree nodes one launch walks at most when the caller names no bound: 2^31.  Origin: at the 1.3e10 env-steps/s the README
// records for the environment kernel, and a node being one lanej_step, that is about a sixth of a second per launch -- short
// enough that the stream stays responsive.  The constant predates any measurement of this kernel's own rate.
constexpr int64_t kLookDefaultNodes = (int64_t)1 << 31;
ABR_HD constexpr int64_t look_leaves(int32_t M, int32_t h) {
    int64_t n = 1;
    for (int32_t j = 0; j < h; j++) n *= M;
    return n;
}
ABR_HD constexpr int64_t look_nodes(int32_t M, int32_t h) {    // M + M^2 + ... + M^h
    int64_t n = 0, pw = 1;
    for (int32_t j = 0; j < h; j++) { pw *= M; n += pw; }
    return n;
}
// lanes per launch: the largest multiple of 64 whose trees hold at most max_nodes nodes (0: the default), and at least 64
ABR_HD int64_t look_lanes_per_launch(int64_t max_nodes, int32_t M, int32_t h) {
    const int64_t lanes = (max_nodes > 0 ? max_nodes : kLookDefaultNodes) / look_nodes(M, h) / 64 * 64;
    return lanes < 64 ? 64 : lanes;
}

struct LookWeights {
    double wr, ws, wv, wl;
    int32_t M;
    bool quality;                  // a quality model is installed: the step reward carries its term
};
// One node of the tree: the lane after the node's step, the sum of the float32 rewards down to it, and whether anything is
// left below (false: timed out, finished, or not a lane at all).  The two clocks a step's reward starts from are the
// parent's own n_rb and n_su (what the kernels keep as n_rb_obs / n_su_obs after every step), so a node saves neither.
struct LookNode {
    LaneJ s;
    double R;
    bool live;
};
// candidate `key` replaces `best` when it is a number and smaller; equal keys (-0.0 and +0.0 among them) keep the earlier one
ABR_HD bool look_better(double key, double best) { return key == key && !(best <= key); }

// Depth first, one saved node per level, reached by template recursion: LVL is a compile-time index, so the stack is H
// named objects (registers on the device) and never an array indexed at run time.  The digits of the sequence are the loop
// counters m: the same in every lane of a wave (`any` folds the lanes' live flags, so the loops and the early-out are uniform
// control flow); the only divergence is under `if (c.live)`.  Accessors: br(chunk, rate), G(n), lat(lane) = average_latency
// of a lane state, qt(chunk, rate) = the weighted quality term, any(flag) = the flag in some lane of the wave (the host
// harness: the flag itself).  Visits children in rate order and keeps the first least key: ties go to the
// lexicographically smaller sequence.
// sz(chunk, a, rate) = the step's target_size, rate being br(chunk, a): rate * t.L, or the environment's size table's entry
// (include/abr_env.h: abr_env_set_size_table), which decides what is downloaded while `rate` keeps deciding what is scored.
template <int LVL, int H, class TB, class BR, class SZ, class GT, class LAT, class QT, class ANY>
ABR_HD void look_visit(const LookWeights &w, const TB &t, const BR &br, const SZ &sz, const GT &G, const LAT &lat,
                       const QT &qt, const ANY &any, const LookNode &par, int32_t n_rb_obs, int32_t n_su_obs, int32_t a,
                       double &best) {
    LookNode c = par;
    if (c.live) {
        const int32_t prev = c.s.last_action, chunk = c.s.chunk_id;
        const double rate = br(chunk, a);
        const StepResult r = lanej_step(c.s, t, sz(chunk, a, rate), a);
        const double g_rb = G(c.s.n_rb), g_su = G(c.s.n_su);
        double var = 0.0;
        if (r.hit && prev >= 0) var = fabs(rate - br(chunk - 1, prev));
        double rew = w.wr * (g_rb - G(n_rb_obs)) + w.ws * (g_su - G(n_su_obs)) + w.wv * var;
        if (w.quality) rew = rew - (r.hit ? qt(chunk, a) : 0.0);
        c.R = c.R + (double)(float)rew;                  // reward_out's rounding: abr_beam_select's sum
        const bool last = r.ended || LVL + 1 == H;       // h = min(H, V - chunk_id): the episode's end closes a sequence
        c.live = !r.timeout && !last;
        if (!r.timeout && last) {
            const double key = c.R + w.wl * lat(c.s);
            if (look_better(key, best)) best = key;
        }
    }
    if constexpr (LVL + 1 < H) {
        if (any(c.live))
            for (int32_t m = 0; m < w.M; m++) look_visit<LVL + 1, H>(w, t, br, sz, G, lat, qt, any, c, c.s.n_rb, c.s.n_su, m, best);
    }
}

// q[a0] of one lane: the least key over the valid sequences that start with a0 from `root` (n_rb_obs / n_su_obs: the lane's
// clocks at its last reported step), NaN when there is none or the lane is not live
template <int H, class TB, class BR, class SZ, class GT, class LAT, class QT, class ANY>
ABR_HD double look_subtree(const LookWeights &w, const TB &t, const BR &br, const SZ &sz, const GT &G, const LAT &lat,
                           const QT &qt, const ANY &any, const LaneJ &root, bool live, int32_t n_rb_obs, int32_t n_su_obs,
                           int32_t a0) {
    LookNode n;
    n.s = root; n.R = 0.0; n.live = live;
    double best = __builtin_nan("");
    look_visit<0, H>(w, t, br, sz, G, lat, qt, any, n, n_rb_obs, n_su_obs, a0, best);
    return best;
}
// without a size table: every target is bitrate x chunk_length
template <int H, class TB, class BR, class GT, class LAT, class QT, class ANY>
ABR_HD double look_subtree(const LookWeights &w, const TB &t, const BR &br, const GT &G, const LAT &lat, const QT &qt,
                           const ANY &any, const LaneJ &root, bool live, int32_t n_rb_obs, int32_t n_su_obs, int32_t a0) {
    const auto sz = [&](int32_t, int32_t, double rate) { return rate * t.L; };
    return look_subtree<H>(w, t, br, sz, G, lat, qt, any, root, live, n_rb_obs, n_su_obs, a0);
}

// the lane's answer from its q column: the first least q(m), or -1 and NaN
template <class Q>
ABR_HD void look_pick(const Q &q, int32_t M, int32_t &action, double &key) {
    action = -1; key = __builtin_nan("");
    for (int32_t m = 0; m < M; m++) {
        const double v = q(m);
        const bool take = look_better(v, key);
        action = take ? m : action; key = take ? v : key;
    }
}

// ---- forecast MPC (include/abr_env.h: abr_plan_config): the same walk on a predicted bandwidth ----
// The built-in forecast of one lane at chunk c: RobustMPC's estimate on the lane's rows of `state`, or, with state ==
// nullptr, the same arithmetic with no error ever stored (P = hm; nothing is read or written).  0.0: no decision, and a
// finished lane takes none and keeps its state.
template <class HIST>
ABR_HD double plan_forecast(int32_t W, bool done, int32_t c, const HIST &hist, uint8_t *state, int64_t N, int64_t lane) {
    if (done) return 0.0;
    if (state) return robust_estimate_rows(W, c, hist, state, N, lane);
    int32_t cs1 = 0, cnt = 0;
    double ps = 0.0, none = 0.0;
    return robust_estimate(W, c, hist, cs1, cnt, ps, [&](int32_t) -> double & { return none; });
}
// a forecast the walk can plan on: finite and > 0 (NaN fails both comparisons)
ABR_HD bool plan_usable(double P) { return P > 0.0 && P <= 1.79769313486231570815e+308; }
// the root's cursor: a one-sample trace at *P, so that every interval the walk downloads in has bandwidth *P (trace_wrap
// folds the six-sample look-ahead of lanej_begin_load onto it); cur.j, the clock's interval index, stays the lane's
ABR_HD void plan_cursor(Cursor &c, const double *P) { c.trace = P; c.tlen = 1; c.tpos = 0; }

}  // namespace abrx
#endif
