// CPU harness for the two guard forms of chain_segment (abr_exact_jump.h: GuardKind) and for the callers' side of the proven
// one (abr_lane_jump.h: chains_proven, TablesT<false>::kGuards).
//   guards_check   chains on given inputs: proven == checked == the naive loop, bits of x, the count and the hit flag, and
//                  (values below 2^1023) the same number of segments in both forms;
//   cg_*           episodes through the lane functions on the no-speeds tables (proven chains) and on the general tables
//                  (checked chains), side by side; a hook on every call of the proven form counts the calls and those that
//                  break a precondition (budget outside 1..2^20, a value that is not finite);
//   cg_proven      the handle's proof for a configuration, on the tick tables abr_env_create builds.
// Built two ways by tests/test_chain_guards_cpu.py: as a shared library (helpers.native_harness), and with
// -DCHAIN_GUARDS_MAIN as a stand-alone program (the sanitizer build) that reads the chain cases from a file and replays a
// built-in set of episodes.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int64_t g_segments = 0;                     // every chain_segment call
static int64_t g_proven_calls = 0, g_proven_bad = 0;
static void proven_hook(int32_t n, double x);
#define ABR_SEGMENT_HOOK(STOP) (g_segments++)
#define ABR_PROVEN_HOOK(STOP, n, x) proven_hook((n), (x))
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

using namespace abrx;

static void proven_hook(int32_t n, double x) {
    g_proven_calls++;
    if (n < 1 || n > kJumpCap || !(fabs(x) <= 1.7976931348623157e308)) g_proven_bad++;
}

template <int STOP>
static bool naive(double &x, double c, double thr, int32_t n, int32_t &a) {
    a = 0;
    while (a < n) {
        x = x + c;
        a++;
        if (stop_hit<STOP>(x, thr)) return true;
    }
    return false;
}

static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

// stats[0] += segments of the checked form, stats[1] += segments of the proven form, stats[2] += hits
template <int STOP, int BIAS>
static int64_t run(const double *x0, const double *c, const double *thr, const int32_t *n, int64_t cases, int64_t *stats) {
    for (int64_t i = 0; i < cases; i++) {
        double xn = x0[i], xc = x0[i], xp = x0[i];
        int32_t an = 0, ac = 0, ap = 0;
        const bool hn = naive<STOP>(xn, c[i], thr[i], n[i], an);
        int64_t s0 = g_segments;
        const bool hc = chain<STOP, BIAS, SETTLE_REMAINDER, GUARDS_CHECKED>(xc, c[i], thr[i], n[i], ac);
        const int64_t seg_c = g_segments - s0;
        s0 = g_segments;
        const bool hp = chain<STOP, BIAS, SETTLE_REMAINDER, GUARDS_PROVEN>(xp, c[i], thr[i], n[i], ap);
        const int64_t seg_p = g_segments - s0;
        if (bits(xp) != bits(xn) || ap != an || hp != hn) { stats[3] = 1; return i; }
        if (bits(xc) != bits(xn) || ac != an || hc != hn) { stats[3] = 2; return i; }
        // the same trips: `can` is the same predicate below 2^1023 (a spoiled estimate moves both forms alike)
        if (fabs(x0[i]) < 0x1p1022 && fabs(xn) < 0x1p1022 && seg_p != seg_c) { stats[3] = 3; return i; }
        if (seg_p > seg_c) { stats[3] = 3; return i; }
        stats[0] += seg_c; stats[1] += seg_p; stats[2] += hn ? 1 : 0;
    }
    return -1;
}

// ---- episodes through the lane functions ----
struct Ctx {
    TickTables tt;
    TablesT<false> tp;       // proven chains
    Tables tc;               // checked chains, no speed feature on
    double ladder[16];
    int n_rates;
    bool proven;             // chains_proven() of this configuration
};

template <class TB>
static void fill(TB &t, const TickTables &tt, double L, double max_buffer, double start_up_length, int32_t V, int32_t max_ticks) {
    t.G = tt.G.data(); t.interval_tick = tt.interval_tick.data(); t.avail_tick = tt.avail_tick.data();
    t.L = L; t.sd = tt.sd; t.max_buffer = max_buffer; t.start_up_length = start_up_length;
    t.V = V; t.max_ticks = max_ticks;
    t.drain = make_drain_tab(tt.sd, max_buffer + L);     // as abr_env_create does
}

// One episode on tables TB.  rec[s*8 + ..] as tests/native/lane_jump_harness.cpp: global_time, rebuffer_time, start_up_time,
// play_time, buffer_level, last_bw, sumk, flags; fin[0..5]; fin_i[0] = n_play.  Also runs the download side's call-site
// prediction at every decision (its chains are part of what the tables select) and folds its answer into `pred`.
template <class TB>
static int episode(const Ctx *c, const TB &t, const double *trace, int32_t tlen, int32_t offset, const int32_t *actions,
                   double *rec, double *bw_out, double *fin, int32_t *fin_i, int64_t *pred) {
    LaneJ s;
    s.cur.trace = trace; s.cur.tlen = tlen;
    s.sd = t.sd; s.pt = 0.0; s.pl_left = 0; s.play_id = 0; s.pt_sum = 0.0; s.lane = 0;
    lanej_init(s, t, offset);
    if (!lanej_wait_call(s, t)) return -2;
    double last_bw = 0.0;
    for (int step = 0; step < t.V; step++) {
        double *r = rec + (size_t)step * 8;
        r[0] = t.G[s.k]; r[1] = t.G[s.n_rb]; r[2] = t.G[s.n_su]; r[3] = c->tt.GP[s.n_play];
        r[4] = s.buf; r[5] = last_bw; r[6] = (double)s.sumk;
        r[7] = (double)((s.su ? 1 : 0) | (s.be ? 2 : 0) | (s.bf ? 4 : 0));
        const int a = actions[step];
        const double buf0 = s.buf; const bool su0 = s.su, be0 = s.be; const int32_t k0 = s.k;
        const StepStart st = lanej_begin_step(s.cur, t, s.k, s.chunk_id);
        const Download dd = lanej_download(s.cur, t, st, s.k, c->ladder[a] * t.L);
        StepResult sr = lanej_after_download(s, t, dd, st.avail_next, a);
        if (sr.timeout) return -2;
        if (!sr.ended && dd.hit && lanej_gate_possible(buf0, su0, be0, dd.n_dl, t)) {
            int32_t kn = -1;
            if (lanej_predict_next_call(buf0, k0, dd.n_dl, st.avail_next, t, kn)) {
                if (kn != s.k) return -7;
                *pred += kn;
            }
        }
        last_bw = sr.bw;
        bw_out[step] = sr.bw;
        if (sr.ended != (step == t.V - 1)) return -5;
    }
    fin[0] = t.G[s.k]; fin[1] = t.G[s.n_rb]; fin[2] = t.G[s.n_su]; fin[3] = c->tt.GP[s.n_play];
    fin[4] = s.buf; fin[5] = (double)s.sumk;
    fin_i[0] = s.n_play; fin_i[1] = 0;
    return 0;
}

extern "C" {

// kind: 0 >=, 1 <=, 2 <; bias: 0, +4, -4.  Every n must be in 1..kJumpCap and every value finite (the proven form's
// preconditions): -3 if one is not.  Returns the first failing case or -1; stats[3] = why (1: proven != naive, 2: checked !=
// naive, 3: the trips differ); -2: bad arguments.
int64_t guards_check(int32_t kind, int32_t bias, const double *x0, const double *c, const double *thr, const int32_t *n,
                     int64_t cases, int64_t *stats) {
    for (int64_t i = 0; i < cases; i++)
        if (n[i] < 1 || n[i] > kJumpCap || !isfinite(x0[i]) || !isfinite(c[i]) || !isfinite(thr[i])) return -3;
    g_proven_bad = 0;
    int64_t r = -2;
#define ABR_CASE(K, B) if (kind == (K) && bias == (B)) r = run<(K), (B)>(x0, c, thr, n, cases, stats);
    ABR_CASE(0, 0) ABR_CASE(0, 4) ABR_CASE(0, -4)
    ABR_CASE(1, 0) ABR_CASE(1, 4) ABR_CASE(1, -4)
    ABR_CASE(2, 0) ABR_CASE(2, 4) ABR_CASE(2, -4)
#undef ABR_CASE
    if (r == -1 && g_proven_bad) { stats[3] = 4; return 0; }
    return r;
}
int32_t guards_jump_cap() { return kJumpCap; }

void *cg_create(double interval, double L, double speed, int32_t V, double max_buffer, double start_up_length,
                int32_t max_ticks, const double *ladder, int32_t n_rates) {
    Ctx *c = new Ctx;
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    c->tt = build_tick_tables(interval, L, speed, V, max_ticks, n_iv);
    fill(c->tp, c->tt, L, max_buffer, start_up_length, V, max_ticks);
    fill(c->tc, c->tt, L, max_buffer, start_up_length, V, max_ticks);
    c->tc.per_lane_speed = false; c->tc.speed_rows = 0; c->tc.speed_stride = 0; c->tc.speeds = nullptr;
    c->n_rates = n_rates;
    for (int i = 0; i < n_rates && i < 16; i++) c->ladder[i] = ladder[i];
    c->proven = chains_proven(c->tt.interval_tick.data(), c->tt.interval_tick.size(), max_ticks, c->tt.sd, L, max_buffer,
                              ladder, n_rates);
    return c;
}
void cg_destroy(void *h) { delete (Ctx *)h; }
// the handle's proof (abr_env_create computes exactly this and launch_env routes on it)
int32_t cg_proven(void *h) { return ((Ctx *)h)->proven ? 1 : 0; }

// n_lanes episodes on the tables launch_env would pick: the no-speeds tables (proven chains) when the proof holds, else the
// general ones; when the proof holds the general tables run next to them and every output must agree bit for bit.
// stats[0] = calls of the proven form, [1] = of them outside its preconditions, [2] = segments on the proven tables,
// [3] = segments on the checked tables (the same episodes).  Returns 0, -(1000 + 10 * lane + code) on a failing episode,
// -1 - lane when the two tables disagree.
int64_t cg_batch(void *h, const double *traces, const int64_t *trace_off, const int32_t *trace_len, const int32_t *trace_id,
                 const int32_t *offset, const int32_t *actions, int32_t n_lanes, double *rec, double *bw_out, double *fin,
                 int32_t *fin_i, int64_t *stats) {
    Ctx *c = (Ctx *)h;
    const int V = c->tc.V;
    std::vector<double> rec2((size_t)V * 8), bw2((size_t)V);
    double fin2[6];
    int32_t fi2[2];
    g_proven_calls = g_proven_bad = 0;
    stats[2] = stats[3] = 0;
    for (int32_t i = 0; i < n_lanes; i++) {
        const int tid = trace_id[i];
        const double *tr = traces + trace_off[tid];
        double *r1 = rec + (size_t)i * V * 8, *b1 = bw_out + (size_t)i * V, *f1 = fin + (size_t)i * 6;
        int32_t *i1 = fin_i + (size_t)i * 2;
        int64_t p1 = 0, p2 = 0;
        int64_t s0 = g_segments;
        int rc = c->proven ? episode(c, c->tp, tr, trace_len[tid], offset[i], actions + (size_t)i * V, r1, b1, f1, i1, &p1)
                           : episode(c, c->tc, tr, trace_len[tid], offset[i], actions + (size_t)i * V, r1, b1, f1, i1, &p1);
        if (rc) return -(1000 + (int64_t)i * 10 - rc);
        (c->proven ? stats[2] : stats[3]) += g_segments - s0;
        if (!c->proven) continue;
        s0 = g_segments;
        rc = episode(c, c->tc, tr, trace_len[tid], offset[i], actions + (size_t)i * V, rec2.data(), bw2.data(), fin2, fi2, &p2);
        if (rc) return -(1000 + (int64_t)i * 10 - rc);
        stats[3] += g_segments - s0;
        if (memcmp(r1, rec2.data(), sizeof(double) * V * 8) || memcmp(b1, bw2.data(), sizeof(double) * V) ||
            memcmp(f1, fin2, sizeof(fin2)) || i1[0] != fi2[0] || p1 != p2)
            return -1 - (int64_t)i;
    }
    stats[0] = g_proven_calls; stats[1] = g_proven_bad;
    return 0;
}
}

#ifdef CHAIN_GUARDS_MAIN
// File: int64 blocks; per block int32 kind, int32 bias, int32 0, int32 0, int64 cases, then x0[], c[], thr[] (float64) and
// n[] (int32).  Then a built-in replay: episodes of random actions on seeded traces (zeros, tiny and huge samples among
// them), proven against checked.  Prints "ok <cases> <proven calls>" and exits 0 when everything passes.
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t blocks = 0, total = 0;
    if (fread(&blocks, 8, 1, f) != 1) return 2;
    for (int64_t b = 0; b < blocks; b++) {
        int32_t kb[4];
        int64_t cases = 0, stats[4] = {0, 0, 0, 0};
        if (fread(kb, 4, 4, f) != 4 || fread(&cases, 8, 1, f) != 1 || cases < 0) return 2;
        const size_t N = (size_t)cases;
        std::vector<double> x0(N + 1), c(N + 1), thr(N + 1);
        std::vector<int32_t> n(N + 1);
        if (fread(x0.data(), 8, N, f) != N || fread(c.data(), 8, N, f) != N || fread(thr.data(), 8, N, f) != N ||
            fread(n.data(), 4, N, f) != N)
            return 2;
        const int64_t bad = guards_check(kb[0], kb[1], x0.data(), c.data(), thr.data(), n.data(), cases, stats);
        if (bad != -1) {
            printf("block %lld (kind %d bias %d): case %lld fails, why %lld\n", (long long)b, kb[0], kb[1], (long long)bad,
                   (long long)stats[3]);
            return 1;
        }
        total += cases;
    }
    fclose(f);
    // ---- the lane functions ----
    const double ladder[6] = {0.3, 0.75, 1.2, 1.85, 2.85, 4.3};
    const double special[6] = {0.0, 0.0, 1e-6, 5e-324, 1e-310, 1e300};
    uint64_t lcg = 12345;
    auto rnd = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg >> 33); };
    int64_t calls = 0;
    for (int cfg = 0; cfg < 3; cfg++) {
        const int32_t V = 6, mt = 400000;
        const double interval = cfg == 0 ? 1.0 : cfg == 1 ? 0.05 : 0.3, max_buffer = cfg == 2 ? 6.0 : 20.0;
        void *h = cg_create(interval, 4.0, 1.0, V, max_buffer, 4.0, mt, ladder, 6);
        if (!cg_proven(h)) { printf("configuration %d fails the proof\n", cfg); return 1; }
        const int32_t n_lanes = 40, tlen = 97;
        std::vector<double> tr(tlen);
        for (auto &v : tr) v = (rnd() % 4 == 0) ? special[rnd() % 6] : 0.3 + (double)(rnd() % 6000) / 1000.0;
        tr[5] = 2.5;                                     // one live sample whatever the draw
        const int64_t toff[1] = {0};
        const int32_t tl[1] = {tlen};
        std::vector<int32_t> tid(n_lanes, 0), off(n_lanes), act((size_t)n_lanes * V);
        for (auto &v : off) v = (int32_t)(rnd() % tlen);
        for (auto &v : act) v = (int32_t)(rnd() % 6);
        std::vector<double> rec((size_t)n_lanes * V * 8), bw((size_t)n_lanes * V), fin((size_t)n_lanes * 6);
        std::vector<int32_t> fi((size_t)n_lanes * 2);
        int64_t st[4] = {0, 0, 0, 0};
        const int64_t rc = cg_batch(h, tr.data(), toff, tl, tid.data(), off.data(), act.data(), n_lanes, rec.data(), bw.data(),
                                    fin.data(), fi.data(), st);
        cg_destroy(h);
        if (rc != 0 || st[1] != 0 || st[0] == 0 || st[2] != st[3]) {
            printf("replay %d: rc %lld, proven calls %lld, outside the preconditions %lld, segments %lld / %lld\n", cfg,
                   (long long)rc, (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3]);
            return 1;
        }
        calls += st[0];
    }
    printf("ok %lld %lld\n", (long long)total, (long long)calls);
    return 0;
}
#endif
