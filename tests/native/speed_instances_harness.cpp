// CPU harness for the two builds of the lane functions (abr_lane_jump.h: TablesT<SPEEDS>): the same episode through
// TablesT<true> -- the table every other harness fills in, with no speed feature set -- and through TablesT<false>, whose
// lane functions hold no speed code at all.  Built by tests/test_speed_instances_cpu.py.
#include <stdint.h>
#include <stdlib.h>
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

struct Ctx {
    abrx::TickTables tt;
    double L, max_buffer, start_up_length;
    int32_t V, max_ticks;
    double ladder[16];
    int n_rates;
};

template <bool SPEEDS>
static abrx::TablesT<SPEEDS> tables_of(const Ctx &c) {
    abrx::TablesT<SPEEDS> t;
    t.G = c.tt.G.data(); t.interval_tick = c.tt.interval_tick.data(); t.avail_tick = c.tt.avail_tick.data();
    t.L = c.L; t.sd = c.tt.sd; t.max_buffer = c.max_buffer; t.start_up_length = c.start_up_length;
    t.V = c.V; t.max_ticks = c.max_ticks;
    if constexpr (SPEEDS) { t.per_lane_speed = false; t.speed_rows = 0; t.speed_stride = 0; t.speeds = nullptr; }
    t.drain = abrx::make_drain_tab(c.tt.sd, c.max_buffer + c.L);     // as abr_env_create does
    return t;
}

// One episode, the step in its two halves as the role-split kernels run it.  Per-step outputs are taken AT each call site:
// rec[s*8 + ..] = global_time, rebuffer_time, start_up_time, play_time, buffer_level, last_bw, sumk, flags(su|be<<1|bf<<2);
// pred[s] = the download side's prediction of the next call site (-1: none made); fin[0..5] = global_time, rebuffer_time,
// start_up_time, play_time, buffer_level, sumk; fin_i[0] = n_play.  Returns 0, or -2 on timeout, -5 on a wrong episode end.
template <bool SPEEDS>
static int episode(const Ctx &c, const double *trace, int32_t tlen, int32_t offset, const int32_t *actions, double *rec,
                   double *bw_out, int32_t *pred, double *fin, int32_t *fin_i) {
    const abrx::TablesT<SPEEDS> t = tables_of<SPEEDS>(c);
    static_assert(abrx::TablesT<SPEEDS>::kSpeeds == SPEEDS, "the tag the lane functions select on");
    abrx::LaneJ s;
    s.cur.trace = trace; s.cur.tlen = tlen;
    s.sd = t.sd; s.lane = 0;
    abrx::lanej_init(s, t, offset);
    if (!abrx::lanej_wait_call(s, t)) return -2;
    double last_bw = 0.0;
    for (int step = 0; step < t.V; step++) {
        double *r = rec + (size_t)step * 8;
        r[0] = t.G[s.k]; r[1] = t.G[s.n_rb]; r[2] = t.G[s.n_su]; r[3] = c.tt.GP[s.n_play];
        r[4] = s.buf; r[5] = last_bw; r[6] = (double)s.sumk;
        r[7] = (double)((s.su ? 1 : 0) | (s.be ? 2 : 0) | (s.bf ? 4 : 0));
        const int a = actions[step];
        const double buf0 = s.buf; const bool su0 = s.su, be0 = s.be; const int32_t k0 = s.k;
        const abrx::StepStart st = abrx::lanej_begin_step(s.cur, t, s.k, s.chunk_id);
        const abrx::Download dd = abrx::lanej_download(s.cur, t, st, s.k, c.ladder[a] * t.L);
        const abrx::StepResult sr = abrx::lanej_after_download(s, t, dd, st.avail_next, a);
        if (sr.timeout) return -2;
        int32_t kn = -1;
        if (!sr.ended && dd.hit && abrx::lanej_gate_possible(buf0, su0, be0, dd.n_dl, t))
            if (!abrx::lanej_predict_next_call(buf0, k0, dd.n_dl, st.avail_next, t, kn)) kn = -1;
        pred[step] = kn;
        last_bw = sr.bw;
        bw_out[step] = sr.bw;
        if (sr.ended != (step == t.V - 1)) return -5;
    }
    fin[0] = t.G[s.k]; fin[1] = t.G[s.n_rb]; fin[2] = t.G[s.n_su]; fin[3] = c.tt.GP[s.n_play];
    fin[4] = s.buf; fin[5] = (double)s.sumk;
    fin_i[0] = s.n_play; fin_i[1] = 0;
    return 0;
}

extern "C" {

void *si_create(double interval, double L, double speed, int32_t V, double max_buffer, double start_up_length,
                int32_t max_ticks, const double *ladder, int32_t n_rates) {
    Ctx *c = new Ctx;
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    c->tt = abrx::build_tick_tables(interval, L, speed, V, max_ticks, n_iv);
    c->L = L; c->max_buffer = max_buffer; c->start_up_length = start_up_length; c->V = V; c->max_ticks = max_ticks;
    c->n_rates = n_rates;
    for (int i = 0; i < n_rates; i++) c->ladder[i] = ladder[i];
    return c;
}
void si_destroy(void *h) { delete (Ctx *)h; }

// speeds_flag: 1 = the lane functions of TablesT<true> (no feature set), 0 = those of TablesT<false>
int64_t si_batch(void *h, int32_t speeds_flag, const double *traces, const int64_t *trace_off, const int32_t *trace_len,
                 const int32_t *trace_id, const int32_t *offset, const int32_t *actions, int32_t n_lanes, double *rec,
                 double *bw_out, int32_t *pred, double *fin, int32_t *fin_i) {
    const Ctx &c = *(const Ctx *)h;
    const int V = c.V;
    for (int32_t i = 0; i < n_lanes; i++) {
        const int tid = trace_id[i];
        const double *tr = traces + trace_off[tid];
        const int rc = speeds_flag
            ? episode<true>(c, tr, trace_len[tid], offset[i], actions + (size_t)i * V, rec + (size_t)i * V * 8,
                            bw_out + (size_t)i * V, pred + (size_t)i * V, fin + (size_t)i * 6, fin_i + (size_t)i * 2)
            : episode<false>(c, tr, trace_len[tid], offset[i], actions + (size_t)i * V, rec + (size_t)i * V * 8,
                             bw_out + (size_t)i * V, pred + (size_t)i * V, fin + (size_t)i * 6, fin_i + (size_t)i * 2);
        if (rc) return -(1000 + (int64_t)i * 10 - rc);
    }
    return 0;
}

// sizeof / the tag of the two tables, for the test to confirm it ran two different builds: [0] sizeof <true>, [1] sizeof <false>
void si_sizes(int32_t *out) {
    out[0] = (int32_t)sizeof(abrx::TablesT<true>); out[1] = (int32_t)sizeof(abrx::TablesT<false>);
    out[2] = abrx::TablesT<true>::kSpeeds ? 1 : 0; out[3] = abrx::TablesT<false>::kSpeeds ? 1 : 0;
}
}
