// CPU harness for the closed-loop speed rule (abr_lane_jump.h: speed_rule_eval, sched_begin_chunk with a rule): replays
// episodes through the event-driven lane step ON THE HOST -- the same source the kernels compile for gfx950 -- so that
// tests/test_speed_rule_cpu.py can compare it bit for bit with the tick-loop twin (tests/speed_twin.py) without a GPU.
#include <stdint.h>
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

extern "C" {

// the rule alone: out[c] = speed for (lat[c], buf[c])
void sr_eval(const abrx::SpeedRule *r, const double *lat, const double *buf, int64_t n, double *out) {
    for (int64_t c = 0; c < n; c++) out[c] = abrx::speed_rule_eval(*r, lat[c], buf[c]);
}

// n_lanes episodes under one rule.  Per call site s of lane i (before action s is applied):
// rec[(i*V + s)*7 + ..] = global_time, rebuffer_time, start_up_time, play_time, buffer_level, last_bw, play_id;
// bw_out[i*V + s] = the bandwidth of chunk s; fin[i*7 + ..] = the same seven at the end, with pt_sum in place of last_bw;
// fin_n[i*2 + ..] = n_play, sumk; log[i*log_rows + p] = the speed of played chunk p.  Returns 0, or -(1 + lane) on a
// timeout / an episode that ends early.
int64_t sr_batch(const abrx::SpeedRule *rule, double interval, double L, int32_t V, double max_buffer,
                 double start_up_length, int32_t max_ticks, const double *ladder,
                 const double *traces, const int64_t *trace_off, const int32_t *trace_len,
                 const int32_t *trace_id, const int32_t *offset, const int32_t *actions, int32_t n_lanes,
                 double *rec, double *bw_out, double *fin, int64_t *fin_n, double *log, int32_t log_rows) {
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    abrx::TickTables tt = abrx::build_tick_tables(interval, L, 1.0, V, max_ticks, n_iv);
    abrx::SpeedRuleBlock rb{};
    rb.rule = *rule; rb.log_rows = log_rows;
    abrx::Tables t;
    t.G = tt.G.data(); t.interval_tick = tt.interval_tick.data(); t.avail_tick = tt.avail_tick.data();
    t.L = L; t.sd = tt.sd; t.max_buffer = max_buffer; t.start_up_length = start_up_length;
    t.V = V; t.max_ticks = max_ticks;
    t.per_lane_speed = true;                      // as make_tables does under a rule: a schedule whose rows are computed
    t.speed_rows = abrx::kSpeedRowsRule; t.speed_stride = 1; t.speeds = nullptr; t.rule = &rb;
    t.drain.n = 0;
    for (int32_t i = 0; i < n_lanes; i++) {
        rb.log = log + (int64_t)i * log_rows;
        abrx::LaneJ s;
        s.cur.trace = traces + trace_off[trace_id[i]]; s.cur.tlen = trace_len[trace_id[i]];
        s.sd = t.sd; s.lane = 0;
        abrx::lanej_init(s, t, offset[i]);
        if (!abrx::lanej_wait_call(s, t)) return -(1 + (int64_t)i);
        double last_bw = 0.0;
        for (int32_t step = 0; step < V; step++) {
            double *r = rec + ((int64_t)i * V + step) * 7;
            r[0] = t.G[s.k]; r[1] = t.G[s.n_rb]; r[2] = t.G[s.n_su]; r[3] = s.pt; r[4] = s.buf; r[5] = last_bw;
            r[6] = (double)s.play_id;
            const int32_t a = actions[(int64_t)i * V + step];
            // the two halves, as the role-split kernels run them
            const abrx::StepStart st = abrx::lanej_begin_step(s.cur, t, s.k, s.chunk_id);
            const abrx::Download d = abrx::lanej_download(s.cur, t, st, s.k, ladder[a] * t.L);
            const abrx::StepResult sr = abrx::lanej_after_download(s, t, d, st.avail_next, a);
            if (sr.timeout || sr.ended != (step == V - 1)) return -(1 + (int64_t)i);
            last_bw = sr.bw;
            bw_out[(int64_t)i * V + step] = sr.bw;
        }
        double *f = fin + (int64_t)i * 7;
        f[0] = t.G[s.k]; f[1] = t.G[s.n_rb]; f[2] = t.G[s.n_su]; f[3] = s.pt; f[4] = s.buf; f[5] = s.pt_sum;
        f[6] = (double)s.play_id;
        fin_n[(int64_t)i * 2] = s.n_play; fin_n[(int64_t)i * 2 + 1] = s.sumk;
    }
    return 0;
}

}
