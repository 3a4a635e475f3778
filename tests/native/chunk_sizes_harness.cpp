// CPU harness for the environment's size table (include/abr_env.h: abr_env_set_size_table): the three places of
// abr_lane_jump.h that read it -- look_subtree's size accessor, the learned policy's feature builder, the rules' effective
// bitrates -- the same source the kernels compile for gfx950, built on the host by tests/test_chunk_sizes_cpu.py and
// compared there with the oracle and numpy.
#include <stdint.h>
#include <math.h>
#include <vector>
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

using TB = abrx::TablesT<false>;

extern "C" {

// The walk of n lanes at their first call site (lane i: trace trace_id[i] from offset[i]) with bitrates br [V][M] (what is
// scored) and sizes sz [V][M] (what is downloaded; NULL: the form without a size accessor).  weights: wr, wv, ws, wl.
// q [M][n].  Returns 0, or -1 on a horizon other than 2 or 3.
int cs_walk(int32_t horizon, double interval, double L, int32_t V, double max_buffer, double start_up_length,
            int32_t max_ticks, const double *br, const double *sz, int32_t M, const double *weights, const double *traces,
            const int64_t *trace_off, const int32_t *trace_len, const int32_t *trace_id, const int32_t *offset, int32_t n,
            double *q) {
    if (horizon != 2 && horizon != 3) return -1;
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    const abrx::TickTables tt = abrx::build_tick_tables(interval, L, 1.0, V, max_ticks, n_iv);
    TB t;
    t.G = tt.G.data(); t.interval_tick = tt.interval_tick.data(); t.avail_tick = tt.avail_tick.data();
    t.L = L; t.sd = tt.sd; t.max_buffer = max_buffer; t.start_up_length = start_up_length; t.V = V; t.max_ticks = max_ticks;
    t.drain = abrx::make_drain_tab(tt.sd, max_buffer + L);
    abrx::LookWeights w;
    w.wr = weights[0]; w.wv = weights[1]; w.ws = weights[2]; w.wl = weights[3]; w.M = M; w.quality = false;
    const auto brf = [&](int32_t chunk, int32_t rate) { return br[(int64_t)chunk * M + rate]; };
    const auto szf = [&](int32_t chunk, int32_t a, double) { return sz[(int64_t)chunk * M + a]; };
    const auto G = [&](int32_t k) { return t.G[k]; };
    const auto lat = [&](const abrx::LaneJ &s) {     // abr_env.hip: lane_avg_latency
        if (s.n_play == 0) return 0.0;
        const double tri = (double)(((long long)s.n_play * (s.n_play - 1)) / 2);
        return (0.01 * (double)s.sumk - t.sd * tri) / tt.GP[s.n_play];
    };
    const auto qt = [](int32_t, int32_t) { return 0.0; };
    const auto any = [](bool f) { return f; };
    for (int32_t i = 0; i < n; i++) {
        abrx::LaneJ s{};
        const int32_t tr = trace_id[i];
        s.cur.trace = traces + trace_off[tr]; s.cur.tlen = trace_len[tr]; s.sd = t.sd;
        abrx::lanej_init(s, t, offset[i]);
        const bool live = abrx::lanej_wait_call(s, t);
        for (int32_t m = 0; m < M; m++) {
            double v;
            if (!sz) v = horizon == 2 ? abrx::look_subtree<2>(w, t, brf, G, lat, qt, any, s, live, 0, 0, m)
                                      : abrx::look_subtree<3>(w, t, brf, G, lat, qt, any, s, live, 0, 0, m);
            else v = horizon == 2 ? abrx::look_subtree<2>(w, t, brf, szf, G, lat, qt, any, s, live, 0, 0, m)
                                  : abrx::look_subtree<3>(w, t, brf, szf, G, lat, qt, any, s, live, 0, 0, m);
            q[(int64_t)m * n + i] = v;
        }
    }
    return 0;
}

// policy_features of n call sites with the next chunk's row read from nx [V][M] (NULL: the form without it, from br).
// x_out [n][F], F = 4 + W + M.
void cs_features(int64_t n, int32_t W, int32_t M, int32_t V, const double *norm, const int32_t *c, const int32_t *a,
                 const double *B, const double *G, const double *P, const double *h, int32_t hmax, const double *br,
                 const double *nx, float *x_out) {
    abrx::PolicyNet nt{};
    nt.window = W; nt.M = M; nt.F = 4 + W + M; nt.norm = norm;
    for (int64_t i = 0; i < n; i++) {
        const double *hi = h + i * hmax;
        const auto hf = [&](int32_t j) { return hi[j]; };
        const auto brf = [&](int32_t r, int32_t m) { return br[(int64_t)r * M + m]; };
        const auto nxf = [&](int32_t r, int32_t m) { return nx[(int64_t)r * M + m]; };
        float x[abrx::kPolicyMaxF];
        if (nx) abrx::policy_features(nt, hf, brf, nxf, V, c[i], a[i], B[i], G[i], P[i], x);
        else abrx::policy_features(nt, hf, brf, V, c[i], a[i], B[i], G[i], P[i], x);
        for (int32_t f = 0; f < nt.F; f++) x_out[i * nt.F + f] = x[f];
    }
}

// rule_select_at of n call sites as rule_action forms it under a size table: kind[i] with its parameters, chunk c[i],
// buffer B[i], bitrates br [V][M], sizes sz [V][M], chunk length L, history h[i][0..c), utilities u [V][M].
void cs_rule(int64_t n, const int32_t *kind, int32_t window, double reservoir, double cushion, double safety, double bola_v,
             double bola_gp, const int32_t *c, const double *B, int32_t M, int32_t V, const double *br, const double *sz,
             double L, const double *h, int32_t hmax, const double *u, int32_t *out) {
    for (int64_t i = 0; i < n; i++) {
        abrx::RuleParams r{};
        r.kind = kind[i]; r.window = window; r.reservoir = reservoir; r.cushion = cushion; r.safety = safety;
        r.bola_v = bola_v; r.bola_gp = bola_gp; r.utility = u;
        const double *hi = h + i * hmax;
        const bool cost = abrx::rule_reads_cost(r.kind);
        const auto brf = [&](int32_t m) {
            return cost ? abrx::rule_cost(sz + (int64_t)c[i] * M, L, m) : br[(int64_t)c[i] * M + m];
        };
        const auto hf = [&](int32_t j) { return hi[j]; };
        out[i] = abrx::rule_select_at(r, brf, hf, M, V, c[i], -1, B[i]);
    }
}

}
