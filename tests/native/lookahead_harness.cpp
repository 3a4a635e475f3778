// CPU harness for the lookahead expert (abr_lane_jump.h: look_subtree, look_pick, the launch-splitting arithmetic): the walk
// the lookahead kernel compiles for gfx950, built on the host by tests/test_lookahead_cpu.py, next to a brute-force loop that
// shares nothing with it but lanej_step: for every flat index it copies the root, steps h times and forms the key.
#include <stdint.h>
#include <math.h>
#include <vector>
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

using TB = abrx::TablesT<false>;

struct Ctx {
    abrx::TickTables tt;
    TB t;
    double ladder[16];
    double wr, wv, ws, wl;
    int32_t M;
    abrx::EpisodeQuality ql;       // base != nullptr: a quality model is installed (the harness never writes through it)
};

// a lane at a call site, as the workspace would hold it
struct Root {
    abrx::LaneJ s;
    int32_t n_rb_obs, n_su_obs;
    bool done;
};

static double avg_latency(const Ctx *c, const abrx::LaneJ &s) {     // abr_env.hip: lane_avg_latency
    if (s.n_play == 0) return 0.0;
    const double tri = (double)(((long long)s.n_play * (s.n_play - 1)) / 2);
    return (0.01 * (double)s.sumk - c->t.sd * tri) / c->tt.GP[s.n_play];
}

// reset, then n_prefix scripted decisions: what abr_env_reset and abr_env_step leave behind
static Root make_root(const Ctx *c, const double *trace, int32_t tlen, int32_t offset, const int32_t *prefix,
                      int32_t n_prefix) {
    Root r{};
    r.s.cur.trace = trace; r.s.cur.tlen = tlen; r.s.sd = c->t.sd;
    abrx::lanej_init(r.s, c->t, offset);
    r.done = !abrx::lanej_wait_call(r.s, c->t);
    for (int32_t j = 0; j < n_prefix && !r.done; j++) {
        const abrx::StepResult sr = abrx::lanej_step(r.s, c->t, c->ladder[prefix[j]] * c->t.L, prefix[j]);
        r.n_rb_obs = r.s.n_rb; r.n_su_obs = r.s.n_su;
        r.done = sr.ended || sr.timeout;
    }
    return r;
}

template <int H>
static void walk(const Ctx *c, const Root &r, int32_t *action, double *key, double *q) {
    abrx::LookWeights w;
    w.wr = c->wr; w.ws = c->ws; w.wv = c->wv; w.wl = c->wl; w.M = c->M; w.quality = c->ql.base != nullptr;
    const auto br = [&](int32_t, int32_t rate) { return c->ladder[rate]; };
    const auto G = [&](int32_t n) { return c->t.G[n]; };
    const auto lat = [&](const abrx::LaneJ &x) { return avg_latency(c, x); };
    const auto qt = [&](int32_t chunk, int32_t rate) { return abrx::quality_peek(c->ql, c->M, chunk, rate); };
    const auto any = [](bool f) { return f; };
    for (int32_t m = 0; m < c->M; m++)
        q[m] = abrx::look_subtree<H>(w, c->t, br, G, lat, qt, any, r.s, !r.done, r.n_rb_obs, r.n_su_obs, m);
    abrx::look_pick([&](int32_t m) { return q[m]; }, c->M, *action, *key);
}

// Every sequence by its flat index, a_0 the most significant digit.  leaf_R / leaf_lat / leaf_ok (nullable, [M^h]): each
// sequence's reward sum, final latency and validity, for the comparison with the oracle.  Returns h.
static int32_t brute(const Ctx *c, const Root &r, int32_t horizon, int32_t *action, double *key, double *q, double *leaf_R,
                     double *leaf_lat, uint8_t *leaf_ok) {
    const int32_t M = c->M;
    for (int32_t m = 0; m < M; m++) q[m] = NAN;
    *action = -1; *key = NAN;
    if (r.done) return 0;
    const int32_t left = c->t.V - r.s.chunk_id, h = horizon < left ? horizon : left;
    int64_t leaves = 1;
    for (int32_t j = 0; j < h; j++) leaves *= M;
    std::vector<uint8_t> have(M, 0);
    for (int64_t f = 0; f < leaves; f++) {
        abrx::LaneJ s = r.s;
        int32_t n_rb_obs = r.n_rb_obs, n_su_obs = r.n_su_obs;
        double R = 0.0;
        bool ok = true;
        int64_t div = leaves;
        int32_t a0 = 0;
        for (int32_t j = 0; j < h; j++) {
            div /= M;
            const int32_t a = (int32_t)((f / div) % M);
            if (j == 0) a0 = a;
            const int32_t prev = s.last_action, chunk = s.chunk_id;
            const abrx::StepResult sr = abrx::lanej_step(s, c->t, c->ladder[a] * c->t.L, a);
            if (sr.timeout) { ok = false; break; }
            double var = 0.0;
            if (prev >= 0) var = fabs(c->ladder[a] - c->ladder[prev]);
            double rew = c->wr * (c->t.G[s.n_rb] - c->t.G[n_rb_obs]) + c->ws * (c->t.G[s.n_su] - c->t.G[n_su_obs]) + c->wv * var;
            if (c->ql.base) rew = rew - c->ql.wq * c->ql.u[(int64_t)chunk * M + a];
            R = R + (double)(float)rew;
            n_rb_obs = s.n_rb; n_su_obs = s.n_su;
        }
        const double lt = ok ? avg_latency(c, s) : NAN;
        const double k = R + c->wl * lt;
        if (leaf_R) { leaf_R[f] = R; leaf_lat[f] = lt; leaf_ok[f] = ok ? 1 : 0; }
        if (!ok || k != k) continue;
        if (!have[a0] || k < q[a0]) { q[a0] = k; have[a0] = 1; }
    }
    for (int32_t m = 0; m < M; m++)
        if (have[m] && (*action < 0 || q[m] < *key)) { *action = m; *key = q[m]; }
    return h;
}

extern "C" {

int la_node_size(void) { return (int)sizeof(abrx::LookNode); }
int64_t la_leaves(int32_t M, int32_t h) { return abrx::look_leaves(M, h); }
int64_t la_nodes(int32_t M, int32_t h) { return abrx::look_nodes(M, h); }
int64_t la_lanes_per_launch(int64_t max_nodes, int32_t M, int32_t h) { return abrx::look_lanes_per_launch(max_nodes, M, h); }
int64_t la_default_nodes(void) { return abrx::kLookDefaultNodes; }
int64_t la_max_leaves(void) { return abrx::kLookMaxLeaves; }

// weights: wr, wv, ws, wl (QOEMetric's order)
void *la_create(double interval, double L, double speed, int32_t V, double max_buffer, double start_up_length,
                int32_t max_ticks, const double *ladder, int32_t n_rates, const double *weights) {
    Ctx *c = new Ctx;
    const int32_t n_iv = (int32_t)((double)max_ticks * 0.01 / interval + 4.0);
    c->tt = abrx::build_tick_tables(interval, L, speed, V, max_ticks, n_iv);
    c->t.G = c->tt.G.data();
    c->t.interval_tick = c->tt.interval_tick.data();
    c->t.avail_tick = c->tt.avail_tick.data();
    c->t.L = L; c->t.sd = c->tt.sd; c->t.max_buffer = max_buffer; c->t.start_up_length = start_up_length;
    c->t.V = V; c->t.max_ticks = max_ticks;
    c->t.drain = abrx::make_drain_tab(c->tt.sd, max_buffer + L);     // as abr_env_create does
    c->M = n_rates;
    for (int i = 0; i < n_rates; i++) c->ladder[i] = ladder[i];
    c->wr = weights[0]; c->wv = weights[1]; c->ws = weights[2]; c->wl = weights[3];
    c->ql = abrx::EpisodeQuality{};
    return c;
}
void la_destroy(void *h) { delete (Ctx *)h; }

// u: [V][n_rates], kept by the caller; NULL: no model
void la_set_quality(void *h, double wq, const double *u) {
    Ctx *c = (Ctx *)h;
    c->ql = abrx::EpisodeQuality{};
    if (u) { c->ql.wq = wq; c->ql.u = u; c->ql.base = (void *)u; c->ql.rows = 1; }
}

// n lanes: lane i plays trace trace_id[i] from offset[i], takes prefix[i][0 .. n_prefix) and is then asked.  mode 0: the
// walk; 1: brute force.  Outputs action [n], key [n], q [M][n], done [n] (the root was finished or timed out); leaf_* (mode
// 1 only, nullable): [n][M^horizon], a lane's first M^h entries used.  Returns 0, or -1 on a bad horizon.
int la_run(void *h, int32_t mode, int32_t horizon, const double *traces, const int64_t *trace_off, const int32_t *trace_len,
           const int32_t *trace_id, const int32_t *offset, const int32_t *prefix, int32_t n_prefix, int32_t n,
           int32_t *action, double *key, double *q, uint8_t *done, double *leaf_R, double *leaf_lat, uint8_t *leaf_ok) {
    const Ctx *c = (const Ctx *)h;
    if (horizon < 1 || horizon > 8) return -1;
    const int64_t stride = abrx::look_leaves(c->M, horizon);
    double qm[16];
    for (int32_t i = 0; i < n; i++) {
        const int32_t t = trace_id[i];
        const Root r = make_root(c, traces + trace_off[t], trace_len[t], offset[i], prefix + (int64_t)i * n_prefix, n_prefix);
        done[i] = r.done ? 1 : 0;
        if (mode == 0) {
            switch (horizon) {
            case 1: walk<1>(c, r, &action[i], &key[i], qm); break;
            case 2: walk<2>(c, r, &action[i], &key[i], qm); break;
            case 3: walk<3>(c, r, &action[i], &key[i], qm); break;
            case 4: walk<4>(c, r, &action[i], &key[i], qm); break;
            case 5: walk<5>(c, r, &action[i], &key[i], qm); break;
            case 6: walk<6>(c, r, &action[i], &key[i], qm); break;
            case 7: walk<7>(c, r, &action[i], &key[i], qm); break;
            default: walk<8>(c, r, &action[i], &key[i], qm); break;
            }
        } else {
            brute(c, r, horizon, &action[i], &key[i], qm, leaf_R ? leaf_R + i * stride : nullptr,
                  leaf_lat ? leaf_lat + i * stride : nullptr, leaf_ok ? leaf_ok + i * stride : nullptr);
        }
        for (int32_t m = 0; m < c->M; m++) q[(int64_t)m * n + i] = qm[m];
    }
    return 0;
}

}
