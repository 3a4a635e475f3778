// CPU harness for forecast MPC (abr_lane_jump.h: plan_forecast, plan_usable, plan_cursor around look_subtree), built on the
// host by tests/test_plan_cpu.py.  It compiles the lookahead harness's source into this library as it stands -- its context,
// its roots, its walk and its brute-force loop (la_*) -- and adds the planner's two pieces: the walk with the root's cursor
// on a one-sample forecast, next to the brute force on an explicit constant trace, and the forecast on a column-major state.
#include "lookahead_harness.cpp"

extern "C" {

// n lanes as la_run: lane i plays its real trace from offset[i] through prefix[i], then plans on forecast[i].
// mode 0: the planner's walk (cursor = one sample at &forecast[i]; a forecast that is not usable answers -1 / NaN).
// mode 1: brute force over flat indices on an explicit trace of const_len samples, all forecast[i], entered at
// const_pos[i] (any position: the trace is constant).  Outputs as la_run.  Returns 0, or -1 on a bad horizon.
int pl_run(void *h, int32_t mode, int32_t horizon, const double *traces, const int64_t *trace_off, const int32_t *trace_len,
           const int32_t *trace_id, const int32_t *offset, const int32_t *prefix, int32_t n_prefix, int32_t n,
           const double *forecast, int32_t const_len, const int32_t *const_pos, int32_t *action, double *key, double *q,
           uint8_t *done) {
    const Ctx *c = (const Ctx *)h;
    if (horizon < 1 || horizon > 8) return -1;
    double qm[16];
    for (int32_t i = 0; i < n; i++) {
        const int32_t t = trace_id[i];
        Root r = make_root(c, traces + trace_off[t], trace_len[t], offset[i], prefix + (int64_t)i * n_prefix, n_prefix);
        done[i] = r.done ? 1 : 0;
        const bool usable = abrx::plan_usable(forecast[i]);
        std::vector<double> flat((size_t)const_len, forecast[i]);
        if (mode == 0) {
            abrx::plan_cursor(r.s.cur, forecast + i);
            if (!usable) r.done = true;                 // the kernel's `live = false`
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
            r.s.cur.trace = flat.data(); r.s.cur.tlen = const_len; r.s.cur.tpos = const_pos[i] % const_len;
            if (!usable) r.done = true;
            brute(c, r, horizon, &action[i], &key[i], qm, nullptr, nullptr, nullptr);
        }
        for (int32_t m = 0; m < c->M; m++) q[(int64_t)m * n + i] = qm[m];
    }
    return 0;
}

// The built-in forecast of n lanes as plan_forecast_kernel runs it: done [n], c [n], hist [T][n] (row j = previous_bandwidths
// [j]), state = the n-lane byte image in abr_mpc_robust's layout (NULL: robust == 0), P_out [n].
void pl_forecast(int64_t n, int32_t W, const uint8_t *done, const int32_t *c, const double *hist, uint8_t *state,
                 double *P_out) {
    for (int64_t i = 0; i < n; i++) {
        const auto hf = [&](int32_t j) { return hist[(int64_t)j * n + i]; };
        P_out[i] = abrx::plan_forecast(W, done[i] != 0, c[i], hf, state, n, i);
    }
}

int pl_usable(double P) { return abrx::plan_usable(P) ? 1 : 0; }

}
