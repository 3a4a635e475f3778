// abr_env.hip -- HIP kernels (gfx950 / CDNA4) and the C ABI of include/abr_env.h.
//
// Hot path restated from the reference (file:line into Elliotshui/ABRSimulator):
//   K1/K2 env_jump_kernel<MODE>     Simulator.py:95-133,135-208   event-driven, one thread per lane: the
//         tick loop's float64 sequences advanced in exact closed form (abr_lane_jump.h,
//         abr_exact_jump.h); MODE 0 reset, 1 step, 2 fused random-policy rollout, 3 fused scripted rollout,
//         4 fused rollout under a bitrate rule (BUFFER / RATE / BOLA: abr_lane_jump.h rule_select; rule_select_kernel
//         is the same decision without a step)
//   K1    env_split3_kernel<MODE>   the same lane functions on three waves per 64 lanes (download / player /
//         service; abr_env_roles.h): what impl 3 (auto) runs up to kSplit3MaxLanes (65 536) lanes -- for launches of more
//         than one decision; a single decision per launch goes to env_jump_kernel at every size
//   K1    env_split_kernel<MODE>    ... on two waves per 64 lanes (download / player): up to kSplitMaxLanes (131 072) lanes
//   K1/K2 env_advance_kernel<MODE>  the same, one loop trip per 0.01 s tick (cross-check)
//   K3    mpc_select_kernel<H, B, WVM>   mpc.py:81-93,104-186   harmonic predictor (mpc_predict_kernel ahead of it when the
//         caller provides scratch) + exhaustive B^H: B^2 threads per lane; tables in LDS, depth-first enumeration with
//         prefix sharing, LDS arg-max over the threads, first-leaf search below the winning node
//   K3r   mpc_robust_predict_kernel      RobustMPC's estimate (abr_lane_jump.h: robust_estimate) ahead of the same search
//   K3f   fastmpc_grid_kernel / _pack    FastMPC's table: every grid point through the same search, first actions as uint8;
//         the lookup itself is MODE 4 (abr_lane_jump.h: fastmpc_lookup) and fastmpc_select_kernel
//   K4    episode_qoe_kernel        Simulator.py:79-86
//
// Exactness contract: every quantity that feeds a decision in the
// reference (downloaded_size >= target, buffer_level vs 0 / max_buffer / start_up_length,
// int(global_time / x), play_length >= L) is reproduced bit-for-bit: the lane-specific
// ones (downloaded_size, buffer_level) as the float64 value the serial additions produce,
// the lane-independent ones (global_time and everything that is "k additions of dt
// starting from 0") through tick tables computed once on the host in float64
// (abr_tick_tables.h).  Compile with -ffp-contract=off: an FMA would round
// bandwidth*dt + downloaded_size once instead of twice (Simulator.py:160).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "abr_env.h"

// Cycle stamps and per-workgroup timing exist only in the diagnostic build (tools/diag/csrc: -DABR_SPLIT_STAMPS); the
// product compiles them to nothing.
#ifdef ABR_SPLIT_STAMPS
#include "abr_diag_stamps.h"
#else
#define ABR_STAMP(n)
#define ABR_STAMP_INIT()
#define ABR_STAMP_FLUSH()
#define ABR_WG_TIME(slot)
#define ABR_WG_WHERE(role)
#define K3_STAMP_DECL
#define K3_STAMP(n)
#define K3_STAMP_FLUSH()
#endif
// where EnvParams::speed_rule lies in the kernarg segment of every kernel that takes `EnvParams p` as its FIRST argument
// (asserted below): abr_lane_jump.h reads a speed rule there when a played chunk begins
#define ABR_RULE_KERNARG_OFFSET 592
#include "abr_lane_jump.h"
#include "abr_tick_tables.h"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess)                                                            \
            return fail(ABR_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e__));       \
    } while (0)

extern "C" int abr_abi_version(void) { return ABR_ABI_VERSION; }
extern "C" const char *abr_last_error(void) { return g_err; }

// ---------------------------------------------------------------------------
// device-side parameter block (passed by value to every env kernel)
// ---------------------------------------------------------------------------
constexpr double kDt = 0.01;  // Simulator.py:133
constexpr int kFlagStartUp = 1, kFlagBufEmpty = 2, kFlagBufFull = 4;
constexpr int kFlagArmed = 8;    // the lane has been reset at least once since abr_env_create

struct EnvParams {
    // config
    int32_t n_rates, video_length, max_ticks, auto_reset;
    int32_t play_ticks_per_chunk;  // P: first n with n-fold sum of speed*dt >= chunk_length (:185)
    int32_t n_intervals;           // entries in interval_tick minus sentinel
    int32_t t_block;               // ticks per block of the tick loop (<= shortest interval)
    int32_t n_traces;              // rows of trace_off / trace_len (range check of reset's trace ids)
    double chunk_length, max_buffer, start_up_length;
    double wr, wv, ws, wl;
    double sd;                     // speed * dt, the product the reference forms each tick (:182)
    double ladder[ABR_MAX_RATES];
    int64_t n_lanes, lane_id_base;
    // tables (device)
    const double *G;               // G[n] = dt added n times to 0.0
    const double *GP;              // same for sd (aliases G when speed == 1)
    const int32_t *interval_tick;  // first tick k with int(G[k]/interval) >= j   (:158)
    const int32_t *avail_tick;     // first tick k with int(G[k]/L) - 1 >= c      (:143)
    abrx::DrainTab drain;          // the per-binade cascade of buffer_level -= sd (abr_exact_jump.h); n == 0: none
    // traces (device, caller-owned)
    const double *traces;
    const int64_t *trace_off;
    const int32_t *trace_len;
    // per-lane state, SoA (device, in the workspace)
    double *buf, *last_bw, *hist_n, *hist_s;
    double *sd_lane, *pt_lane;     // per-lane speed*dt and play_time (only touched when lane_speeds != nullptr)
    const double *lane_speeds;     // caller-owned per-lane play speeds [speed_rows][n_lanes], or nullptr: one speed for all lanes
    int32_t speed_rows;            // 1: one constant speed per lane; >= 2: a schedule, one row per played chunk
    int32_t avail_j_blocks;        // avail_j -- the trace interval avail_tick[c] lies in (abr_tick_tables.h) -- starts this many
                                   // 256-byte blocks after avail_tick (in the four bytes that were padding: no offset moves)
    int32_t *pl_left, *play_id;    // speed schedule only: playing ticks left in the played chunk, chunks played
    double *pt_sum;                // speed schedule only: sum of play_time over the playing ticks
    const double *br_table;        // caller-owned [video_length][n_rates] per-chunk ladders, or nullptr: `ladder`
    long long *sumk;               // sum of tick indices of playing ticks (latency integral)
    int32_t *k, *chunk_id, *n_su, *n_rb, *n_play, *j, *tpos, *trace_id, *offset0;
    int32_t *last_action, *n_su_obs, *n_rb_obs, *episode_no;
    uint8_t *flags, *done;
    uint8_t *action_hist;          // [V][n_lanes]
    double *bw_hist;               // [V][n_lanes]
    double *ep_qoe_terms;          // [4][n_lanes]: rebuffer, startup, avg latency, bitrate variance of the last finished episode
    double *var_run;               // [n_lanes] sum of |br[a_i] - br[a_(i+1)]| over the running episode so far (:82), in its order
    // abr_debug_selfcheck only (nullptr otherwise): instance <9> of a role-split kernel writes 1 here if fresh_params() -- the
    // parameter block re-read from the kernarg segment -- is THIS launch's block (it carries `sentinel`), 2 if not
    uint32_t *selfcheck_out;
    uint64_t sentinel;
    // abr_env_set_speed_rule (appended: everything above keeps its offset; the block grew from 592 to 880 bytes).  A rule
    // runs as a speed schedule whose rows are computed: speed_rows == abrx::kSpeedRowsRule, and lane_speeds then points at
    // sd_lane -- non-null, so that every "per-lane speeds" test holds, and never read as speeds.  The kernels read this
    // block from the kernarg segment only when a played chunk begins (abr_lane_jump.h: sched_begin_chunk).
    abrx::SpeedRuleBlock speed_rule;
    // abr_env_set_size_table (appended likewise: 880 -> 888 bytes): caller-owned [video_length][n_rates] sizes of what is
    // DOWNLOADED, or nullptr: bitrate x chunk_length.  Read by chunk_target, chunk_next_size, rule_action and the walks' sz.
    const double *sz_table;
};
static_assert(offsetof(EnvParams, speed_rule) == ABR_RULE_KERNARG_OFFSET, "abr_lane_jump.h reads the rule at this offset");
static_assert(sizeof(EnvParams) == 888, "the parameter block: 592 bytes + 288 of the speed rule + the size table");
static_assert(sizeof(abrx::SpeedRule) == sizeof(abr_speed_rule) &&
              offsetof(abrx::SpeedRule, lat_thr) == offsetof(abr_speed_rule, lat_thr) &&
              offsetof(abrx::SpeedRule, buf_thr) == offsetof(abr_speed_rule, buf_thr) &&
              offsetof(abrx::SpeedRule, speed) == offsetof(abr_speed_rule, speed), "abr_speed_rule: one layout");

// What a workspace says about itself, in its last 256 bytes: written by abr_env_create, compared by abr_env_notify_restore
// (and by the Python wrapper's load_state_dict before it copies anything).  A checkpoint is a copy of the workspace, and the
// layout of the regions in front of this tag changes between ABI versions (3: ep_actions gone, var_run added; 4: this tag):
// restoring a workspace of another version, lane count or configuration would otherwise be reinterpreted with shifted
// offsets and no error -- sizes can coincide.  kLayoutRev counts layout changes inside one ABI version.
constexpr uint32_t kTagMagic = 0x57524241u;          // "ABRW"
constexpr uint32_t kLayoutRev = 2;                  // 2: the avail_j table, a region of its own in front of the tag
struct WorkspaceTag {
    uint32_t magic, abi_version, layout_rev, n_rates;
    int64_t n_lanes;
    int32_t video_length, max_ticks, n_intervals, reserved_;
    uint64_t total_bytes;
    double chunk_length, interval, speed;            // the tick tables in front depend on these
    uint8_t pad_[256 - 72];
};
static_assert(sizeof(WorkspaceTag) == 256, "the tag is one 256-byte block");
static_assert(sizeof(abrx::EpisodeSampler) == sizeof(abr_episode_sampler) &&
              offsetof(abrx::EpisodeSampler, pool) == offsetof(abr_episode_sampler, pool) &&
              offsetof(abrx::EpisodeSampler, n_pool) == offsetof(abr_episode_sampler, n_pool) &&
              offsetof(abrx::EpisodeSampler, offset_span) == offsetof(abr_episode_sampler, offset_span),
              "abr_episode_sampler: one layout");
static_assert(sizeof(abrx::EpisodeLedger) == sizeof(abr_episode_ledger) &&
              offsetof(abrx::EpisodeLedger, base) == offsetof(abr_episode_ledger, base_dev) &&
              offsetof(abrx::EpisodeLedger, rows) == offsetof(abr_episode_ledger, rows),
              "abr_episode_ledger: one layout");
static_assert(sizeof(abrx::EpisodeQuality) == sizeof(abr_episode_quality) &&
              offsetof(abrx::EpisodeQuality, wq) == offsetof(abr_episode_quality, wq) &&
              offsetof(abrx::EpisodeQuality, u) == offsetof(abr_episode_quality, u_dev) &&
              offsetof(abrx::EpisodeQuality, base) == offsetof(abr_episode_quality, base_dev) &&
              offsetof(abrx::EpisodeQuality, rows) == offsetof(abr_episode_quality, rows),
              "abr_episode_quality: one layout");

struct abr_env {
    EnvParams p;
    abr_env_config cfg;
    size_t workspace_bytes;
    void *tag_dev;                  // the workspace's layout tag (device) and what it must hold
    WorkspaceTag tag;
    int impl;   // 3 = auto (default): see effective_impl(); 5 / 2 = role-split event-driven kernels, three / two waves
                // per 64 lanes; 0 = event-driven, one thread per lane; 1 = tick-by-tick kernels (cross-check);
                // 4 = asynchronous role pipeline (diagnostic build only)
    int32_t *mpc_action;            // [n_lanes] scratch of abr_env_step_mpc (in the workspace)
    void *mpc_scratch;              // predictor scratch of abr_env_step_mpc (in the workspace)
    const double *pending_speeds;   // abr_env_set_lane_speeds / _speed_schedule: latched by the next full reset
    int32_t pending_speed_rows;
    bool pending_rule_on;           // abr_env_set_speed_rule: latched the same way (speeds_dirty)
    abrx::SpeedRuleBlock pending_rule;
    bool speeds_dirty;
    const double *pending_br_table; // abr_env_set_bitrate_table: latched the same way
    bool br_table_dirty;
    const double *pending_sz_table; // abr_env_set_size_table: likewise
    bool sz_table_dirty;
    bool armed;                     // abr_env_reset has run at least once: episodes may be in flight
    bool sampler_on;                // abr_env_set_episode_sampler: launches run the SAMPLE instances with `sampler`
    abrx::EpisodeSampler sampler;
    abrx::EpisodeLedger ledger;     // abr_env_set_episode_ledger: base == nullptr while none is installed
    abrx::EpisodeQuality quality;   // abr_env_set_episode_quality: likewise
    bool chains_proven;             // abr_env_create: abrx::chains_proven() holds for this handle's tables and config, so its
                                    // launches may run the no-speeds instances, whose chains carry no per-segment guards
};

// A handle on which no reset has run has no episode to protect: the setters take effect at once
// (a freshly built handle that receives a checkpointed workspace must already carry them).
static void apply_pending(abr_env *env) {
    if (env->br_table_dirty) { env->p.br_table = env->pending_br_table; env->br_table_dirty = false; }
    if (env->sz_table_dirty) { env->p.sz_table = env->pending_sz_table; env->sz_table_dirty = false; }
    if (env->speeds_dirty) {
        env->p.lane_speeds = env->pending_speeds; env->p.speed_rows = env->pending_speed_rows;
        env->p.speed_rule = env->pending_rule;
        if (env->pending_rule_on) { env->p.lane_speeds = env->p.sd_lane; env->p.speed_rows = abrx::kSpeedRowsRule; }
        env->speeds_dirty = false;
    }
}

// mpd.chunks[chunk].bitrates[rate]: the single ladder run() indexes (Simulator.py:82,156), or --
// the evident intent of set_mpd's one-ladder-per-line file (Simulator.py:71-76) -- chunk's own
__device__ inline double chunk_bitrate(const EnvParams &p, int32_t chunk, int32_t rate) {
    return p.br_table ? p.br_table[(int64_t)chunk * p.n_rates + rate] : p.ladder[rate];
}

// target_size of chunk's download at `rate` (Simulator.py:156: bitrate x chunk_length), or -- while a size table is in
// force (include/abr_env.h: abr_env_set_size_table) -- the table's entry.  SIZED == false is the form of the no-speeds
// instances, which a handle with a size table never launches (launch_env): they hold no test of the pointer.
template <bool SIZED>
__device__ __forceinline__ double chunk_target(const EnvParams &p, int32_t chunk, int32_t rate) {
    if constexpr (SIZED) {
        if (p.sz_table) return p.sz_table[(int64_t)chunk * p.n_rates + rate];
    }
    return chunk_bitrate(p, chunk, rate) * p.chunk_length;
}
// what the learned policy's features 4 + W + m hold: chunk's bitrates, or under a size table its sizes (next_chunk_sizes)
__device__ __forceinline__ double chunk_next_size(const EnvParams &p, int32_t chunk, int32_t rate) {
    return p.sz_table ? p.sz_table[(int64_t)chunk * p.n_rates + rate] : chunk_bitrate(p, chunk, rate);
}

// ---------------------------------------------------------------------------
// philox4x32-10 (Salmon et al. 2011) -- counter-based, so shards reproduce the
// unsharded run: ctr = (global lane id lo, hi, episode step, episode number)
// ---------------------------------------------------------------------------
__host__ __device__ inline uint32_t philox_action(uint64_t seed, uint64_t lane, uint32_t step,
                                                  uint32_t episode, uint32_t n_rates) {
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
    return (uint32_t)(((uint64_t)c0 * n_rates) >> 32);   // multiply-shift into [0, n_rates)
}

// ---------------------------------------------------------------------------
// K1/K2: the tick loop
// ---------------------------------------------------------------------------
// "Call site" = the instant inside tick k at which the reference calls
// abr_controller.get_next_bitrate (Simulator.py:155): T1-T3 of tick k are done,
// the download is not paused and download_time == 0.  A step runs from one call
// site to the next and has two phases:
//   A  downloading: every tick adds bandwidth*dt until downloaded_size >= target.
//      The download cannot pause inside phase A: buffer_full only turns on in a
//      tick that completes a chunk (buffer_level grows nowhere else, :170), and
//      availability is monotone in time.
//   B  waiting for the next call site: chunk available (:143) and not buffer_full.
//
// Kernel structure (one lane per thread, one wave per workgroup):
//   block loop   every T ticks (T <= the shortest trace interval, so a lane
//                crosses at most one interval boundary per block):
//                - SERVICE lanes that reached a step boundary in the last block:
//                  finish the chunk record (one float64 division), emit
//                  reward/obs/done, take the next action (fused mode) or retire;
//                - PREFETCH bandwidth*dt of the current and next interval and the
//                  boundary tick, so that
//   tick loop    is straight-line predicated VALU code with no memory access and
//                no divergent branch: ~40 vector instructions per tick per wave.
//                `__any(running)` ends it early when the whole wave is waiting.
// Lanes that hit their boundary mid-block idle until the block ends (T/2 ticks
// on average, against ~400 ticks per step).
struct Lane {
    double buf, dl, target, c, c_next;   // buffer_level, downloaded_size, target_size, bandwidth*dt
    long long sumk;
    int32_t k, k_end, chunk_id, n_su, n_rb, n_play, n_dl, j, tpos, tlen;
    int32_t avail_k, avail_next, cur_action, last_action;
    bool su, be, bf;        // start_up, buffer_empty, buffer_full
    bool done_dl;           // phase B
    bool running;           // ticking inside the current block
    const double *trace;
};

// T1-T3 of tick s.k (Simulator.py:137-149 with R2/R3); sets running = not at a call site
__device__ inline void lane_head(Lane &s) {
    s.n_su += s.su ? 1 : 0;
    s.n_rb += (!s.su && s.be) ? 1 : 0;
    const bool call = s.done_dl && (s.k >= s.avail_k) && !s.bf;
    s.running = !call;
}

__device__ inline void lane_init(Lane &s, const EnvParams &p, int32_t offset0) {
    // Simulator.py:95-130
    s.buf = 0.0; s.dl = 0.0; s.target = 0.0; s.sumk = 0;
    s.k = 0; s.chunk_id = 0; s.n_su = 0; s.n_rb = 0; s.n_play = 0; s.n_dl = 0;
    s.cur_action = -1; s.last_action = -1;
    s.su = true; s.be = true; s.bf = false;
    s.done_dl = true;                  // nothing is downloading: wait for the first call site
    s.j = 0;                           // int(0.0 / interval) == 0
    s.tpos = offset0 % s.tlen;
    s.avail_k = p.avail_tick[0];
    s.avail_next = s.avail_k;
    lane_head(s);                      // T1-T3 of tick 0
}

// Per-block refresh of the interval constants.  Moves j/tpos forward while k has
// passed the interval end (also covers intervals shorter than one tick), then
// loads bandwidth*dt for the current and the next interval.
__device__ inline void lane_refresh_interval(Lane &s, const EnvParams &p) {
    int32_t ke = p.interval_tick[s.j + 1];
    while (s.k >= ke) {
        s.j++;
        s.tpos = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
        ke = p.interval_tick[s.j + 1];
    }
    s.k_end = ke;
    const int32_t tn = (s.tpos + 1 == s.tlen) ? 0 : s.tpos + 1;
    s.c = s.trace[s.tpos] * kDt;       // bandwidth * dt  (:160; the product is formed first)
    s.c_next = s.trace[tn] * kDt;
}

// average_latency (Simulator.py:179-180).  The reference's recurrence telescopes
// to sum(instant_latency) / play_time with instant_latency = global_time -
// play_time at each playing tick.  We carry the sum as exact integers: the m-th
// playing tick (m = 0..n_play-1) happened at tick k_m, so
//   sum = sum_m (G[k_m] - GP[m])  ~=  dt * sum_m k_m - sd * n_play (n_play - 1) / 2
// which differs from the reference only by float64 drift of the clocks
// (<= 1e-11 relative, measured in tests); it feeds no decision.
__device__ inline double avg_latency_from(double sd, double play_time, long long sumk, int32_t n_play) {
    if (n_play == 0) return 0.0;
    double tri = (double)(((long long)n_play * (n_play - 1)) / 2);
    return (kDt * (double)sumk - sd * tri) / play_time;
}
__device__ inline double lane_avg_latency(const EnvParams &p, long long sumk, int32_t n_play) {
    return avg_latency_from(p.sd, p.GP[n_play], sumk, n_play);
}
// with a speed schedule play_time is not n_play equal steps: the sum of play_time over the playing
// ticks is carried instead of the closed form sd * n(n-1)/2
__device__ inline double avg_latency_sched(double play_time, long long sumk, double pt_sum, int32_t n_play) {
    if (n_play == 0) return 0.0;
    return (kDt * (double)sumk - pt_sum) / play_time;
}

__device__ inline void lane_load(Lane &s, const EnvParams &p, int64_t i) {
    s.buf = p.buf[i]; s.sumk = p.sumk[i];
    s.k = p.k[i]; s.chunk_id = p.chunk_id[i]; s.n_su = p.n_su[i]; s.n_rb = p.n_rb[i];
    s.n_play = p.n_play[i]; s.j = p.j[i]; s.tpos = p.tpos[i];
    s.last_action = p.last_action[i]; s.cur_action = -1;
    const uint8_t f = p.flags[i];
    s.su = f & kFlagStartUp; s.be = f & kFlagBufEmpty; s.bf = f & kFlagBufFull;
    s.dl = 0.0; s.n_dl = 0; s.target = 0.0; s.done_dl = true; s.running = false;
    const int32_t c = s.chunk_id < p.video_length ? s.chunk_id : p.video_length;
    s.avail_k = p.avail_tick[c];
    s.avail_next = s.avail_k;
}

__device__ inline void lane_store(const Lane &s, const EnvParams &p, int64_t i) {
    p.buf[i] = s.buf; p.sumk[i] = s.sumk;
    p.k[i] = s.k; p.chunk_id[i] = s.chunk_id; p.n_su[i] = s.n_su; p.n_rb[i] = s.n_rb;
    p.n_play[i] = s.n_play; p.j[i] = s.j; p.tpos[i] = s.tpos; p.last_action[i] = s.last_action;
    p.flags[i] = (uint8_t)((s.su ? kFlagStartUp : 0) | (s.be ? kFlagBufEmpty : 0) |
                           (s.bf ? kFlagBufFull : 0) | kFlagArmed);
}

__device__ inline void write_obs(const Lane &s, const EnvParams &p, int64_t i, float *obs,
                                 double last_bw) {
    if (!obs) return;
    const int64_t n = p.n_lanes;
    obs[ABR_OBS_CHUNK_ID * n + i] = (float)s.chunk_id;
    obs[ABR_OBS_LAST_BITRATE * n + i] = (float)s.last_action;
    obs[ABR_OBS_LAST_BANDWIDTH * n + i] = (float)last_bw;
    obs[ABR_OBS_BUFFER_LEVEL * n + i] = (float)s.buf;
    obs[ABR_OBS_GLOBAL_TIME * n + i] = (float)p.G[s.k];
    obs[ABR_OBS_PLAY_TIME * n + i] = (float)p.GP[s.n_play];
    obs[ABR_OBS_REBUFFER_TIME * n + i] = (float)p.G[s.n_rb];
    obs[ABR_OBS_STARTUP_TIME * n + i] = (float)p.G[s.n_su];
}

// The variance term of calculate_qoe (Simulator.py:82-83: sum over the episode of |br[a_i] - br[a_(i+1)]|) is accumulated as the
// episode goes -- the same terms in the same order as the loop over previous_bitrates, hence the same float64 -- and left in
// ep_qoe_terms[3] when the episode ends.  (Rounds 1-4 copied the episode's 48 actions aside at every auto-reset for K4 to
// loop over: six dependent rounds of byte loads and stores per lane, ~10 us per episode end for the whole workgroup.)

// MODE 4's action: a standard bitrate rule (abr_lane_jump.h: rule_select) on the lane's call-site state -- chunk_id,
// buffer_level, and previous_bandwidths read back from the lane's bw_hist rows (coalesced: row stride n_lanes; the rows
// of this launch's earlier decisions are the lane's own stores); FastMPC also reads previous_bitrates[-1] (pv)
// Under a size table RATE and BOLA read the effective bitrates (abr_lane_jump.h: rule_cost).  SIZED: as chunk_target.
template <bool SIZED = true>
__device__ inline int32_t rule_action(const EnvParams &p, const abrx::RuleParams &rule, int64_t i, int32_t c, int32_t pv,
                                      double B) {
    const auto hist = [&](int32_t j) { return p.bw_hist[(int64_t)j * p.n_lanes + i]; };
    if constexpr (SIZED) {
        // a branch of its own around the whole rule, so that the unsized path's accessor stays the plain one
        if (p.sz_table && abrx::rule_reads_cost(rule.kind)) {
            const double *row = p.sz_table + (int64_t)c * p.n_rates;
            const auto e = [&](int32_t m) { return abrx::rule_cost(row, p.chunk_length, m); };
            return abrx::rule_select_at(rule, e, hist, p.n_rates, p.video_length, c, pv, B);
        }
    }
    const auto br = [&](int32_t m) { return chunk_bitrate(p, c, m); };
    return abrx::rule_select_at(rule, br, hist, p.n_rates, p.video_length, c, pv, B);
}

// The episode sampler's (trace, start offset) of episode e of lane i (include/abr_env.h: abr_episode_sampler)
__device__ inline void sampled_episode(const EnvParams &p, const abrx::EpisodeSampler &smp, int64_t i, int32_t e,
                                       int32_t &t, int32_t &off) {
    abrx::episode_assign(smp, (uint64_t)(p.lane_id_base + i), (uint32_t)e, p.n_traces, p.trace_len, t, off);
}

// The episode ledger (include/abr_env.h: abr_episode_ledger): lane i's episode has just ended and its ep_qoe_terms are
// written -- append the same terms, calculate_qoe's sum of them, and what the episode was.  Called only by the LEDGER
// instances; trace_id / offset0 are the FINISHED episode's, read before a re-arm replaces them.
__device__ inline void ledger_record(const EnvParams &p, const abrx::EpisodeLedger &led, int64_t i, double g_rb, double g_su,
                                     double lat, double var_run, int32_t episode_no, int32_t trace_id, int32_t offset0,
                                     int32_t chunks, uint8_t done) {
    abrx::ledger_append(led, p.n_lanes, i, p.wr, p.wv, p.ws, p.wl, g_rb, g_su, lat, var_run, episode_no, trace_id, offset0,
                        chunks, (int32_t)done);
}

// The quality model (include/abr_env.h: abr_episode_quality).  Called only by the QUALITY instances.  quality_term: lane
// i's step has completed the download of `chunk` at rate `a` -- the weighted table entry that comes off the step's reward;
// quality_record: the lane's episode has just ended (where ledger_record is called).
// (the term's variable in the kernels: a double in the QUALITY instances, an empty object in the others, which then hold no
// dead initialisation of it)
struct NoQualityTerm {};
template <bool QUALITY> using QualityTerm = std::conditional_t<QUALITY, double, NoQualityTerm>;
__device__ inline double quality_term(const EnvParams &p, const abrx::EpisodeQuality &ql, int64_t i, int32_t chunk, int32_t a) {
    return abrx::quality_step(ql, p.n_lanes, p.n_rates, i, chunk, a);
}
__device__ inline void quality_record(const EnvParams &p, const abrx::EpisodeQuality &ql, int64_t i, bool rearm) {
    abrx::quality_close(ql, p.n_lanes, i, rearm);
}

// The kernarg segment of env_jump_kernel (by-value arguments lie in it like a C struct; the code object's metadata gives each
// argument's .offset).  The QUALITY instances read the ledger and the quality model from it afresh where an episode ends,
// through a vector register, as the role-split kernels do (abr_env_roles.h: ledger_record_split, and for its reason): held as
// kernel arguments across the decision loop, the two are ten more live scalars next to the model's per-step three, and
// the instances with both came out with 12-72 B of private segment per lane.
struct JumpKernargs {
    EnvParams p;
    const int32_t *actions, *trace_id_in, *offset_in;
    const uint8_t *lane_mask;
    float *obs_out, *reward_out;
    uint8_t *done_out;
    int32_t *actions_out;
    int32_t n_steps;
    uint64_t seed;
    abrx::RuleParams rule;
    abrx::EpisodeSampler smp;
    abrx::EpisodeLedger led;
    abrx::EpisodeQuality ql;
};
static_assert(offsetof(JumpKernargs, n_steps) == sizeof(EnvParams) + 64 && offsetof(JumpKernargs, seed) == sizeof(EnvParams) + 72 &&
              offsetof(JumpKernargs, rule) == sizeof(EnvParams) + 80 &&
              offsetof(JumpKernargs, smp) == sizeof(EnvParams) + 80 + sizeof(abrx::RuleParams) &&
              offsetof(JumpKernargs, ql) == offsetof(JumpKernargs, led) + 16 &&
              sizeof(JumpKernargs) == offsetof(JumpKernargs, ql) + 32, "env_jump_kernel's kernarg segment");
__device__ __forceinline__ const JumpKernargs &fresh_jump_args() {
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+v"(kp));
    return *(const JumpKernargs *)kp;
}

// MODE 0: reset (fresh lanes run to their first call site)
// MODE 1: step  (one externally supplied action per lane)
// MODE 2: fused random-policy rollout of n_steps decisions per lane
// MODE 3: fused rollout of n_steps scripted decisions per lane, actions[step][lane]
// MODE 4: fused rollout of n_steps decisions per lane taken by a bitrate rule (`rule`; the other modes ignore it)
// SAMPLE: the instance that runs while an episode sampler is installed: a reset draws each lane's (trace, offset) from
// `smp` (trace_id_in / offset_in unused) and a re-arm draws the new episode's; the other instances never read `smp`
// LEDGER: the instance that runs while an episode ledger is installed: every episode end appends a record to `led`; the
// other instances never read `led` and are, instruction for instruction, what they were without it
// SPEEDS: the tick kernel plays one speed for all lanes (kFeatures), so it exists only as the no-speeds instance
// QUALITY: the instance that runs while a quality model is installed (`ql`): a completed download takes its weighted table
// entry off the reward, every episode end records the episode's sum; the other instances never read `ql`
template <int MODE, bool SAMPLE = false, bool LEDGER = false, bool SPEEDS = false, bool QUALITY = false>
__global__ __launch_bounds__(64) void env_advance_kernel(
    EnvParams p, const int32_t *__restrict__ actions, const int32_t *__restrict__ trace_id_in,
    const int32_t *__restrict__ offset_in, const uint8_t *__restrict__ lane_mask,
    float *__restrict__ obs_out, float *__restrict__ reward_out, uint8_t *__restrict__ done_out,
    int32_t *__restrict__ actions_out, int32_t n_steps, uint64_t seed, abrx::RuleParams rule,
    abrx::EpisodeSampler smp, abrx::EpisodeLedger led, abrx::EpisodeQuality ql) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_range = i < p.n_lanes;
    static_assert(!SPEEDS, "the tick kernel takes no per-lane speeds");
    const int32_t n_total = (MODE >= 2) ? n_steps : 1;
    Lane s;
    bool active = in_range;       // still has work in this launch
    bool touched = in_range;      // state must be written back
    bool fresh = (MODE == 0);     // running a new episode up to its first call site
    bool need_action = false;     // at a call site, waiting for the block loop to hand it an action
    uint8_t done = 0;
    int32_t n_su_obs = 0, n_rb_obs = 0, episode_no = 0, offset0 = 0, prev_action = -1;
    double last_bw = 0.0, hist_n = 0.0, hist_s = 0.0, var_run = 0.0;
    int32_t step_idx = 0;
    s.running = false; s.done_dl = true;

    if (in_range) {
        if (MODE == 0) {
            if (lane_mask && !lane_mask[i]) { active = false; touched = false; }
            if (active) {
                int32_t t;
                if constexpr (SAMPLE) {
                    sampled_episode(p, smp, i, (p.flags[i] & kFlagArmed) ? p.episode_no[i] + 1 : 0, t, offset0);
                } else {
                    t = trace_id_in[i];
                    offset0 = offset_in ? offset_in[i] : 0;
                }
                // a trace id / start offset outside the tables: the lane is frozen with
                // ABR_DONE_BADARG instead of reading out of bounds (it runs on trace 0, unseen)
                if (t < 0 || t >= p.n_traces || offset0 < 0) { done |= ABR_DONE_BADARG; t = 0; offset0 = 0; }
                // a re-armed lane starts a NEW episode of the counter-based policy
                episode_no = (p.flags[i] & kFlagArmed) ? p.episode_no[i] + 1 : 0;
                p.trace_id[i] = t; p.offset0[i] = offset0;
                s.tlen = p.trace_len[t]; s.trace = p.traces + p.trace_off[t];
                lane_init(s, p, offset0);
                if (done) {            // frozen (BADARG): still report the fresh lane's observation, as every implementation does
                    write_obs(s, p, i, obs_out, 0.0);
                    active = false; s.running = false;
                }
            }
        } else {
            done = p.done[i];
            const int32_t t = p.trace_id[i];
            offset0 = p.offset0[i];
            s.tlen = p.trace_len[t]; s.trace = p.traces + p.trace_off[t];
            lane_load(s, p, i);
            n_su_obs = p.n_su_obs[i]; n_rb_obs = p.n_rb_obs[i]; episode_no = p.episode_no[i];
            last_bw = p.last_bw[i]; hist_n = p.hist_n[i]; hist_s = p.hist_s[i]; var_run = p.var_run[i];
            if (done) active = false;
            need_action = active;        // a live lane sits at a call site
        }
    }

    const double L = p.chunk_length, sd = p.sd, max_buffer = p.max_buffer, sul = p.start_up_length;
    const int32_t V = p.video_length, max_ticks = p.max_ticks, T = p.t_block;

    while (__any(active)) {
        // ================= SERVICE: lanes at a step boundary =================
        if (active && !s.running) {
            const bool ended = s.chunk_id >= V;
            const bool timeout = !ended && (s.k >= max_ticks);
            bool emit_obs = !need_action;      // need_action: nothing happened yet in this launch
            if (!need_action && !fresh) {
                const int64_t o = (int64_t)step_idx * p.n_lanes + i;
                double var = 0.0;
                QualityTerm<QUALITY> qw{};
                if (s.done_dl && s.cur_action >= 0) {
                    // the chunk this step downloaded (:164-165)
                    const double bw = s.dl / p.G[s.n_dl];
                    const int64_t h = (int64_t)(s.chunk_id - 1) * p.n_lanes + i;
                    p.bw_hist[h] = bw;
                    p.action_hist[h] = (uint8_t)s.cur_action;
                    last_bw = bw;
                    hist_s = hist_s + 1.0 / bw;        // sum(1/x), list order (mpc.py:86-88)
                    hist_n = hist_n + 1.0;
                    s.last_action = s.cur_action;
                    if (prev_action >= 0)
                        var = fabs(chunk_bitrate(p, s.chunk_id - 1, s.cur_action) -
                                   chunk_bitrate(p, s.chunk_id - 2, prev_action));
                    var_run = var_run + var;
                    if constexpr (QUALITY) qw = quality_term(p, ql, i, s.chunk_id - 1, s.cur_action);
                }
                // per-step split of calculate_qoe (Simulator.py:83-85)
                double r = p.wr * (p.G[s.n_rb] - p.G[n_rb_obs]) +
                           p.ws * (p.G[s.n_su] - p.G[n_su_obs]) + p.wv * var;
                if constexpr (QUALITY) r = r - qw;          // 0.0 without a completed download: no bit of r moves
                if (ended) done |= ABR_DONE_EPISODE;
                if (timeout) done |= ABR_DONE_TIMEOUT;
                if (reward_out) reward_out[o] = (float)r;
                if (done_out) done_out[o] = done;
                n_su_obs = s.n_su; n_rb_obs = s.n_rb;
                s.cur_action = -1;
                if (ended || timeout) {
                    p.ep_qoe_terms[0 * p.n_lanes + i] = p.G[s.n_rb];
                    p.ep_qoe_terms[1 * p.n_lanes + i] = p.G[s.n_su];
                    p.ep_qoe_terms[2 * p.n_lanes + i] = lane_avg_latency(p, s.sumk, s.n_play);
                    p.ep_qoe_terms[3 * p.n_lanes + i] = var_run;
                    if constexpr (LEDGER)
                        ledger_record(p, led, i, p.G[s.n_rb], p.G[s.n_su], lane_avg_latency(p, s.sumk, s.n_play), var_run,
                                      episode_no, p.trace_id[i], offset0, s.chunk_id, done);
                    // (straight from the arguments: this kernel has no register bound to meet, and with the kernarg read of
                    // env_jump_kernel its sampled rule rollouts picked up 36 B of private segment)
                    if constexpr (QUALITY) quality_record(p, ql, i, p.auto_reset && ended);
                    if (p.auto_reset && ended) {
                        // re-arm: this step's obs is the new episode's first call site
                        if constexpr (SAMPLE) {
                            int32_t t;
                            sampled_episode(p, smp, i, episode_no + 1, t, offset0);
                            p.trace_id[i] = t; p.offset0[i] = offset0;
                            s.tlen = p.trace_len[t]; s.trace = p.traces + p.trace_off[t];
                        }
                        lane_init(s, p, offset0);
                        episode_no++;
                        n_su_obs = 0; n_rb_obs = 0;
                        last_bw = 0.0; hist_n = 0.0; hist_s = 0.0; var_run = 0.0;
                        done = 0; fresh = true;
                        emit_obs = !s.running;     // already at a call site only if avail_tick[0] == 0
                    }
                }
            } else if (!need_action && fresh && timeout) {
                done |= ABR_DONE_TIMEOUT;
                if (MODE != 0 && done_out) done_out[(int64_t)step_idx * p.n_lanes + i] = done;
            }
            if (emit_obs) {
                fresh = false;
                float *obs = obs_out ? obs_out + (int64_t)step_idx * ABR_OBS_DIM * p.n_lanes : nullptr;
                write_obs(s, p, i, obs, last_bw);
                step_idx++;
                if (done || step_idx >= n_total) active = false;
                else need_action = true;       // fused: take the next action right away
            }
            if (active && need_action) {
                // ---- the call site: get_next_bitrate's return value (Simulator.py:155-156) ----
                int32_t a;
                if (MODE == 1) a = actions[i];
                else if (MODE == 3) a = actions[(int64_t)step_idx * p.n_lanes + i];
                else if (MODE == 4) a = rule_action<true>(p, rule, i, s.chunk_id, s.last_action, s.buf);
                else a = (int32_t)philox_action(seed, (uint64_t)(p.lane_id_base + i),
                                                (uint32_t)s.chunk_id, (uint32_t)episode_no,
                                                (uint32_t)p.n_rates);
                if ((MODE == 2 || MODE == 4) && actions_out) actions_out[(int64_t)step_idx * p.n_lanes + i] = a;
                need_action = false;
                if (a < 0 || a >= p.n_rates) {
                    done |= ABR_DONE_BADACT;
                    if (done_out) done_out[(int64_t)step_idx * p.n_lanes + i] = done;
                    if (reward_out) reward_out[(int64_t)step_idx * p.n_lanes + i] = 0.0f;
                    float *obs = obs_out ? obs_out + (int64_t)step_idx * ABR_OBS_DIM * p.n_lanes : nullptr;
                    write_obs(s, p, i, obs, last_bw);
                    step_idx++;
                    active = false;
                } else {
                    prev_action = s.last_action;
                    s.cur_action = a;
                    s.target = chunk_target<true>(p, s.chunk_id, a);   // :156 (the kernel's one form: the pointer is tested)
                    s.dl = 0.0; s.n_dl = 0; s.done_dl = false;
                    s.avail_next = p.avail_tick[s.chunk_id + 1];
                    s.running = true;          // T4 of this very tick comes next
                }
            }
        }
        if (!__any(active)) break;
        // ================= PREFETCH interval constants =================
        if (active) lane_refresh_interval(s, p);

        // ================= TICK LOOP: predicated, no memory, no divergence =================
        double buf = s.buf, dl = s.dl, c = s.c;
        const double target = s.target, c_next = s.c_next;
        int32_t k = s.k, k_end = s.k_end, chunk_id = s.chunk_id, n_su = s.n_su, n_rb = s.n_rb;
        int32_t n_play = s.n_play, n_dl = s.n_dl, avail_k = s.avail_k;
        const int32_t avail_next = s.avail_next;
        uint32_t sk = 0;
        bool su = s.su, be = s.be, bf = s.bf, done_dl = s.done_dl;
        bool running = active && s.running;
        bool crossed = false;
        for (int32_t t = 0; t < T; t++) {
            if (!__any(running)) break;
            // ---- T4 download (Simulator.py:152-170) ----
            const bool dling = running && !done_dl;
            const double dl2 = dl + c;                               // :160
            dl = dling ? dl2 : dl;
            n_dl += dling ? 1 : 0;                                   // :161
            const bool hit = dling && (dl2 >= target);               // :163
            done_dl = done_dl || hit;
            chunk_id += hit ? 1 : 0;                                 // :166
            avail_k = hit ? avail_next : avail_k;
            const double bufA = hit ? buf + L : buf;                 // :170
            // ---- T5 playback (:174-187) ----
            const bool playing = running && !(be || su);
            sk += playing ? (uint32_t)k : 0u;                        // latency integral
            n_play += playing ? 1 : 0;
            const double bufB = playing ? bufA - sd : bufA;          // :184
            // ---- T6 buffer flags (:190-198) ----
            bf = bufB >= max_buffer;
            be = bufB <= 0.0;
            buf = be ? 0.0 : bufB;
            // ---- T7 start-up exit (:201-202) ----
            su = su && !(buf >= sul);
            // ---- T8/T9 clock, termination (:205-208) ----
            k += running ? 1 : 0;
            const bool next = running && (chunk_id < V) && (k < max_ticks);
            // ---- T1-T3 of the next tick (:137-149) ----
            n_su += (next && su) ? 1 : 0;
            n_rb += (next && !su && be) ? 1 : 0;
            const bool call = done_dl && (k >= avail_k) && !bf;
            running = next && !call;
            // ---- bandwidth of the next tick's interval (:158-159) ----
            const bool cross = (k == k_end);
            c = cross ? c_next : c;
            crossed = crossed || cross;
        }
        if (active) {
            s.buf = buf; s.dl = dl; s.c = c; s.k = k; s.chunk_id = chunk_id; s.n_su = n_su;
            s.n_rb = n_rb; s.n_play = n_play; s.n_dl = n_dl; s.avail_k = avail_k;
            s.su = su; s.be = be; s.bf = bf; s.done_dl = done_dl; s.running = running;
            s.sumk += (long long)sk;
            (void)crossed;   // j/tpos catch up in lane_refresh_interval
        }
    }

    if (touched) {
        lane_store(s, p, i);
        p.n_su_obs[i] = n_su_obs; p.n_rb_obs[i] = n_rb_obs; p.episode_no[i] = episode_no;
        p.last_bw[i] = last_bw; p.hist_n[i] = hist_n; p.hist_s[i] = hist_s; p.var_run[i] = var_run;
        p.done[i] = done;
        if (MODE != 0) {
            // lanes that were already finished (or finished early in a fused launch)
            // report their terminal record for the remaining steps
            for (int32_t t = step_idx; t < n_total; t++) {
                const int64_t o = (int64_t)t * p.n_lanes + i;
                if (reward_out) reward_out[o] = 0.0f;
                if (done_out) done_out[o] = done;
                if ((MODE == 2 || MODE == 4) && actions_out) actions_out[o] = -1;
                if (obs_out)
                    write_obs(s, p, i, obs_out + (int64_t)t * ABR_OBS_DIM * p.n_lanes, last_bw);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// K1/K2, event-driven form, one thread per lane: abr_lane_jump.h does the per-lane work
// ---------------------------------------------------------------------------
using abrx::LaneJ;

// cascade: whether the drains of this kernel go through the per-binade cascade (abr_exact_jump.h: drain_cascade) where it
// applies.  Same results either way; measured per kernel (profiles/r06_ab_cascade.txt): +3.4 % for one thread per lane at
// 1 M lanes, +2.5 % for the two-wave role split at 131 072 -- and -2 % for the three-wave kernel at 65 536, whose player
// wave is not what an iteration waits for (fewer vector instructions, the same iteration time, more scalar traffic).
//
// SPEEDS: the env kernels exist in two instances.  <true> serves a handle that has per-lane speeds, a speed schedule or a
// speed rule installed; <false> every other handle, and holds none of their code: no test of lane_speeds, no speed state
// in registers, parking words or mailboxes.  The host picks the instance per launch (launch_env), as it picks SAMPLE and
// LEDGER: speeds are latched at a full reset, so env->p.lane_speeds is known at every launch.
// SpeedParams is the ONE door through which the env kernels read the speed part of the parameter block: the <false> view
// has constants for lane_speeds / speed_rows and no accessor at all for the per-lane speed state, so code that would touch
// that state in a no-speeds instance does not compile.
template <bool SPEEDS>
struct SpeedParams;
template <>
struct SpeedParams<true> {
    static __device__ __forceinline__ const double *lane_speeds(const EnvParams &p) { return p.lane_speeds; }
    static __device__ __forceinline__ int32_t speed_rows(const EnvParams &p) { return p.speed_rows; }
    static __device__ __forceinline__ double *sd_lane(const EnvParams &p) { return p.sd_lane; }
    static __device__ __forceinline__ double *pt_lane(const EnvParams &p) { return p.pt_lane; }
    static __device__ __forceinline__ double *pt_sum(const EnvParams &p) { return p.pt_sum; }
    static __device__ __forceinline__ int32_t *pl_left(const EnvParams &p) { return p.pl_left; }
    static __device__ __forceinline__ int32_t *play_id(const EnvParams &p) { return p.play_id; }
};
template <>
struct SpeedParams<false> {
    static __device__ __forceinline__ constexpr const double *lane_speeds(const EnvParams &) { return nullptr; }
    static __device__ __forceinline__ constexpr int32_t speed_rows(const EnvParams &) { return 1; }
};

// TB: the table type filled in -- TablesT<SPEEDS>, or a type derived from it that only changes a trait (abr_lane_jump.h)
template <bool SPEEDS = true, class TB = abrx::TablesT<SPEEDS>>
__device__ inline TB make_tables(const EnvParams &p, bool cascade = true) {
    TB t;
    t.G = p.G; t.interval_tick = p.interval_tick; t.avail_tick = p.avail_tick;
    t.avail_j = p.avail_tick + (int64_t)p.avail_j_blocks * 64;
    t.L = p.chunk_length; t.sd = p.sd; t.max_buffer = p.max_buffer;
    t.start_up_length = p.start_up_length; t.V = p.video_length; t.max_ticks = p.max_ticks;
    using SP = SpeedParams<SPEEDS>;
    if constexpr (SPEEDS) {
        t.per_lane_speed = SP::lane_speeds(p) != nullptr;
        t.speed_rows = SP::lane_speeds(p) ? SP::speed_rows(p) : 0;
        t.speed_stride = p.n_lanes; t.speeds = SP::lane_speeds(p);
    }
    t.drain = p.drain;
    if (SP::lane_speeds(p) || !cascade) t.drain.n = 0;      // per-lane speeds: every lane has a subtrahend of its own
#ifdef ABR_NO_DRAIN_CASCADE
    t.drain.n = 0;                 // A/B knob (tools/diag/csrc: make AB_FLAGS=-DABR_NO_DRAIN_CASCADE ab): round 5's drains
#endif
    return t;
}

template <bool SPEEDS = true>
__device__ inline void lanej_load(LaneJ &s, const EnvParams &p, int64_t i) {
    using SP = SpeedParams<SPEEDS>;
    s.buf = p.buf[i]; s.sumk = p.sumk[i];
    s.k = p.k[i]; s.chunk_id = p.chunk_id[i]; s.n_su = p.n_su[i]; s.n_rb = p.n_rb[i];
    s.n_play = p.n_play[i]; s.cur.j = p.j[i]; s.cur.tpos = p.tpos[i];
    s.last_action = p.last_action[i];
    const uint8_t f = p.flags[i];
    s.su = f & kFlagStartUp; s.be = f & kFlagBufEmpty; s.bf = f & kFlagBufFull;
    const int32_t c = s.chunk_id < p.video_length ? s.chunk_id : p.video_length;
    s.avail_k = p.avail_tick[c];
    if constexpr (SPEEDS) {
        if (SP::lane_speeds(p)) { s.sd = SP::sd_lane(p)[i]; s.pt = SP::pt_lane(p)[i]; } else { s.sd = p.sd; s.pt = 0.0; }
        s.lane = i; s.pl_left = 0; s.play_id = 0; s.pt_sum = 0.0;
        if (SP::lane_speeds(p) && SP::speed_rows(p) >= 2) { s.pl_left = SP::pl_left(p)[i]; s.play_id = SP::play_id(p)[i]; s.pt_sum = SP::pt_sum(p)[i]; }
    } else {
        s.sd = p.sd; s.lane = i;           // the one play speed; no speed state
    }
}

template <bool SPEEDS = true>
__device__ inline void lanej_store(const LaneJ &s, const EnvParams &p, int64_t i) {
    p.buf[i] = s.buf; p.sumk[i] = s.sumk;
    p.k[i] = s.k; p.chunk_id[i] = s.chunk_id; p.n_su[i] = s.n_su; p.n_rb[i] = s.n_rb;
    p.n_play[i] = s.n_play; p.j[i] = s.cur.j; p.tpos[i] = s.cur.tpos; p.last_action[i] = s.last_action;
    p.flags[i] = (uint8_t)((s.su ? kFlagStartUp : 0) | (s.be ? kFlagBufEmpty : 0) |
                           (s.bf ? kFlagBufFull : 0) | kFlagArmed);
    if constexpr (SPEEDS) {
        using SP = SpeedParams<SPEEDS>;
        if (SP::lane_speeds(p)) { SP::sd_lane(p)[i] = s.sd; SP::pt_lane(p)[i] = s.pt; }
        if (SP::lane_speeds(p) && SP::speed_rows(p) >= 2) { SP::pl_left(p)[i] = s.pl_left; SP::play_id(p)[i] = s.play_id; SP::pt_sum(p)[i] = s.pt_sum; }
    }
}

// Outputs (observations, rewards, done bytes, the actions and history rows) are written once and never read by the launch that
// writes them: non-temporal stores, so that they do not evict the tick tables, traces and lane state from the XCD's L2.  Same-box
// A/B (profiles/r05_ab_nt_stores.txt): +1.0 % at 65 536 lanes (three-wave kernel's service role), +0.6 % at 131 072 (two-wave
// kernel's player), +2.7 % at 1 048 576 (one thread per lane: 1.9 GB of outputs per launch).  -DABR_NO_NT_STORES builds the plain form.
#ifndef ABR_NO_NT_STORES
#define ABR_OUT(ref, val) __builtin_nontemporal_store((val), &(ref))
#else
#define ABR_OUT(ref, val) ((ref) = (val))
#endif

template <bool SPEEDS = true>
__device__ inline void write_obs_j(const LaneJ &s, const EnvParams &p, int64_t i, float *obs,
                                   double last_bw) {
    if (!obs) return;
    const int64_t n = p.n_lanes;
    ABR_OUT(obs[ABR_OBS_CHUNK_ID * n + i], (float)s.chunk_id);
    ABR_OUT(obs[ABR_OBS_LAST_BITRATE * n + i], (float)s.last_action);
    ABR_OUT(obs[ABR_OBS_LAST_BANDWIDTH * n + i], (float)last_bw);
    ABR_OUT(obs[ABR_OBS_BUFFER_LEVEL * n + i], (float)s.buf);
    ABR_OUT(obs[ABR_OBS_GLOBAL_TIME * n + i], (float)p.G[s.k]);
    ABR_OUT(obs[ABR_OBS_PLAY_TIME * n + i], (float)(SpeedParams<SPEEDS>::lane_speeds(p) ? s.pt : p.GP[s.n_play]));
    ABR_OUT(obs[ABR_OBS_REBUFFER_TIME * n + i], (float)p.G[s.n_rb]);
    ABR_OUT(obs[ABR_OBS_STARTUP_TIME * n + i], (float)p.G[s.n_su]);
}

// the same rows from table values the caller has already loaded: G[k], play_time, G[n_rb], G[n_su]
__device__ inline void write_obs_vals(const LaneJ &s, const EnvParams &p, int64_t i, float *obs, double last_bw,
                                      double g_k, double g_play, double g_rb, double g_su) {
    if (!obs) return;
    const int64_t n = p.n_lanes;
    ABR_OUT(obs[ABR_OBS_CHUNK_ID * n + i], (float)s.chunk_id);
    ABR_OUT(obs[ABR_OBS_LAST_BITRATE * n + i], (float)s.last_action);
    ABR_OUT(obs[ABR_OBS_LAST_BANDWIDTH * n + i], (float)last_bw);
    ABR_OUT(obs[ABR_OBS_BUFFER_LEVEL * n + i], (float)s.buf);
    ABR_OUT(obs[ABR_OBS_GLOBAL_TIME * n + i], (float)g_k);
    ABR_OUT(obs[ABR_OBS_PLAY_TIME * n + i], (float)g_play);
    ABR_OUT(obs[ABR_OBS_REBUFFER_TIME * n + i], (float)g_rb);
    ABR_OUT(obs[ABR_OBS_STARTUP_TIME * n + i], (float)g_su);
}

// Waves per SIMD the one-thread-per-lane kernels are compiled for.  Round 2: four (128 VGPRs + 48 B of scratch) instead
// of three at 138 VGPRs, +8 % at 262 144 lanes, +5 % at 1 M; a fifth then cost 30 % in spills.  Round 4's shorter segment
// needs 103 VGPRs, so five waves (<= 102 VGPRs) cost one spilled register: +2 % at 131 072 lanes, +4 % at 1 M (1.89e10
// env-steps/s); six (<= 85) -7 % (profiles/r04_ab_download_loop.txt (6))
#ifndef ABR_JUMP_WAVES
#define ABR_JUMP_WAVES 5
#endif
// MODE 1 (ONE decision per launch: abr_env_step, the K1 launches of abr_env_step_mpc -- what `auto` runs at every size) is
// compiled for four waves: a single pass through a decision gains nothing from the fifth wave, and the 102-VGPR bound
// cost it 12 B of scratch per lane (round 5).  MODE 4 (a rule rollout) too: at five waves its rule loops push the
// register bound into 36 B of spills, at four it keeps none.  The episode sampler's instances (SAMPLE) as well: at five
// waves the draw at a re-arm spilled 52-68 B per lane, at four they keep none.  The episode ledger's (LEDGER) for the same
// reason: the append's addresses at five waves took the fused rollout from 32 B of scratch to 100 B.
#ifndef ABR_JUMP_WAVES_ONE
// MODE 1's bound as an A/B knob.  With the no-speeds instances: <1, false, false, false> needs 89 VGPRs, so it runs five
// waves per SIMD under either bound; a bound of five only squeezes the SPEEDS forms (98 -> 96 VGPRs), and abr_env_step
// launches measured 0.5-0.9 % slower with it.  ABR_JUMP_WAVES 4 and 6 against 5 at 1 048 576 lanes: within the run-to-run
// spread (profiles/speed_instances_ab.json: part4_mode1_bound, part4_jump_waves).  Both stay as they were.
#define ABR_JUMP_WAVES_ONE 4
#endif
#define ABR_JUMP_BOUNDS(MODE, SAMPLE) \
    __launch_bounds__(64, ((MODE) == 1 ? ABR_JUMP_WAVES_ONE : ((MODE) == 4 || (SAMPLE)) ? 4 : ABR_JUMP_WAVES))
// SAMPLE, LEDGER, QUALITY: as env_advance_kernel; SPEEDS: see make_tables
template <int MODE, bool SAMPLE = false, bool LEDGER = false, bool SPEEDS = true, bool QUALITY = false>
__global__ ABR_JUMP_BOUNDS(MODE, SAMPLE || LEDGER || QUALITY) void env_jump_kernel(
    EnvParams p, const int32_t *__restrict__ actions, const int32_t *__restrict__ trace_id_in,
    const int32_t *__restrict__ offset_in, const uint8_t *__restrict__ lane_mask,
    float *__restrict__ obs_out, float *__restrict__ reward_out, uint8_t *__restrict__ done_out,
    int32_t *__restrict__ actions_out, int32_t n_steps, uint64_t seed, abrx::RuleParams rule,
    abrx::EpisodeSampler smp, abrx::EpisodeLedger led, abrx::EpisodeQuality ql) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const bool in_range = i < p.n_lanes;
    const int32_t n_total = (MODE >= 2) ? n_steps : 1;
    const abrx::TablesT<SPEEDS> tb = make_tables<SPEEDS>(p);
    using SP = SpeedParams<SPEEDS>;      // (<false>: lane_speeds() is a constant nullptr, so every test of it below folds)
    LaneJ s;
    bool active = in_range, touched = in_range;
    uint8_t done = 0;
    int32_t n_su_obs = 0, n_rb_obs = 0, episode_no = 0, offset0 = 0;
    double last_bw = 0.0, hist_n = 0.0, hist_s = 0.0, var_run = 0.0;
    double g_su_obs = 0.0, g_rb_obs = 0.0;    // G[n_su_obs], G[n_rb_obs] carried in registers

    if (in_range) {
        if (MODE == 0) {
            if (lane_mask && !lane_mask[i]) { active = false; touched = false; }
            if (active) {
                int32_t t;
                if constexpr (SAMPLE) {
                    sampled_episode(p, smp, i, (p.flags[i] & kFlagArmed) ? p.episode_no[i] + 1 : 0, t, offset0);
                } else {
                    t = trace_id_in[i];
                    offset0 = offset_in ? offset_in[i] : 0;
                }
                // a trace id / start offset outside the tables: the lane is frozen with
                // ABR_DONE_BADARG instead of reading out of bounds (it sits on trace 0, unseen)
                const bool bad = t < 0 || t >= p.n_traces || offset0 < 0;
                if (bad) { done |= ABR_DONE_BADARG; t = 0; offset0 = 0; }
                // a re-armed lane starts a NEW episode of the counter-based policy
                episode_no = (p.flags[i] & kFlagArmed) ? p.episode_no[i] + 1 : 0;
                p.trace_id[i] = t; p.offset0[i] = offset0;
                s.cur.tlen = p.trace_len[t]; s.cur.trace = p.traces + p.trace_off[t];
                // play_speed * dt (:182); a rule sets it at the lane's first playing tick (sched_begin_chunk)
                s.sd = (SP::lane_speeds(p) && SP::speed_rows(p) != abrx::kSpeedRowsRule) ? SP::lane_speeds(p)[i] * kDt : p.sd;
                s.lane = i;
                abrx::lanej_init(s, tb, offset0);
                if (!bad && !abrx::lanej_wait_call(s, tb)) done |= ABR_DONE_TIMEOUT;
                write_obs_j<SPEEDS>(s, p, i, obs_out, 0.0);
            }
        } else {
            done = p.done[i];
            const int32_t t = p.trace_id[i];
            offset0 = p.offset0[i];
            s.cur.tlen = p.trace_len[t]; s.cur.trace = p.traces + p.trace_off[t];
            lanej_load<SPEEDS>(s, p, i);
            n_su_obs = p.n_su_obs[i]; n_rb_obs = p.n_rb_obs[i]; episode_no = p.episode_no[i];
            last_bw = p.last_bw[i]; hist_n = p.hist_n[i]; hist_s = p.hist_s[i]; var_run = p.var_run[i];
            g_su_obs = p.G[n_su_obs]; g_rb_obs = p.G[n_rb_obs];
            if (done) active = false;
        }
    }

    if (MODE != 0) {
        // the fused rollouts know which trace interval every call site but a launch's first lies in (abr_lane_jump.h:
        // lanej_begin_step_at); a launch of one decision starts from the workspace, so it searches.  Not the rule rollout
        // (MODE 4) and not the SPEEDS instances: the carried index cost the first a wave per SIMD and the others private
        // segment (profiles/step_start_resources.txt).
        constexpr bool kSiteKnown = (MODE == 2 || MODE == 3) && !SPEEDS;
        int32_t j_site = abrx::kSiteSearch;
        for (int32_t step = 0; step < n_total; step++) {
            const int64_t o = (int64_t)step * p.n_lanes + i;
            float *obs = obs_out ? obs_out + (int64_t)step * ABR_OBS_DIM * p.n_lanes : nullptr;
            if (active) {
                // MODE 4: the rule runs BEFORE the step's burst of loads, so that its loops do not hold the burst's
                // registers live (it decides chunk_id's download: nothing of the step is needed)
                const int32_t a_rule = (MODE == 4) ? rule_action<SPEEDS>(p, rule, i, s.chunk_id, s.last_action, s.buf) : 0;
                // one burst of loads for everything the step needs (issued before the
                // policy arithmetic so that the two overlap)
                const abrx::StepStart st = kSiteKnown ? abrx::lanej_begin_step_at(s.cur, tb, s.k, s.chunk_id, j_site)
                                                      : abrx::lanej_begin_step(s.cur, tb, s.k, s.chunk_id);
                // ---- the call site: get_next_bitrate's return value (Simulator.py:155-156) ----
                int32_t a;
                if (MODE == 1) a = actions[i];
                else if (MODE == 3) a = actions[o];
                else if (MODE == 4) a = a_rule;
                else a = (int32_t)philox_action(seed, (uint64_t)(p.lane_id_base + i),
                                                (uint32_t)s.chunk_id, (uint32_t)episode_no,
                                                (uint32_t)p.n_rates);
                if ((MODE == 2 || MODE == 4) && actions_out) ABR_OUT(actions_out[o], a);
                if (a < 0 || a >= p.n_rates) {
                    done |= ABR_DONE_BADACT;
                    if (reward_out) ABR_OUT(reward_out[o], 0.0f);
                    if (done_out) ABR_OUT(done_out[o], (uint8_t)done);
                    write_obs_j<SPEEDS>(s, p, i, obs, last_bw);
                    active = false;
                } else {
                    const int32_t prev_action = s.last_action;
                    const int32_t chunk = s.chunk_id;
                    const abrx::StepResult r = kSiteKnown
                        ? abrx::lanej_download_and_wait_site(s, tb, st, chunk_target<SPEEDS>(p, chunk, a) /* :156 */, a, j_site)
                        : abrx::lanej_download_and_wait(s, tb, st, chunk_target<SPEEDS>(p, chunk, a) /* :156 */, a);
                    // the reward's two clocks and the observation's four tick-table values in ONE burst of loads
                    const double g_rb = p.G[s.n_rb], g_su = p.G[s.n_su];
                    double o_k = p.G[s.k], o_pl = SP::lane_speeds(p) ? s.pt : p.GP[s.n_play], o_rb = g_rb, o_su = g_su;
                    double var = 0.0;
                    QualityTerm<QUALITY> qw{};
                    if (r.hit) {
                        const int64_t h = (int64_t)chunk * p.n_lanes + i;
                        ABR_OUT(p.bw_hist[h], r.bw);                            // :164
                        ABR_OUT(p.action_hist[h], (uint8_t)a);                  // :165
                        last_bw = r.bw;
                        hist_s = hist_s + 1.0 / r.bw;   // sum(1/x), list order (mpc.py:86-88)
                        hist_n = hist_n + 1.0;
                        if (prev_action >= 0)
                            var = fabs(chunk_bitrate(p, chunk, a) - chunk_bitrate(p, chunk - 1, prev_action));
                        var_run = var_run + var;
                        if constexpr (QUALITY) qw = quality_term(p, ql, i, chunk, a);
                    }
                    // ---- step boundary: per-step split of calculate_qoe (:83-85) ----
                    double rew = p.wr * (g_rb - g_rb_obs) + p.ws * (g_su - g_su_obs) + p.wv * var;
                    if constexpr (QUALITY) rew = rew - qw;      // 0.0 without a completed download: no bit of rew moves
                    if (r.ended) done |= ABR_DONE_EPISODE;
                    if (r.timeout) done |= ABR_DONE_TIMEOUT;
                    if (reward_out) ABR_OUT(reward_out[o], (float)rew);
                    if (done_out) ABR_OUT(done_out[o], (uint8_t)done);
                    n_su_obs = s.n_su; n_rb_obs = s.n_rb;
                    g_su_obs = g_su; g_rb_obs = g_rb;
                    if (r.ended || r.timeout) {
                        p.ep_qoe_terms[0 * p.n_lanes + i] = g_rb;
                        p.ep_qoe_terms[1 * p.n_lanes + i] = g_su;
                        p.ep_qoe_terms[2 * p.n_lanes + i] =
                            !SP::lane_speeds(p) ? lane_avg_latency(p, s.sumk, s.n_play)
                            : (SP::speed_rows(p) >= 2 ? avg_latency_sched(s.pt, s.sumk, s.pt_sum, s.n_play)
                                                    : avg_latency_from(s.sd, s.pt, s.sumk, s.n_play));
                        p.ep_qoe_terms[3 * p.n_lanes + i] = var_run;
                        if constexpr (QUALITY) {  // (the ledger and the model from the kernarg segment: JumpKernargs)
                            const JumpKernargs &ka = fresh_jump_args();
                            if constexpr (LEDGER)
                                ledger_record(p, ka.led, i, g_rb, g_su, p.ep_qoe_terms[2 * p.n_lanes + i], var_run, episode_no,
                                              p.trace_id[i], offset0, s.chunk_id, done);
                            quality_record(p, ka.ql, i, p.auto_reset && r.ended);
                        } else if constexpr (LEDGER)     // the latency term as stored: read back (this thread's own store)
                            ledger_record(p, led, i, g_rb, g_su, p.ep_qoe_terms[2 * p.n_lanes + i], var_run, episode_no,
                                          p.trace_id[i], offset0, s.chunk_id, done);
                        if (p.auto_reset && r.ended) {
                            // re-arm: this step's obs is the new episode's first call site
                            if constexpr (SAMPLE) {
                                int32_t t;
                                sampled_episode(p, smp, i, episode_no + 1, t, offset0);
                                p.trace_id[i] = t; p.offset0[i] = offset0;
                                s.cur.tlen = p.trace_len[t]; s.cur.trace = p.traces + p.trace_off[t];
                            }
                            abrx::lanej_init(s, tb, offset0);
                            episode_no++;
                            n_su_obs = 0; n_rb_obs = 0; g_su_obs = 0.0; g_rb_obs = 0.0;
                            last_bw = 0.0; hist_n = 0.0; hist_s = 0.0; var_run = 0.0;
                            done = 0;
                            if (!abrx::lanej_wait_call(s, tb)) done |= ABR_DONE_TIMEOUT;
                            // a fresh cursor, and a call site at the first chunk's availability
                            if (kSiteKnown) j_site = s.k == tb.avail_tick[0] ? tb.avail_j[0] : abrx::kSiteSearch;
                            o_k = p.G[s.k]; o_pl = SP::lane_speeds(p) ? s.pt : p.GP[s.n_play];
                            o_rb = p.G[s.n_rb]; o_su = p.G[s.n_su];
                        }
                    }
                    write_obs_vals(s, p, i, obs, last_bw, o_k, o_pl, o_rb, o_su);
                    if (done) active = false;
                }
            } else if (in_range) {
                // lanes already finished report their terminal record again
                if (reward_out) ABR_OUT(reward_out[o], 0.0f);
                if (done_out) ABR_OUT(done_out[o], (uint8_t)done);
                if ((MODE == 2 || MODE == 4) && actions_out) ABR_OUT(actions_out[o], (int32_t)-1);
                write_obs_j<SPEEDS>(s, p, i, obs, last_bw);
            }
        }
    }

    if (touched) {
        lanej_store<SPEEDS>(s, p, i);
        p.n_su_obs[i] = n_su_obs; p.n_rb_obs[i] = n_rb_obs; p.episode_no[i] = episode_no;
        p.last_bw[i] = last_bw; p.hist_n[i] = hist_n; p.hist_s[i] = hist_s; p.var_run[i] = var_run;
        p.done[i] = done;
    }
}

#include "abr_env_roles.h"     // K1, role-split form: env_split3_kernel (three waves per 64 lanes), env_split_kernel (two)
// Diagnostic builds only (tools/diag/csrc; `auto` never picks them, the product library does not contain them):
#ifdef ABR_WITH_RING
#include "abr_env_ring.h"      // the role pipeline coupled by LDS rings instead of a per-iteration barrier (round 5, impl 6)
#include "abr_env_pair.h"      // download and player wave in lock-step, the service wave behind a ring (round 5, impl 7)
#endif
#ifdef ABR_WITH_ASYNC
#include "abr_env_async.h"     // the asynchronous pipeline of round 3 (impl 4)
#endif

// K4: calculate_qoe in the reference's operation order (Simulator.py:79-86)
__global__ void episode_qoe_kernel(EnvParams p, double *__restrict__ qoe_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_lanes) return;
    double variance = 0.0;
    if (p.auto_reset) {
        // previous_bitrates now holds the NEXT episode's actions: the finished episode's sum was left here when it ended
        variance = p.ep_qoe_terms[3 * p.n_lanes + i];
    } else {
        for (int c = 0; c < p.video_length - 1; c++) {
            int a0 = p.action_hist[(int64_t)c * p.n_lanes + i], a1 = p.action_hist[(int64_t)(c + 1) * p.n_lanes + i];
            variance += fabs(chunk_bitrate(p, c, a0) - chunk_bitrate(p, c + 1, a1));   // :82
        }
    }
    qoe_out[i] = p.wr * p.ep_qoe_terms[0 * p.n_lanes + i] + p.wv * variance +
                 p.ws * p.ep_qoe_terms[1 * p.n_lanes + i] +
                 p.wl * p.ep_qoe_terms[2 * p.n_lanes + i];               // :83-86
}

__global__ void observe_f64_kernel(EnvParams p, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_lanes) return;
    const int64_t n = p.n_lanes;
    out[ABR_F64_GLOBAL_TIME * n + i] = p.G[p.k[i]];
    out[ABR_F64_REBUFFER_TIME * n + i] = p.G[p.n_rb[i]];
    out[ABR_F64_STARTUP_TIME * n + i] = p.G[p.n_su[i]];
    int32_t P = p.play_ticks_per_chunk;
    const bool sched = p.lane_speeds && p.speed_rows >= 2;
    if (p.lane_speeds) {
        // per-lane speed: ticks per played chunk = additions of speed*dt from 0 until >= L (:185)
        double x = 0.0; int32_t a = 0;
        abrx::chain<abrx::STOP_GE>(x, p.sd_lane[i], p.chunk_length, p.max_ticks + 1, a);
        P = a > 0 ? a : 1;
        out[ABR_F64_PLAY_TIME * n + i] = p.pt_lane[i];
        out[ABR_F64_AVERAGE_LATENCY * n + i] =
            sched ? avg_latency_sched(p.pt_lane[i], p.sumk[i], p.pt_sum[i], p.n_play[i])
                  : avg_latency_from(p.sd_lane[i], p.pt_lane[i], p.sumk[i], p.n_play[i]);
    } else {
        out[ABR_F64_PLAY_TIME * n + i] = p.GP[p.n_play[i]];
        out[ABR_F64_AVERAGE_LATENCY * n + i] = lane_avg_latency(p, p.sumk[i], p.n_play[i]);
    }
    out[ABR_F64_BUFFER_LEVEL * n + i] = p.buf[i];
    // play_length restarts from 0 every P playing ticks (:185-187); play_id counts the restarts
    if (sched) {
        // ticks already played of the current played chunk at its speed (0 between chunks)
        const int32_t pl = p.pl_left[i];
        double x = 0.0; int32_t a = 0;
        abrx::chain<abrx::STOP_GE>(x, p.sd_lane[i], 1.0e300, pl > 0 ? P - pl : 0, a);
        out[ABR_F64_PLAY_LENGTH * n + i] = x;
    } else if (p.lane_speeds) {
        double x = 0.0; int32_t a = 0;
        abrx::chain<abrx::STOP_GE>(x, p.sd_lane[i], 1.0e300, p.n_play[i] % P, a);
        out[ABR_F64_PLAY_LENGTH * n + i] = x;
    } else {
        out[ABR_F64_PLAY_LENGTH * n + i] = p.GP[p.n_play[i] % P];
    }
    out[ABR_F64_LAST_BANDWIDTH * n + i] = p.last_bw[i];
    out[ABR_F64_CHUNK_ID * n + i] = (double)p.chunk_id[i];
    out[ABR_F64_PLAY_ID * n + i] = sched ? (double)p.play_id[i] : (double)(p.n_play[i] / P);
    out[ABR_F64_LAST_BITRATE * n + i] = (double)p.last_action[i];
    out[ABR_F64_FLAGS * n + i] = (double)p.flags[i];
    out[ABR_F64_HIST_N * n + i] = p.hist_n[i];
    out[ABR_F64_HIST_SUM_INV * n + i] = p.hist_s[i];
    out[ABR_F64_TICK * n + i] = (double)p.k[i];
    out[ABR_F64_DOWNLOAD_TIME * n + i] = 0.0;   // download_time is 0 at every call site (:154)
}

// ---------------------------------------------------------------------------
// host side of the env ABI
// ---------------------------------------------------------------------------
static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// scratch of the fused MPC rollout's predictor kernel, sized for the longest horizon
static size_t mpc_scratch_bytes_max(size_t n_lanes) {
    return n_lanes * ((size_t)ABR_MAX_HORIZON * sizeof(double) + 2 * sizeof(int32_t));
}

struct Layout {
    size_t G, GP, interval_tick, avail_tick;        // table offsets
    size_t f64_state, i64_state, i32_state, u8_state, action_hist, bw_hist, ep_terms;
    size_t mpc_action, mpc_scratch;
    size_t avail_j;                                  // table (appended: layout 2)
    size_t tag;                                      // the layout tag: the workspace's LAST 256 bytes (WorkspaceTag)
    size_t total;
    int32_t max_ticks, n_intervals;
};

// Default per-episode tick bound: 32 x the live-stream minimum V * ceil(L/dt), capped at 16e6
// ticks (a 128 MB G table) but never below 2 x the minimum; compute_layout rejects a bound
// under which no episode could finish.
static double min_episode_ticks(const abr_env_config *c) {
    return ((double)c->video_length + 1.0) * ceil(c->chunk_length / kDt);
}
static double default_max_ticks(const abr_env_config *c) {
    double per_chunk = ceil(c->chunk_length / kDt);
    double mt = 32.0 * c->video_length * per_chunk;
    if (mt > 16.0e6) mt = 16.0e6;
    if (mt < 2.0 * min_episode_ticks(c)) mt = 2.0 * min_episode_ticks(c);
    if (mt < 1024) mt = 1024;
    return mt;
}

static int validate_cfg(const abr_env_config *c) {
    if (!c) return fail(ABR_E_INVALID, "config is NULL");
    if (c->n_rates < 1 || c->n_rates > ABR_MAX_RATES)
        return fail(ABR_E_INVALID, "n_rates %d outside 1..%d", c->n_rates, ABR_MAX_RATES);
    if (c->video_length < 1 || c->video_length > 65535)
        return fail(ABR_E_INVALID, "video_length %d outside 1..65535", c->video_length);
    if (!(c->chunk_length > 0) || !(c->interval > 0) || !(c->speed > 0))
        return fail(ABR_E_INVALID, "chunk_length, interval and speed must be > 0");
    if (!(c->max_buffer > 0)) return fail(ABR_E_INVALID, "max_buffer must be > 0");
    if (!(c->start_up_length >= 0)) return fail(ABR_E_INVALID, "start_up_length must be >= 0");
    if (c->chunk_length / kDt > 1.0e6)
        return fail(ABR_E_UNSUPPORTED, "chunk_length %g s is more than 1e6 ticks", c->chunk_length);
    for (int r = 0; r < c->n_rates; r++)
        if (!(c->ladder[r] > 0)) return fail(ABR_E_INVALID, "ladder[%d] must be > 0", r);
    return ABR_OK;
}

static int compute_layout(const abr_env_config *c, int64_t n_lanes, Layout *L) {
    int rc = validate_cfg(c);
    if (rc) return rc;
    if (n_lanes < 1) return fail(ABR_E_INVALID, "n_lanes must be >= 1");
    const double mtd = c->max_ticks > 0 ? (double)c->max_ticks : default_max_ticks(c);
    if (mtd > 256.0e6)
        return fail(ABR_E_UNSUPPORTED, "video_length %d x chunk_length %g s needs a %g-entry tick table",
                    c->video_length, c->chunk_length, mtd);
    if (mtd < min_episode_ticks(c))
        return fail(ABR_E_INVALID, "max_ticks %g is below (video_length + 1) * ceil(chunk_length / dt) = %g: "
                    "every lane would end in ABR_DONE_TIMEOUT", mtd, min_episode_ticks(c));
    const int32_t mt = (int32_t)mtd;
    double n_iv = (double)mt * kDt / c->interval + 4.0;
    if (n_iv > 32.0e6)
        return fail(ABR_E_UNSUPPORTED, "interval %g s needs a %g-entry tick table", c->interval, n_iv);
    L->max_ticks = mt;
    L->n_intervals = (int32_t)n_iv;
    size_t o = 0;
    const size_t A = 256;
    size_t N = (size_t)n_lanes, V = (size_t)c->video_length;
    L->G = o; o = align_up(o + sizeof(double) * ((size_t)mt + 2), A);
    L->GP = o; o = align_up(o + sizeof(double) * ((size_t)mt + 2), A);
    L->interval_tick = o; o = align_up(o + sizeof(int32_t) * ((size_t)L->n_intervals + 8), A);
    L->avail_tick = o; o = align_up(o + sizeof(int32_t) * (V + 2), A);
    L->f64_state = o; o = align_up(o + sizeof(double) * 8 * N, A);
    L->i64_state = o; o = align_up(o + sizeof(long long) * 1 * N, A);
    L->i32_state = o; o = align_up(o + sizeof(int32_t) * 15 * N, A);
    L->u8_state = o; o = align_up(o + 2 * N, A);
    L->action_hist = o; o = align_up(o + V * N, A);
    L->bw_hist = o; o = align_up(o + sizeof(double) * V * N, A);
    L->ep_terms = o; o = align_up(o + sizeof(double) * 4 * N, A);
    L->mpc_action = o; o = align_up(o + sizeof(int32_t) * N, A);
    L->mpc_scratch = o; o = align_up(o + mpc_scratch_bytes_max(N), A);
    L->avail_j = o; o = align_up(o + sizeof(int32_t) * (V + 2), A);
    L->tag = o; o = align_up(o + sizeof(WorkspaceTag), A);
    L->total = o;
    return ABR_OK;
}

extern "C" int abr_env_workspace_bytes(const abr_env_config *cfg, int64_t n_lanes,
                                       size_t *bytes_out) {
    Layout L;
    int rc = compute_layout(cfg, n_lanes, &L);
    if (rc) return rc;
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    *bytes_out = L.total;
    return ABR_OK;
}

extern "C" int abr_env_create(const abr_env_config *cfg, const double *traces_dev,
                              const int64_t *trace_off_dev, const int32_t *trace_len_dev,
                              int32_t n_traces, int64_t n_lanes, void *workspace_dev,
                              size_t workspace_bytes, void *stream, abr_env **env_out) {
    Layout L;
    int rc = compute_layout(cfg, n_lanes, &L);
    if (rc) return rc;
    if (!env_out) return fail(ABR_E_INVALID, "env_out is NULL");
    if (!traces_dev || !trace_off_dev || !trace_len_dev || n_traces < 1)
        return fail(ABR_E_INVALID, "trace arrays missing");
    if (!workspace_dev || ((uintptr_t)workspace_dev & 255))
        return fail(ABR_E_WORKSPACE, "workspace must be non-NULL and 256-B aligned");
    if (workspace_bytes < L.total)
        return fail(ABR_E_WORKSPACE, "workspace has %zu bytes, need %zu", workspace_bytes, L.total);

    // ---- universal tick tables, float64 on the host (abr_tick_tables.h) ----
    const int32_t mt = L.max_ticks;
    abrx::TickTables tt = abrx::build_tick_tables(cfg->interval, cfg->chunk_length, cfg->speed,
                                                  cfg->video_length, mt, L.n_intervals);
    std::vector<double> &G = tt.G, &GP = tt.GP;
    std::vector<int32_t> &itick = tt.interval_tick, &atick = tt.avail_tick;
    const double sd = tt.sd;
    const int32_t P = tt.play_ticks_per_chunk;
    int32_t t_block = tt.min_interval_ticks < 128 ? tt.min_interval_ticks : 128;
    if (t_block < 1) t_block = 1;
    if (P == INT_MAX)
        return fail(ABR_E_UNSUPPORTED, "max_ticks %d too small to play one chunk", mt);

    abr_env *e = new (std::nothrow) abr_env;
    if (!e) return fail(ABR_E_INVALID, "out of host memory");
    memset(e, 0, sizeof(*e));
    e->cfg = *cfg;
    e->impl = 3;
    e->chains_proven = abrx::chains_proven(itick.data(), itick.size(), mt, sd, cfg->chunk_length, cfg->max_buffer, cfg->ladder,
                                           cfg->n_rates);
    e->workspace_bytes = L.total;
    EnvParams &p = e->p;
    p.n_rates = cfg->n_rates; p.video_length = cfg->video_length; p.max_ticks = mt;
    p.auto_reset = cfg->auto_reset; p.play_ticks_per_chunk = P; p.n_intervals = L.n_intervals;
    p.t_block = t_block; p.n_traces = n_traces;
    p.chunk_length = cfg->chunk_length; p.max_buffer = cfg->max_buffer;
    p.start_up_length = cfg->start_up_length;
    p.wr = cfg->rebuffer_weight; p.wv = cfg->variance_weight; p.ws = cfg->startup_weight;
    p.wl = cfg->latency_weight; p.sd = sd;
    for (int r = 0; r < ABR_MAX_RATES; r++) p.ladder[r] = cfg->ladder[r];
    p.n_lanes = n_lanes; p.lane_id_base = 0;
    char *w = (char *)workspace_dev;
    p.G = (const double *)(w + L.G); p.GP = (const double *)(w + L.GP);
    p.interval_tick = (const int32_t *)(w + L.interval_tick);
    p.avail_tick = (const int32_t *)(w + L.avail_tick);
    p.avail_j_blocks = (int32_t)((L.avail_j - L.avail_tick) / 256);   // both 256-byte aligned
    // buffer_level never exceeds max_buffer + chunk_length (a download only starts below max_buffer, :144); a level above
    // the cascade would send its wave through the general chains (abr_lane_jump.h: lanej_drain)
    p.drain = abrx::make_drain_tab(sd, cfg->max_buffer + cfg->chunk_length);
    p.traces = traces_dev; p.trace_off = trace_off_dev; p.trace_len = trace_len_dev;
    const size_t N = (size_t)n_lanes;
    double *f = (double *)(w + L.f64_state);
    p.buf = f; p.last_bw = f + N; p.hist_n = f + 2 * N; p.hist_s = f + 3 * N;
    p.sd_lane = f + 4 * N; p.pt_lane = f + 5 * N; p.pt_sum = f + 6 * N; p.var_run = f + 7 * N; p.lane_speeds = nullptr;
    p.speed_rows = 1;
    p.speed_rule = abrx::SpeedRuleBlock{};
    p.sumk = (long long *)(w + L.i64_state);
    int32_t *q = (int32_t *)(w + L.i32_state);
    p.k = q; p.chunk_id = q + N; p.n_su = q + 2 * N; p.n_rb = q + 3 * N; p.n_play = q + 4 * N;
    p.j = q + 5 * N; p.tpos = q + 6 * N; p.trace_id = q + 7 * N; p.offset0 = q + 8 * N;
    p.last_action = q + 9 * N; p.n_su_obs = q + 10 * N; p.n_rb_obs = q + 11 * N;
    p.episode_no = q + 12 * N; p.pl_left = q + 13 * N; p.play_id = q + 14 * N;
    uint8_t *u = (uint8_t *)(w + L.u8_state);
    p.flags = u; p.done = u + N;
    p.action_hist = (uint8_t *)(w + L.action_hist);
    p.bw_hist = (double *)(w + L.bw_hist);
    p.ep_qoe_terms = (double *)(w + L.ep_terms);
    e->mpc_action = (int32_t *)(w + L.mpc_action);
    e->mpc_scratch = (void *)(w + L.mpc_scratch);

    hipStream_t st = (hipStream_t)stream;
    hipError_t he;
#define UP(dst, vec)                                                                           \
    he = hipMemcpyAsync((void *)(dst), (vec).data(), (vec).size() * sizeof((vec)[0]),          \
                        hipMemcpyHostToDevice, st);                                            \
    if (he != hipSuccess) { delete e; return fail(ABR_E_HIP, "table upload: %s", hipGetErrorString(he)); }
    UP(p.G, G) UP(p.GP, GP) UP(p.interval_tick, itick) UP(p.avail_tick, atick)
    he = hipMemsetAsync(w + L.f64_state, 0, L.total - L.f64_state, st);
    if (he == hipSuccess) { UP(w + L.avail_j, tt.avail_j) }
#undef UP
    if (he == hipSuccess) he = hipMemsetAsync(p.done, ABR_DONE_EPISODE, N, st);  // not reset yet
    {
        WorkspaceTag &tg = e->tag;
        memset(&tg, 0, sizeof(tg));
        tg.magic = kTagMagic; tg.abi_version = ABR_ABI_VERSION; tg.layout_rev = kLayoutRev; tg.n_rates = (uint32_t)cfg->n_rates;
        tg.n_lanes = n_lanes; tg.video_length = cfg->video_length; tg.max_ticks = mt; tg.n_intervals = L.n_intervals;
        tg.total_bytes = L.total; tg.chunk_length = cfg->chunk_length; tg.interval = cfg->interval; tg.speed = cfg->speed;
        e->tag_dev = w + L.tag;
        if (he == hipSuccess) he = hipMemcpyAsync(e->tag_dev, &tg, sizeof(tg), hipMemcpyHostToDevice, st);
    }
    if (he == hipSuccess) he = hipStreamSynchronize(st);   // host vectors die at return
    if (he != hipSuccess) { delete e; return fail(ABR_E_HIP, "workspace init: %s", hipGetErrorString(he)); }
    *env_out = e;
    return ABR_OK;
}

extern "C" int abr_env_destroy(abr_env *env) {
    delete env;
    return ABR_OK;
}

// which implementations this build of the library can run (abr_env_set_impl): the product holds 0, 1, 2, 3, 5
extern "C" int abr_env_has_impl(int32_t impl) {
    switch (impl) {
    case 0: case 1: case 2: case 3: case 5: return 1;
#ifdef ABR_WITH_ASYNC
    case 4: return 1;
#endif
#ifdef ABR_WITH_RING
    case 6: case 7: return 1;
#endif
    default: return 0;
    }
}

// Which implementation can serve which feature: bit k of `impls` = impl k.  The tick kernels (1) play one speed for all
// lanes and take no MPC rollout; a speed rule is read where a played chunk begins, which the pipelines 4, 6 and 7 do not
// do; a bitrate rule needs the call-site state in the thread that decides, which the role-split kernels' download wave
// (2, 5: it runs ahead of the player) does not have -- `auto` (3) runs the one-thread-per-lane kernel for it.
enum Feature { kLaneSpeeds, kSpeedRule, kRuleRollout, kMpcRollout, kPolicyRollout };
static const struct { unsigned impls; const char *what; } kFeatures[] = {
    {0xFDu, "per-lane speeds and speed schedules need the event-driven kernels"},   // all but 1
    {0x2Du, "a speed rule needs the event-driven kernels that read it"},            // 0, 2, 3, 5
    {0x0Bu, "rule rollouts run on the one-thread-per-lane kernels"},                // 0, 1, 3
    {0xFDu, "the fused MPC rollout needs the event-driven kernels"},                // all but 1
    {0xFDu, "the fused policy rollout needs the event-driven kernels"},             // all but 1 (as the MPC rollout)
};

// ABR_OK if `impl` can serve `f`, else ABR_E_UNSUPPORTED with a message that names the impls this build accepts for it
static int require(Feature f, int impl) {
    const unsigned ok = kFeatures[f].impls;
    if (ok >> impl & 1u) return ABR_OK;
    int ks[8], n = 0, len = 0;
    for (int k = 0; k < 8; k++)
        if ((ok >> k & 1u) && abr_env_has_impl(k)) ks[n++] = k;
    char list[48] = "";
    for (int i = 0; i < n; i++)
        len += snprintf(list + len, sizeof(list) - len, "%s%d", i == 0 ? "" : i + 1 < n ? ", " : " or ", ks[i]);
    return fail(ABR_E_UNSUPPORTED, "%s (impl %s), not impl %d", kFeatures[f].what, list, impl);
}

// 3 = auto (default), 5 / 2 = role-split event-driven kernels (three / two waves per 64 lanes),
// 0 = event-driven, one thread per lane, 1 = tick-by-tick kernels (kept as a cross-check)
extern "C" int abr_env_set_impl(abr_env *env, int32_t impl) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (impl < 0 || impl > 7)
        return fail(ABR_E_INVALID, "impl must be in 0..7: 0 (jump), 1 (tick), 2 (split), 3 (auto) or 5 (split3); 4, 6 "
                    "and 7 in the diagnostic build; got %d", impl);
    if (!abr_env_has_impl(impl))
        return fail(ABR_E_UNSUPPORTED, "impl %d (4: the asynchronous pipeline, 6: the ring-coupled role pipeline, 7: the pair rendezvous) is not part of "
                    "the product library: it is slower than what `auto` selects; the diagnostic build "
                    "tools/diag/lib/libabr_hip_diag.so carries it", impl);
    // what the running episodes play, or the next full reset will: a rule plays through the per-lane speeds as well
    const bool speeds = env->p.lane_speeds || (env->speeds_dirty && (env->pending_speeds || env->pending_rule_on));
    const bool rule = env->speeds_dirty ? env->pending_rule_on : env->p.speed_rows == abrx::kSpeedRowsRule;
    int rc;
    if (speeds && (rc = require(kLaneSpeeds, impl))) return rc;
    if (rule && (rc = require(kSpeedRule, impl))) return rc;
    env->impl = impl;
    return ABR_OK;
}

// one constant play speed per lane (8f rank 3); nullptr restores the single config speed
extern "C" int abr_env_set_lane_speeds(abr_env *env, const double *speeds_dev) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    int rc;
    if (speeds_dev && (rc = require(kLaneSpeeds, env->impl))) return rc;
    // latched by the next FULL abr_env_reset: until then the running episodes keep the
    // speeds (and the carried play_time) they were started with
    env->pending_speeds = speeds_dev;
    env->pending_speed_rows = 1;
    env->pending_rule_on = false;
    env->speeds_dirty = true;
    if (!env->armed) apply_pending(env);
    return ABR_OK;
}

// a speed controller's answers, one row per played chunk (8f rank 3): speeds_dev [n_rows][n_lanes]
extern "C" int abr_env_set_speed_schedule(abr_env *env, const double *speeds_dev, int32_t n_rows) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    int rc;
    if (speeds_dev && (rc = require(kLaneSpeeds, env->impl))) return rc;
    if (speeds_dev && n_rows < 1) return fail(ABR_E_INVALID, "n_rows must be >= 1");
    env->pending_speeds = speeds_dev;
    env->pending_speed_rows = speeds_dev ? n_rows : 1;
    env->pending_rule_on = false;
    env->speeds_dirty = true;
    if (!env->armed) apply_pending(env);
    return ABR_OK;
}

// a closed-loop speed controller (include/abr_env.h: abr_speed_rule), evaluated where the reference calls get_next_speed()
static int check_speed_rule(const abr_speed_rule *r) {
    const int nl = r->n_lat, nb = r->n_buf;
    if (nl < 0 || nl > ABR_SPEED_RULE_MAX_THR) return fail(ABR_E_INVALID, "speed rule: n_lat must be in 0..4, got %d", nl);
    if (nb < 0 || nb > ABR_SPEED_RULE_MAX_THR) return fail(ABR_E_INVALID, "speed rule: n_buf must be in 0..4, got %d", nb);
    for (int q = 0; q < nl; q++) {
        if (!std::isfinite(r->lat_thr[q])) return fail(ABR_E_INVALID, "speed rule: lat_thr[%d] is not finite", q);
        if (q > 0 && !(r->lat_thr[q] > r->lat_thr[q - 1]))
            return fail(ABR_E_INVALID, "speed rule: lat_thr must be strictly ascending (lat_thr[%d])", q);
    }
    for (int q = 0; q < nb; q++) {
        if (!std::isfinite(r->buf_thr[q])) return fail(ABR_E_INVALID, "speed rule: buf_thr[%d] is not finite", q);
        if (q > 0 && !(r->buf_thr[q] > r->buf_thr[q - 1]))
            return fail(ABR_E_INVALID, "speed rule: buf_thr must be strictly ascending (buf_thr[%d])", q);
    }
    for (int i = 0; i <= nl; i++)
        for (int j = 0; j <= nb; j++)
            if (!(std::isfinite(r->speed[i][j]) && r->speed[i][j] > 0.0))
                return fail(ABR_E_INVALID, "speed rule: speed[%d][%d] must be finite and > 0", i, j);
    return ABR_OK;
}

extern "C" int abr_env_set_speed_rule(abr_env *env, const abr_speed_rule *rule, double *speed_log_dev, int32_t log_rows) {
    // the struct before the handle: a CPU test drives every refusal with env == NULL
    if (rule) {
        const int rc = check_speed_rule(rule);
        if (rc != ABR_OK) return rc;
        if (log_rows < 0) return fail(ABR_E_INVALID, "log_rows must be >= 0, got %d", log_rows);
        if (log_rows > 0 && !speed_log_dev) return fail(ABR_E_INVALID, "log_rows > 0 needs speed_log_dev");
    }
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    int rc;
    if (rule && (rc = require(kSpeedRule, env->impl))) return rc;
    env->pending_speeds = nullptr;
    env->pending_speed_rows = 1;
    env->pending_rule_on = rule != nullptr;
    env->pending_rule = abrx::SpeedRuleBlock{};
    if (rule) {
        std::memcpy(&env->pending_rule.rule, rule, sizeof(abr_speed_rule));
        env->pending_rule.log = log_rows > 0 ? speed_log_dev : nullptr;
        env->pending_rule.log_rows = log_rows > 0 ? log_rows : 0;
    }
    env->speeds_dirty = true;
    if (!env->armed) apply_pending(env);
    return ABR_OK;
}

// per-chunk bitrate ladders [video_length][n_rates] (8f rank 2); nullptr restores the config ladder
extern "C" int abr_env_set_bitrate_table(abr_env *env, const double *br_table_dev) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    env->pending_br_table = br_table_dev;
    env->br_table_dirty = true;
    if (!env->armed) apply_pending(env);
    return ABR_OK;
}

// per-chunk sizes [video_length][n_rates] of what is downloaded (include/abr_env.h); nullptr restores bitrate x chunk_length
extern "C" int abr_env_set_size_table(abr_env *env, const double *sz_table_dev) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    env->pending_sz_table = sz_table_dev;
    env->sz_table_dirty = true;
    if (!env->armed) apply_pending(env);
    return ABR_OK;
}

// the caller has copied a checkpointed workspace into this handle's workspace: episodes are in flight.  The copy must be what
// this handle's abr_env_create would have laid out: the tag in its last 256 bytes says so (read back here: this call
// synchronises the device, once per restore).
extern "C" int abr_env_notify_restore(abr_env *env) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    WorkspaceTag got;
    HIP_TRY(hipDeviceSynchronize());           // the caller's copy may still be in flight on any stream
    HIP_TRY(hipMemcpy(&got, env->tag_dev, sizeof(got), hipMemcpyDeviceToHost));
    const WorkspaceTag &w = env->tag;
    if (got.magic != kTagMagic)
        return fail(ABR_E_WORKSPACE, "the restored workspace carries no layout tag: it was not written by this library at ABI "
                    "version >= 4 (a version-2 / -3 checkpoint cannot be restored: the lane-state layout changed)");
    if (got.abi_version != w.abi_version || got.layout_rev != w.layout_rev)
        return fail(ABR_E_WORKSPACE, "the restored workspace was laid out by ABI version %u (layout %u), this library is %u (%u)",
                    got.abi_version, got.layout_rev, w.abi_version, w.layout_rev);
    if (got.n_lanes != w.n_lanes || got.video_length != w.video_length || got.n_rates != w.n_rates ||
        got.max_ticks != w.max_ticks || got.n_intervals != w.n_intervals || got.total_bytes != w.total_bytes ||
        got.chunk_length != w.chunk_length || got.interval != w.interval || got.speed != w.speed)
        return fail(ABR_E_WORKSPACE, "the restored workspace belongs to another configuration: %lld lanes, %d chunks, %u rates, "
                    "%d ticks, %llu bytes (this handle: %lld, %d, %u, %d, %llu)", (long long)got.n_lanes, got.video_length,
                    got.n_rates, got.max_ticks, (unsigned long long)got.total_bytes, (long long)w.n_lanes, w.video_length,
                    w.n_rates, w.max_ticks, (unsigned long long)w.total_bytes);
    apply_pending(env);
    env->armed = true;
    return ABR_OK;
}

// lane id base for the counter-based policy when lanes are a shard of a bigger job
extern "C" int abr_env_set_lane_id_base(abr_env *env, int64_t base) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    env->p.lane_id_base = base;
    return ABR_OK;
}

// the episode sampler (include/abr_env.h: abr_episode_sampler): the struct before the handle, then the pool against it
extern "C" int abr_env_set_episode_sampler(abr_env *env, const abr_episode_sampler *s) {
    if (s) {
        if (s->pool && s->n_pool < 1) return fail(ABR_E_INVALID, "episode sampler: a pool needs n_pool >= 1, got %d", s->n_pool);
        if (s->offset_span < 0) return fail(ABR_E_INVALID, "episode sampler: offset_span must be >= 0, got %d", s->offset_span);
    }
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (!s) { env->sampler_on = false; env->sampler = abrx::EpisodeSampler{}; return ABR_OK; }
    if (s->pool) {
        // read back once: a trace id outside the tables would be read out of bounds by every kernel that draws it
        std::vector<int32_t> pool((size_t)s->n_pool);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(pool.data(), s->pool, pool.size() * sizeof(int32_t), hipMemcpyDefault));
        for (size_t q = 0; q < pool.size(); q++)
            if (pool[q] < 0 || pool[q] >= env->p.n_traces)
                return fail(ABR_E_INVALID, "episode sampler: pool[%zu] = %d outside [0, %d)", q, pool[q], env->p.n_traces);
    }
    abrx::EpisodeSampler v{};
    v.seed = s->seed; v.pool = s->pool; v.n_pool = s->pool ? s->n_pool : 0; v.offset_span = s->offset_span;
    env->sampler = v;
    env->sampler_on = true;
    return ABR_OK;
}

// the episode ledger (include/abr_env.h: abr_episode_ledger): the layout arithmetic needs no handle and no device
extern "C" int abr_env_ledger_bytes(int32_t n_lanes, int32_t rows, size_t *bytes_out) {
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "episode ledger: n_lanes must be >= 1, got %d", n_lanes);
    if (rows < 1) return fail(ABR_E_INVALID, "episode ledger: rows must be >= 1, got %d", rows);
    *bytes_out = abrx::ledger_layout(n_lanes, rows).bytes;
    return ABR_OK;
}

extern "C" int abr_env_set_episode_ledger(abr_env *env, const abr_episode_ledger *l) {
    if (l) {
        if (l->rows < 1) return fail(ABR_E_INVALID, "episode ledger: rows must be >= 1, got %d", l->rows);
        if (!l->base_dev) return fail(ABR_E_INVALID, "episode ledger: base_dev is NULL");
        if ((uintptr_t)l->base_dev % 256) return fail(ABR_E_INVALID, "episode ledger: base_dev must be 256-byte aligned");
    }
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    abrx::EpisodeLedger v{};
    if (l) { v.base = l->base_dev; v.rows = l->rows; }
    env->ledger = v;
    return ABR_OK;
}

// the quality model (include/abr_env.h: abr_episode_quality): the layout arithmetic needs no handle and no device
extern "C" int abr_env_quality_bytes(int32_t n_lanes, int32_t rows, size_t *bytes_out) {
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "quality model: n_lanes must be >= 1, got %d", n_lanes);
    if (rows < 1) return fail(ABR_E_INVALID, "quality model: rows must be >= 1, got %d", rows);
    *bytes_out = abrx::quality_layout(n_lanes, rows).bytes;
    return ABR_OK;
}

extern "C" int abr_env_set_episode_quality(abr_env *env, const abr_episode_quality *q) {
    if (q) {
        if (!std::isfinite(q->wq)) return fail(ABR_E_INVALID, "quality model: wq must be finite");
        if (!q->u_dev) return fail(ABR_E_INVALID, "quality model: u_dev is NULL");
        if ((uintptr_t)q->u_dev % 8) return fail(ABR_E_INVALID, "quality model: u_dev must be 8-byte aligned");
        if (q->rows < 1) return fail(ABR_E_INVALID, "quality model: rows must be >= 1, got %d", q->rows);
        if (!q->base_dev) return fail(ABR_E_INVALID, "quality model: base_dev is NULL");
        if ((uintptr_t)q->base_dev % 256) return fail(ABR_E_INVALID, "quality model: base_dev must be 256-byte aligned");
    }
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    abrx::EpisodeQuality v{};
    if (q) { v.wq = q->wq; v.u = q->u_dev; v.base = q->base_dev; v.rows = q->rows; }
    env->quality = v;
    return ABR_OK;
}

// each lane's last finished episode's quality sum: a copy of the blob's q_last, ordered on the stream
extern "C" int abr_env_episode_quality(abr_env *env, double *q_out_dev, void *stream) {
    if (!env || !q_out_dev) return fail(ABR_E_INVALID, "NULL argument");
    if (!env->quality.base) return fail(ABR_E_INVALID, "no quality model is installed (abr_env_set_episode_quality)");
    const char *b = (const char *)env->quality.base + abrx::quality_layout(env->p.n_lanes, env->quality.rows).q_last;
    HIP_TRY(hipMemcpyAsync(q_out_dev, b, (size_t)env->p.n_lanes * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return ABR_OK;
}

// abr_env_reset with a quality model: the running sums of the lanes it resets start again at zero
__global__ __launch_bounds__(256) void quality_reset_kernel(abrx::EpisodeQuality ql, int64_t n_lanes,
                                                            const uint8_t *__restrict__ lane_mask) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_lanes && (!lane_mask || lane_mask[i])) abrx::quality_reset(ql, n_lanes, i);
}

// each lane's current (trace, start offset, episode number): copies of the workspace rows, ordered on the stream
extern "C" int abr_env_get_episode(abr_env *env, int32_t *trace_id_out_dev, int32_t *offset_out_dev,
                                   int32_t *episode_out_dev, void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    const size_t bytes = (size_t)env->p.n_lanes * sizeof(int32_t);
    hipStream_t st = (hipStream_t)stream;
    if (trace_id_out_dev) HIP_TRY(hipMemcpyAsync(trace_id_out_dev, env->p.trace_id, bytes, hipMemcpyDeviceToDevice, st));
    if (offset_out_dev) HIP_TRY(hipMemcpyAsync(offset_out_dev, env->p.offset0, bytes, hipMemcpyDeviceToDevice, st));
    if (episode_out_dev) HIP_TRY(hipMemcpyAsync(episode_out_dev, env->p.episode_no, bytes, hipMemcpyDeviceToDevice, st));
    return ABR_OK;
}

static inline unsigned grid64(int64_t n) { return (unsigned)((n + 63) / 64); }

// Which kernel serves which size (same box, fused 48, round 5: profiles/r05_sweep_impl.txt -- the role-split kernels gained
// 18 % from the exact call-site prediction, which moved the crossover up): the three-wave role split while all its waves are
// resident (3 x 1 024 waves at 65 536 lanes: 1.15e10 env-steps/s against 1.01e10 two-wave and 7.7e9 one thread per lane); the
// two-wave role split while all ITS waves are resident (2 x 2 048 waves at 131 072 lanes = four per SIMD: 1.39e10 against
// 1.24e10; 1.18e10 / 1.09e10 at 114 688, 1.02e10 / 9.3e9 at 98 304); one thread per lane above (1.22e10 against 1.11e10 at
// 163 840, 1.55e10 against 1.28e10 at 262 144): it then has three or more waves per SIMD of its own and no barrier.
constexpr int64_t kSplit3MaxLanes = 65536;
constexpr int64_t kSplitMaxLanes = 131072;
// The asynchronous pipeline (abr_env_async.h, impl 4) lost to the role-split kernels on MI355X (714 against 418 us
// per launch at 65 536 lanes, profiles/r03_async_*) and `auto` never picked it: the product library is built
// without it.  `make libabr_hip_async.so` (-DABR_WITH_ASYNC) keeps it selectable for the parity tests and records.
#ifdef ABR_WITH_ASYNC
static inline bool async_eligible(const abr_env *env) {
    return !env->p.lane_speeds && env->p.video_length + 2 <= kAvailLds;
}
#endif
// fused == true: more than one decision per launch (step_random / step_script with n_steps > 1)
static inline int effective_impl(const abr_env *env, bool fused = false) {
    int impl = env->impl;
    if (impl == 3) {
        // ONE decision per launch (abr_env_step, the K1 launches of abr_env_step_mpc, a fused call of one
        // step) is a single pass through download -> player -> service whatever the kernel, so the role
        // pipeline has nothing to overlap: one thread per lane is 3-8 % shorter per launch from 4 096 to
        // 65 536 lanes under the random policy and 30 % under MPC's actions (profiles/r04_sweeps_single_step.txt)
        if (!fused) return 0;
        if (env->p.n_lanes <= kSplit3MaxLanes) return 5;
        return env->p.n_lanes <= kSplitMaxLanes ? 2 : 0;
    }
#ifdef ABR_WITH_ASYNC
    if (impl == 4) return (fused && async_eligible(env)) ? 4 : 2;
#endif
    (void)fused;
    return impl;
}
// The implementation that serves one launch of MODE (see launch_env): a reset and a rule rollout run the tick kernel under
// impl 1 and the one-thread-per-lane kernel otherwise; a launch of one decision (MODE 1, or a fused call with
// n_steps == 1) follows effective_impl(env, false), a fused rollout of more decisions effective_impl(env, true).
template <int MODE>
static inline int launch_impl(const abr_env *env, int32_t n_steps) {
    if (MODE == 0 || MODE == 4) return env->impl == 1 ? 1 : 0;
    return effective_impl(env, n_steps > 1);
}

// The one place the environment kernels are launched, on impl = launch_impl<MODE>(...).  MODE 0: reset (trace_id,
// start_offset, lane_mask); 1: one decision on `actions` [n_lanes]; 2: n_steps decisions of the built-in random policy
// (`seed`); 3: n_steps decisions scripted in `actions` [n_steps][n_lanes]; 4: n_steps decisions of `rule`.  Outputs
// obs / rew / dn / acts as abr_env_step_random, all nullable.  A reset and a rule rollout exist only as the tick and the
// one-thread-per-lane kernel, the asynchronous pipeline only for MODE 2 and 3: the `if constexpr` keeps every other
// instance out of the build.  While an episode sampler is installed the SAMPLE instances run (a reset with explicit trace
// ids excepted: it draws nothing); the diagnostic pipelines have none and refuse.  While per-lane speeds, a speed schedule
// or a speed rule is latched (env->p.lane_speeds, set at a full reset) the SPEEDS instances run, else the no-speeds ones,
// which hold none of that code; the tick kernel (no speeds: kFeatures) and the diagnostic pipelines (written against the
// SPEEDS form of the roles) exist in one form only.
template <int MODE, bool SAMPLE, bool LEDGER, bool SPEEDS, bool QUALITY>
static void launch_env_kernels(const abr_env *env, int impl, hipStream_t st, const int32_t *actions, float *obs, float *rew,
                               uint8_t *dn, int32_t *acts, int32_t n_steps, uint64_t seed, const abrx::RuleParams &rule,
                               const int32_t *trace_id, const int32_t *start_offset, const uint8_t *lane_mask) {
    const EnvParams &p = env->p;
    const int64_t N = p.n_lanes;
    const abrx::EpisodeSampler smp = SAMPLE ? env->sampler : abrx::EpisodeSampler{};
    const abrx::EpisodeLedger led = LEDGER ? env->ledger : abrx::EpisodeLedger{};
    const abrx::EpisodeQuality ql = QUALITY ? env->quality : abrx::EpisodeQuality{};
    if (impl == 0) {
        auto *k = env_jump_kernel<MODE, SAMPLE, LEDGER, SPEEDS, QUALITY>;
        hipLaunchKernelGGL(k, dim3(grid64(N)), dim3(64), 0, st, p, actions, trace_id, start_offset, lane_mask, obs, rew, dn,
                           acts, n_steps, seed, rule, smp, led, ql);
    } else if (impl == 1) {
        // one form whatever SPEEDS says: the tick kernel plays no per-lane speeds (launch_env refuses it a handle that has some)
        auto *k = env_advance_kernel<MODE, SAMPLE, LEDGER, false, QUALITY>;
        hipLaunchKernelGGL(k, dim3(grid64(N)), dim3(64), 0, st, p, actions, trace_id, start_offset, lane_mask, obs, rew, dn,
                           acts, n_steps, seed, rule, smp, led, ql);
    } else if constexpr (MODE >= 1 && MODE <= 3) {
        // the role-split kernels: two waves per 64 lanes (impl 2) or three (impl 5); 6 and 7 in the diagnostic build
        if (impl == 5) {
            auto *k = env_split3_kernel<MODE, SAMPLE, LEDGER, SPEEDS, QUALITY>;
            hipLaunchKernelGGL(k, dim3(grid64(N)), dim3(192), 0, st, p, actions, obs, rew, dn, acts, n_steps, seed, smp, led, ql);
        } else if (impl == 2) {
            auto *k = env_split_kernel<MODE, SAMPLE, LEDGER, SPEEDS, QUALITY>;
            hipLaunchKernelGGL(k, dim3(grid64(N)), dim3(128), 0, st, p, actions, obs, rew, dn, acts, n_steps, seed, smp, led, ql);
        }
#ifdef ABR_WITH_RING
        else if constexpr (!SAMPLE && !LEDGER && SPEEDS && !QUALITY) {
            if (impl == 6)
                hipLaunchKernelGGL(env_ring3_kernel<MODE>, dim3(grid64(N)), dim3(64 * ABR_RING_WAVES), 0, st, p, actions, obs,
                                   rew, dn, acts, n_steps, seed);
            else if (impl == 7)
                hipLaunchKernelGGL(env_pair3_kernel<MODE>, dim3(grid64(N)), dim3(192), 0, st, p, actions, obs, rew, dn, acts,
                                   n_steps, seed);
        }
#endif
    }
}

template <int MODE>
static int launch_env(const abr_env *env, int impl, hipStream_t st, const int32_t *actions, float *obs, float *rew,
                      uint8_t *dn, int32_t *acts, int32_t n_steps, uint64_t seed, const abrx::RuleParams &rule = {},
                      const int32_t *trace_id = nullptr, const int32_t *start_offset = nullptr,
                      const uint8_t *lane_mask = nullptr) {
    const EnvParams &p = env->p;
    const int64_t N = p.n_lanes;
    const bool sample = env->sampler_on && !(MODE == 0 && trace_id);
    if (sample && impl != 0 && impl != 1 && impl != 2 && impl != 5)
        return fail(ABR_E_UNSUPPORTED, "the episode sampler runs on impl 0, 1, 2, 3 and 5, not on the diagnostic impl %d", impl);
    if (env->ledger.base && impl != 0 && impl != 1 && impl != 2 && impl != 5)
        return fail(ABR_E_UNSUPPORTED, "the episode ledger runs on impl 0, 1, 2, 3 and 5, not on the diagnostic impl %d", impl);
    if (env->quality.base && impl != 0 && impl != 1 && impl != 2 && impl != 5)
        return fail(ABR_E_UNSUPPORTED, "the quality model runs on impl 0, 1, 2, 3 and 5, not on the diagnostic impl %d", impl);
    if (env->p.sz_table && impl != 0 && impl != 1 && impl != 2 && impl != 5)
        return fail(ABR_E_UNSUPPORTED, "a size table runs on impl 0, 1, 2, 3 and 5, not on the diagnostic impl %d", impl);
    (void)N;
#ifdef ABR_WITH_ASYNC
    if constexpr (MODE == 2 || MODE == 3) {
        if (impl == 4) {
            // the pipeline takes at most kMaxFuse decisions per launch (its action table lives in LDS); longer
            // rollouts are cut into consecutive launches on the same stream
            for (int32_t s0 = 0; s0 < n_steps; s0 += kMaxFuse) {
                const int32_t n = n_steps - s0 < kMaxFuse ? n_steps - s0 : kMaxFuse;
                hipLaunchKernelGGL(env_async_kernel<MODE>, dim3((unsigned)((N + kAW - 1) / kAW)), dim3(3 * kAW), 0, st,
                                   p, actions ? actions + (int64_t)s0 * N : nullptr,
                                   obs ? obs + (int64_t)s0 * ABR_OBS_DIM * N : nullptr,
                                   rew ? rew + (int64_t)s0 * N : nullptr, dn ? dn + (int64_t)s0 * N : nullptr,
                                   acts ? acts + (int64_t)s0 * N : nullptr, n, seed);
            }
            HIP_TRY(hipGetLastError());
            return ABR_OK;
        }
    }
#endif
    // a reset never ends an episode: it has no LEDGER instance
    const bool ledger = MODE != 0 && env->ledger.base;
    // nor a quality model's download: a reset has no QUALITY instance (abr_env_reset clears the running sums behind it)
    const bool quality = MODE != 0 && env->quality.base;
    // speeds are latched at a full reset (apply_pending), so the handle knows at every launch whether any lane has one
    // ... and a handle whose tables fail the chains' proof (an interval shorter than a tick, more than 2^20 ticks: abr_lane_jump.h,
    // chains_proven) runs the SPEEDS form as well: it accepts the no-speed case, and its chains test their guards per segment
    // ... and a handle with a size table (abr_env_set_size_table): the lookup lives in the SPEEDS form only (chunk_target)
    const bool speeds_on = env->p.lane_speeds != nullptr || !env->chains_proven || env->p.sz_table != nullptr;
    // (never with the tick kernel: the speed setters and abr_env_set_impl refuse that pair, kFeatures)
    const auto go = [&](auto smp_on, auto led_on, auto ql_on) {
        // The no-speeds instances exist for handles WITHOUT an episode sampler.  With the sampler's draw in them, four of
        // the ten one-thread-per-lane instances (MODE 2-4) came out with a 36 B private segment where the SPEEDS form has
        // none (profiles/speed_instances_resources.txt), and no measured workload samples episodes at a size where the
        // slimmer state could pay: a sampled handle keeps running the SPEEDS form, whose speed tests are never taken.
        // The diagnostic pipelines (6, 7) are written against the SPEEDS form of the roles: they run it whatever the handle holds.
        constexpr bool kSample = decltype(smp_on)::value;
        constexpr bool kLedger = decltype(led_on)::value;
        constexpr bool kQuality = decltype(ql_on)::value;
        // a quality model's instances exist in the SPEEDS form only, for the sampler's reason: one more flag times two forms
        // is compile time and code size that no measured workload pays back
        if constexpr (kSample || kQuality) {
            launch_env_kernels<MODE, kSample, kLedger, true, kQuality>(
                env, impl, st, actions, obs, rew, dn, acts, n_steps, seed, rule, trace_id, start_offset, lane_mask);
        } else if (speeds_on || impl == 6 || impl == 7) {
            launch_env_kernels<MODE, false, kLedger, true, false>(
                env, impl, st, actions, obs, rew, dn, acts, n_steps, seed, rule, trace_id, start_offset, lane_mask);
        } else {
            launch_env_kernels<MODE, false, kLedger, false, false>(
                env, impl, st, actions, obs, rew, dn, acts, n_steps, seed, rule, trace_id, start_offset, lane_mask);
        }
    };
    constexpr std::true_type on{};
    constexpr std::false_type off{};
    if constexpr (MODE == 0) {
        if (sample) go(on, off, off);
        else go(off, off, off);
    } else {
        const auto with_quality = [&](auto smp_on, auto led_on) {
            if (quality) go(smp_on, led_on, on);
            else go(smp_on, led_on, off);
        };
        if (sample && ledger) with_quality(on, on);
        else if (sample) with_quality(on, off);
        else if (ledger) with_quality(off, on);
        else with_quality(off, off);
    }
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// Row s of a [n_steps][words][n_lanes] output slab (NULL stays NULL): a rollout that takes its decisions one launch at a
// time (mpc_rollout, policy_rollout) hands each launch its own row.
template <class T>
static inline T *slab_row(T *base, int32_t s, int64_t words, int64_t n_lanes) {
    return base ? base + (int64_t)s * words * n_lanes : nullptr;
}

// The env half of decision s of such a rollout: K1 MODE 1 on `actions` [n_lanes], into row s of obs / rew / dn.
static int step_row(const abr_env *env, int impl, hipStream_t st, int32_t s, const int32_t *actions, float *obs, float *rew,
                    uint8_t *dn) {
    const int64_t N = env->p.n_lanes;
    return launch_env<1>(env, impl, st, actions, slab_row(obs, s, ABR_OBS_DIM, N), slab_row(rew, s, 1, N),
                         slab_row(dn, s, 1, N), nullptr, 1, 0ull);
}

// A rollout of n_steps decisions, one launch pair per decision on `st`: decide(s, action_row) enqueues the controller's
// kernels, which write every lane's action into action_row (row s of actions_out, or the workspace's mpc_action when the
// caller wants none), then K1 MODE 1 downloads it.  Refused on an env kernel that cannot serve `feature`.
template <class Decide>
static int rollout_per_launch(const abr_env *env, Feature feature, int32_t n_steps, int32_t *actions_out, hipStream_t st,
                              float *obs, float *rew, uint8_t *dn, const Decide &decide) {
    int rc = require(feature, env->impl);
    if (rc) return rc;
    const int impl = launch_impl<1>(env, 1);
    for (int32_t s = 0; s < n_steps; s++) {
        int32_t *action_row = actions_out ? slab_row(actions_out, s, 1, env->p.n_lanes) : env->mpc_action;
        if ((rc = decide(s, action_row)) || (rc = step_row(env, impl, st, s, action_row, obs, rew, dn))) return rc;
    }
    return ABR_OK;
}

extern "C" int abr_env_reset(abr_env *env, const int32_t *trace_id_dev,
                             const int32_t *start_offset_dev, const uint8_t *lane_mask_dev,
                             float *obs_out_dev, void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (!trace_id_dev && !env->sampler_on)
        return fail(ABR_E_INVALID, "trace_id_dev is NULL (allowed only while an episode sampler is installed)");
    if (!trace_id_dev && start_offset_dev)
        return fail(ABR_E_INVALID, "a sampled reset (trace_id_dev NULL) takes no start_offset_dev");
    if (env->br_table_dirty && lane_mask_dev)
        return fail(ABR_E_INVALID, "abr_env_set_bitrate_table takes effect at a reset of ALL lanes "
                    "(lane_mask_dev must be NULL for the first reset after it)");
    if (env->sz_table_dirty && lane_mask_dev)
        return fail(ABR_E_INVALID, "abr_env_set_size_table takes effect at a reset of ALL lanes "
                    "(lane_mask_dev must be NULL for the first reset after it)");
    if (env->speeds_dirty && lane_mask_dev)
        return fail(ABR_E_INVALID, "abr_env_set_lane_speeds takes effect at a reset of ALL lanes "
                    "(lane_mask_dev must be NULL for the first reset after it)");
    apply_pending(env);
    env->armed = true;
    const int rc = launch_env<0>(env, launch_impl<0>(env, 0), (hipStream_t)stream, nullptr, obs_out_dev, nullptr, nullptr,
                                 nullptr, 0, 0ull, {}, trace_id_dev, start_offset_dev, lane_mask_dev);
    if (rc || !env->quality.base) return rc;
    // a quality model's running sums belong to the episodes the reset abandons: the reset lanes' start again at zero
    hipLaunchKernelGGL(quality_reset_kernel, dim3((unsigned)((env->p.n_lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       env->quality, env->p.n_lanes, lane_mask_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

extern "C" int abr_env_step(abr_env *env, const int32_t *actions_dev, float *obs_out_dev,
                            float *reward_out_dev, uint8_t *done_out_dev, void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (!actions_dev) return fail(ABR_E_INVALID, "actions_dev is NULL");
    return step_row(env, launch_impl<1>(env, 1), (hipStream_t)stream, 0, actions_dev, obs_out_dev, reward_out_dev,
                    done_out_dev);
}

// n_steps fused decisions per lane under the built-in random policy
extern "C" int abr_env_step_random(abr_env *env, int32_t n_steps, uint64_t seed,
                                   float *obs_out_dev, float *reward_out_dev,
                                   uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    return launch_env<2>(env, launch_impl<2>(env, n_steps), (hipStream_t)stream, nullptr, obs_out_dev, reward_out_dev,
                         done_out_dev, actions_out_dev, n_steps, seed);
}

// The same fused rollout with the ABR controller's answers given up front: what run() does with a
// scripted abr_controller (get_next_bitrate returns actions_dev[step][lane], Simulator.py:155).
extern "C" int abr_env_step_script(abr_env *env, int32_t n_steps, const int32_t *actions_dev,
                                   float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                   void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    if (!actions_dev) return fail(ABR_E_INVALID, "actions_dev is NULL");
    return launch_env<3>(env, launch_impl<3>(env, n_steps), (hipStream_t)stream, actions_dev, obs_out_dev, reward_out_dev,
                         done_out_dev, nullptr, n_steps, 0ull);
}

// ---------------------------------------------------------------------------
// bitrate rules (include/abr_env.h: abr_rule_config)
// ---------------------------------------------------------------------------
static int validate_rule(const abr_rule_config *r, abrx::RuleParams *out) {
    if (!r) return fail(ABR_E_INVALID, "rule is NULL");
    if (r->kind != ABR_RULE_BUFFER && r->kind != ABR_RULE_RATE && r->kind != ABR_RULE_BOLA)
        return fail(ABR_E_INVALID, "unknown rule kind %d", r->kind);
    const double v[5] = {r->reservoir, r->cushion, r->safety, r->bola_v, r->bola_gp};
    for (double x : v)
        if (!std::isfinite(x)) return fail(ABR_E_INVALID, "rule parameters must be finite");
    if (r->kind == ABR_RULE_BUFFER && !(r->reservoir >= 0.0 && r->cushion > 0.0))
        return fail(ABR_E_INVALID, "BUFFER needs reservoir >= 0 and cushion > 0 (got %g, %g)", r->reservoir, r->cushion);
    if (r->kind == ABR_RULE_RATE && r->window < 1) return fail(ABR_E_INVALID, "RATE needs window >= 1 (got %d)", r->window);
    if (r->kind == ABR_RULE_RATE && !(r->safety > 0.0)) return fail(ABR_E_INVALID, "RATE needs safety > 0 (got %g)", r->safety);
    if (r->kind == ABR_RULE_BOLA && !(r->bola_v > 0.0)) return fail(ABR_E_INVALID, "BOLA needs bola_v > 0 (got %g)", r->bola_v);
    if (r->kind == ABR_RULE_BOLA && !r->utility_dev) return fail(ABR_E_INVALID, "BOLA needs utility_dev");
    out->kind = r->kind; out->window = r->window;
    out->reservoir = r->reservoir; out->cushion = r->cushion; out->safety = r->safety;
    out->bola_v = r->bola_v; out->bola_gp = r->bola_gp; out->utility = r->utility_dev;
    return ABR_OK;
}

// A rule rollout runs where the call-site state is at hand: the one-thread-per-lane kernel (`auto` at every size -- the
// role-split kernels' download wave speculates ahead of the player, abr_env_roles.h) or the tick kernel (impl 1).
extern "C" int abr_env_step_rule(abr_env *env, const abr_rule_config *rule, int32_t n_steps, float *obs_out_dev,
                                 float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream) {
    abrx::RuleParams rp;
    int rc = validate_rule(rule, &rp);
    if (rc) return rc;
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if ((rc = require(kRuleRollout, env->impl))) return rc;
    return launch_env<4>(env, launch_impl<4>(env, n_steps), (hipStream_t)stream, nullptr, obs_out_dev, reward_out_dev,
                         done_out_dev, actions_out_dev, n_steps, 0ull, rp);
}

__global__ __launch_bounds__(256) void rule_select_kernel(EnvParams p, abrx::RuleParams rule, int32_t *__restrict__ action_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_lanes) return;
    action_out[i] = p.done[i] ? -1 : rule_action<true>(p, rule, i, p.chunk_id[i], p.last_action[i], p.buf[i]);
}

static int launch_rule_select(const abr_env *env, const abrx::RuleParams &rp, int32_t *action_out_dev, void *stream) {
    hipLaunchKernelGGL(rule_select_kernel, dim3((unsigned)((env->p.n_lanes + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, env->p, rp, action_out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

extern "C" int abr_env_rule_select(abr_env *env, const abr_rule_config *rule, int32_t *action_out_dev, void *stream) {
    abrx::RuleParams rp;
    int rc = validate_rule(rule, &rp);
    if (rc) return rc;
    if (!env || !action_out_dev) return fail(ABR_E_INVALID, "NULL argument");
    return launch_rule_select(env, rp, action_out_dev, stream);
}

extern "C" int abr_env_get_effective_impl(abr_env *env, int32_t fused, int32_t *impl_out) {
    if (!env || !impl_out) return fail(ABR_E_INVALID, "NULL argument");
    *impl_out = effective_impl(env, (fused & 1) != 0);
    // bit 1 of `fused` asks for the instance as well: 0x100 is added when a step launch runs the SPEEDS == true form
    // (launch_env: a latched speed feature, a sampler, a quality model, tables that fail the chains' proof, or a size table
    // in force or pending)
    const bool sized = env->p.sz_table || (env->sz_table_dirty && env->pending_sz_table);
    if ((fused & 2) && (env->p.lane_speeds || !env->chains_proven || env->sampler_on || env->quality.base || sized))
        *impl_out |= 0x100;
    return ABR_OK;
}

extern "C" int abr_env_episode_qoe(abr_env *env, double *qoe_out_dev, void *stream) {
    if (!env || !qoe_out_dev) return fail(ABR_E_INVALID, "NULL argument");
    hipLaunchKernelGGL(episode_qoe_kernel, dim3((unsigned)((env->p.n_lanes + 255) / 256)),
                       dim3(256), 0, (hipStream_t)stream, env->p, qoe_out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

extern "C" int abr_env_observe_f64(abr_env *env, double *out_dev, void *stream) {
    if (!env || !out_dev) return fail(ABR_E_INVALID, "NULL argument");
    hipLaunchKernelGGL(observe_f64_kernel, dim3((unsigned)((env->p.n_lanes + 255) / 256)),
                       dim3(256), 0, (hipStream_t)stream, env->p, out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// ---------------------------------------------------------------------------
// lane fork (include/abr_env.h: abr_env_fork): gather every source column into the scratch, then scatter
// ---------------------------------------------------------------------------
// One thread per (pair, row chunk): x runs over the pairs, so a wave reads 64 gathered columns and writes 64 adjacent
// scratch elements per row (the scatter the other way round); y is the row chunk, uniform per workgroup.
template <bool SCATTER>
__global__ __launch_bounds__(256) void fork_kernel(abrx::ForkTable T, const int32_t *__restrict__ src,
                                                   const int32_t *__restrict__ dst, char *__restrict__ scratch) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    abrx::fork_move(T, (int32_t)blockIdx.y, i, src, dst, scratch, SCATTER);
}

static int fork_check_args(const int32_t *src_dev, int64_t count, const void *scratch_dev) {
    if (!src_dev) return fail(ABR_E_INVALID, "fork: src_dev is NULL");
    if (count < 0) return fail(ABR_E_INVALID, "fork: count must be >= 0, got %lld", (long long)count);
    if (count > INT32_MAX) return fail(ABR_E_INVALID, "fork: count %lld is more than 2^31 - 1 pairs", (long long)count);
    if (count > 0 && (!scratch_dev || (uintptr_t)scratch_dev % 256))
        return fail(ABR_E_INVALID, "fork: scratch_dev must be non-NULL and 256-byte aligned");
    return ABR_OK;
}

extern "C" int abr_env_fork_scratch_bytes(abr_env *env, int64_t count, size_t *bytes_out) {
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    if (count < 0) return fail(ABR_E_INVALID, "fork: count must be >= 0, got %lld", (long long)count);
    if (count > INT32_MAX) return fail(ABR_E_INVALID, "fork: count %lld is more than 2^31 - 1 pairs", (long long)count);
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    abrx::ForkTable T;
    *bytes_out = abrx::fork_table_init(T, env->p.video_length, env->p.n_lanes, count);
    return ABR_OK;
}

extern "C" int abr_env_fork(abr_env *env, const int32_t *src_dev, const int32_t *dst_dev, int64_t count, void *scratch_dev,
                            size_t scratch_bytes, float *obs_dev, void *stream) {
    // the arguments before the handle: a CPU test drives these refusals with env == NULL
    int rc = fork_check_args(src_dev, count, scratch_dev);
    if (rc) return rc;
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (env->impl == 4 || env->impl == 6 || env->impl == 7)
        return fail(ABR_E_UNSUPPORTED, "fork: the diagnostic pipelines (impl 4, 6, 7) keep lane state outside the workspace");
    // per-lane speeds and schedules are caller-owned columns that belong to the slot, not to the lane's state; a constant
    // speed and a speed rule (whose per-lane state is in the workspace) are fine
    const bool lane_speeds = (env->p.lane_speeds && env->p.speed_rows != abrx::kSpeedRowsRule) ||
                             (env->speeds_dirty && env->pending_speeds && !env->pending_rule_on);
    if (lane_speeds)
        return fail(ABR_E_UNSUPPORTED, "fork: per-lane speeds or a speed schedule are in force or pending: their columns "
                    "belong to the slot and are not copied");
    abrx::ForkTable T;
    const EnvParams &p = env->p;
    const size_t need = abrx::fork_table_init(T, p.video_length, p.n_lanes, count);
    if (scratch_bytes < need) return fail(ABR_E_INVALID, "fork: scratch has %zu bytes, %lld pairs need %zu", scratch_bytes,
                                          (long long)count, need);
    if (count == 0) return ABR_OK;
    T.r[abrx::kForkF64].base = (char *)p.buf;             // the 8 float64 rows, buf first (abr_env_create)
    T.r[abrx::kForkI64].base = (char *)p.sumk;
    T.r[abrx::kForkI32].base = (char *)p.k;               // the 15 int32 rows, k first
    T.r[abrx::kForkU8].base = (char *)p.flags;            // flags, done
    T.r[abrx::kForkActionHist].base = (char *)p.action_hist;
    T.r[abrx::kForkBwHist].base = (char *)p.bw_hist;
    T.r[abrx::kForkEpTerms].base = (char *)p.ep_qoe_terms;
    T.r[abrx::kForkMpcAction].base = (char *)env->mpc_action;
    if (env->quality.base)
        T.r[abrx::kForkQRun].base = (char *)env->quality.base + abrx::quality_layout(p.n_lanes, 1).q_run;
    T.r[abrx::kForkObs].base = (char *)obs_dev;
    const dim3 grid((unsigned)((count + 255) / 256), (unsigned)T.chunks), block(256);
    hipLaunchKernelGGL(fork_kernel<false>, grid, block, 0, (hipStream_t)stream, T, src_dev, dst_dev, (char *)scratch_dev);
    hipLaunchKernelGGL(fork_kernel<true>, grid, block, 0, (hipStream_t)stream, T, src_dev, dst_dev, (char *)scratch_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// ---------------------------------------------------------------------------
// beam selection (include/abr_env.h: abr_beam_select): per-group top-B by counting rank in LDS
// ---------------------------------------------------------------------------
constexpr int kBeamMaxSlots = 1024;
// One workgroup per group of S = beam * n_rates consecutive lanes, one thread per slot (blockDim = S rounded up to a wave).
// Every thread reads every key: S broadcast LDS reads per thread, S^2 compares per group, no sort network and no atomics, so
// the ranks are a pure function of the keys.
__global__ __launch_bounds__(kBeamMaxSlots) void beam_select_kernel(
    int32_t S, int32_t n_rates, double wl, const double *__restrict__ R_in, const float *__restrict__ reward,
    const double *__restrict__ lat, const uint8_t *__restrict__ done, const uint8_t *__restrict__ valid_in,
    const double *__restrict__ key_override, int32_t *__restrict__ src_out, double *__restrict__ R_out,
    uint8_t *__restrict__ valid_out) {
    __shared__ double s_key[kBeamMaxSlots], s_R[kBeamMaxSlots];
    __shared__ int32_t s_slot[kBeamMaxSlots];       // slot of the candidate with rank r, or -1
    __shared__ uint8_t s_valid[kBeamMaxSlots];
    const int32_t s = (int32_t)threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * S;
    double key = 0.0;
    bool valid = false;
    if (s < S) {
        const int64_t i = base + s;
        const double Rn = abrx::beam_r_new(R_in[i], reward[i]);
        key = key_override ? key_override[i] : abrx::beam_key(Rn, wl, lat[i]);
        valid = abrx::beam_valid(valid_in[i], done[i], key);
        s_key[s] = key; s_R[s] = Rn; s_valid[s] = valid ? 1 : 0; s_slot[s] = -1;
    }
    __syncthreads();
    if (valid) {
        int32_t rank = 0;
        for (int32_t t = 0; t < S; t++)
            rank += (s_valid[t] && abrx::beam_before(s_key[t], t, key, s)) ? 1 : 0;
        s_slot[rank] = s;                           // ranks of valid candidates are distinct and < S
    }
    __syncthreads();
    if (s < S) {
        const int32_t c = s_slot[s / n_rates];      // s / n_rates < beam <= S
        src_out[base + s] = c >= 0 ? (int32_t)(base + c) : -1;
        R_out[base + s] = c >= 0 ? s_R[c] : 0.0;
        valid_out[base + s] = c >= 0 ? 1 : 0;
    }
}

extern "C" int abr_beam_select(int32_t n_groups, int32_t beam, int32_t n_rates, double wl, const double *R_in_dev,
                               const float *reward_dev, const double *lat_dev, const uint8_t *done_dev,
                               const uint8_t *valid_in_dev, const double *key_override_dev, int32_t *src_out_dev,
                               double *R_out_dev, uint8_t *valid_out_dev, void *stream) {
    if (n_groups < 0) return fail(ABR_E_INVALID, "beam select: n_groups must be >= 0, got %d", n_groups);
    if (beam < 1) return fail(ABR_E_INVALID, "beam select: beam must be >= 1, got %d", beam);
    if (n_rates < 1 || n_rates > ABR_MAX_RATES)
        return fail(ABR_E_INVALID, "beam select: n_rates %d outside 1..%d", n_rates, ABR_MAX_RATES);
    if ((int64_t)beam * n_rates > kBeamMaxSlots)
        return fail(ABR_E_UNSUPPORTED, "beam select: beam %d x n_rates %d is more than %d slots per group", beam, n_rates,
                    kBeamMaxSlots);
    if ((int64_t)n_groups * beam * n_rates > INT32_MAX)
        return fail(ABR_E_INVALID, "beam select: n_groups x beam x n_rates is more than 2^31 - 1 lanes");
    if (!R_in_dev || !reward_dev || !done_dev || !valid_in_dev || !src_out_dev || !R_out_dev || !valid_out_dev)
        return fail(ABR_E_INVALID, "beam select: NULL device pointer");
    if (!lat_dev && !key_override_dev) return fail(ABR_E_INVALID, "beam select: lat_dev is NULL and there is no key_override");
    if (n_groups == 0) return ABR_OK;
    const int32_t S = beam * n_rates;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)n_groups), dim3((unsigned)((S + 63) / 64 * 64)), 0,
                       (hipStream_t)stream, S, n_rates, wl, R_in_dev, reward_dev, lat_dev, done_dev, valid_in_dev,
                       key_override_dev, src_out_dev, R_out_dev, valid_out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// ---------------------------------------------------------------------------
// lookahead expert (include/abr_env.h: abr_env_lookahead_select): the exact tree of the next H decisions, per lane
// ---------------------------------------------------------------------------
// A workgroup is 64 lanes times n_rates waves: wave m walks the subtree a_0 = m of its 64 lanes (abr_lane_jump.h:
// look_subtree), writes its q_out row, and the n_rates candidates meet in LDS for action and key.  One instance per horizon,
// n_rates a run-time value.  The leaf cap bounds the waves an instance can be launched with -- the largest M with M^H <=
// 65 536 -- and that is its __launch_bounds__: the deep instances, whose stack of saved lanes is what costs registers, are
// the ones that never run more than a few waves per workgroup.  W halves the shallow instances once more: up to 8 rates (W
// = 8, 512 threads, 256 registers per lane) and up to 16 (W = 16, 128 registers), because at 1 024 threads horizons 3 and 4
// spilled 48 and 256 bytes per lane to scratch, which the 8-wave form does not (profiles/lookahead_resources.txt).
constexpr int look_max_rates(int H) {
    int m = 1;
    while (m < ABR_MAX_RATES && abrx::look_leaves(m + 1, H) <= abrx::kLookMaxLeaves) m++;
    return m;
}
static_assert(look_max_rates(1) == 16 && look_max_rates(4) == 16 && look_max_rates(5) == 9 && look_max_rates(6) == 6 &&
              look_max_rates(7) == 4 && look_max_rates(8) == 4, "the leaf cap's wave counts");

constexpr int look_waves(int H, int W) { return W < look_max_rates(H) ? W : look_max_rates(H); }

// SIZED: the instance that runs while a size table is in force (abr_env_set_size_table): a step's target is the table's
// entry.  An instance of its own, as the quality model's are in the env kernels: with a run-time test of the pointer in
// the one form, nine of the walks' instances gained 12-40 B of scratch per lane and plan_kernel<2> lost a wave of
// occupancy (profiles/chunk_sizes_resources.txt); the <false> instances hold no trace of the table.
template <int H, int W, bool SIZED>
__global__ __launch_bounds__(64 * look_waves(H, W)) void lookahead_kernel(
    EnvParams p, abrx::EpisodeQuality ql, int64_t lane0, int64_t lane_end, int32_t *__restrict__ action_out,
    double *__restrict__ key_out, double *__restrict__ q_out) {
    __shared__ double s_q[look_waves(H, W)][64];
    const int32_t m = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));     // the wave's first digit, scalar
    const int32_t l = (int32_t)(threadIdx.x & 63);
    const int64_t i = lane0 + (int64_t)blockIdx.x * 64 + l;
    const abrx::TablesChecked tb = make_tables<false, abrx::TablesChecked>(p);   // any handle: the checked chains
    LaneJ s{};
    int32_t n_su_obs = 0, n_rb_obs = 0;
    bool live = false;
    if (i < lane_end && p.done[i] == 0) {      // a lane that was never reset carries ABR_DONE_EPISODE (abr_env_create)
        live = true;
        const int32_t t = p.trace_id[i];
        s.cur.tlen = p.trace_len[t]; s.cur.trace = p.traces + p.trace_off[t];
        lanej_load<false>(s, p, i);
        n_su_obs = p.n_su_obs[i]; n_rb_obs = p.n_rb_obs[i];
    }
    abrx::LookWeights w;
    w.wr = p.wr; w.ws = p.ws; w.wv = p.wv; w.wl = p.wl; w.M = p.n_rates; w.quality = ql.base != nullptr;
    const auto br = [&](int32_t chunk, int32_t rate) { return chunk_bitrate(p, chunk, rate); };
    // the step's target: the size table's entry (abr_env_set_size_table), else rate x chunk_length
    const auto sz = [&](int32_t chunk, int32_t a, double rate) {
        if constexpr (SIZED) return p.sz_table[(int64_t)chunk * p.n_rates + a];
        else return rate * tb.L;
    };
    const auto G = [&](int32_t n) { return p.G[n]; };
    const auto lat = [&](const LaneJ &x) { return lane_avg_latency(p, x.sumk, x.n_play); };
    const auto qt = [&](int32_t chunk, int32_t rate) { return abrx::quality_peek(ql, p.n_rates, chunk, rate); };
    const auto any = [](bool f) { return __any(f) != 0; };
    const double q = abrx::look_subtree<H>(w, tb, br, sz, G, lat, qt, any, s, live, n_rb_obs, n_su_obs, m);
    s_q[m][l] = q;
    if (q_out && i < lane_end) ABR_OUT(q_out[(int64_t)m * p.n_lanes + i], q);
    __syncthreads();
    if (m == 0 && i < lane_end) {
        int32_t action;
        double key;
        abrx::look_pick([&](int32_t r) { return s_q[r][l]; }, p.n_rates, action, key);
        ABR_OUT(action_out[i], action);
        if (key_out) ABR_OUT(key_out[i], key);
    }
}

template <bool SIZED>
struct LookaheadKernels { template <int H, int W> static constexpr auto kernel = lookahead_kernel<H, W, SIZED>; };

// One launch of horizon H's instance of a kernel family on lanes [lane0, lane_end); `tail`: the kernel's arguments behind them.
template <class Kernels, int H, class... Tail>
static void launch_walk(const abr_env *env, int64_t lane0, int64_t lane_end, hipStream_t st, Tail... tail) {
    const dim3 grid(grid64(lane_end - lane0)), block(64u * (unsigned)env->p.n_rates);
    if (env->p.n_rates <= 8 || look_max_rates(H) <= 8)       // (the refusals have bounded n_rates by look_max_rates(H))
        hipLaunchKernelGGL((Kernels::template kernel<H, 8>), grid, block, 0, st, env->p, env->quality, lane0, lane_end, tail...);
    else if constexpr (look_max_rates(H) > 8)
        hipLaunchKernelGGL((Kernels::template kernel<H, 16>), grid, block, 0, st, env->p, env->quality, lane0, lane_end, tail...);
}

// The walk of every lane, in launches of at most max_nodes tree nodes each.
template <class Kernels, class... Tail>
static int launch_walks(const abr_env *env, int32_t H, int64_t max_nodes, hipStream_t st, Tail... tail) {
    const EnvParams &p = env->p;
    const int64_t per = abrx::look_lanes_per_launch(max_nodes, p.n_rates, H);
    for (int64_t lane0 = 0; lane0 < p.n_lanes; lane0 += per) {
        const int64_t lane_end = lane0 + per < p.n_lanes ? lane0 + per : p.n_lanes;
        switch (H) {
        case 1: launch_walk<Kernels, 1>(env, lane0, lane_end, st, tail...); break;
        case 2: launch_walk<Kernels, 2>(env, lane0, lane_end, st, tail...); break;
        case 3: launch_walk<Kernels, 3>(env, lane0, lane_end, st, tail...); break;
        case 4: launch_walk<Kernels, 4>(env, lane0, lane_end, st, tail...); break;
        case 5: launch_walk<Kernels, 5>(env, lane0, lane_end, st, tail...); break;
        case 6: launch_walk<Kernels, 6>(env, lane0, lane_end, st, tail...); break;
        case 7: launch_walk<Kernels, 7>(env, lane0, lane_end, st, tail...); break;
        default: launch_walk<Kernels, 8>(env, lane0, lane_end, st, tail...); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// What a walk's config and decision output must be, whoever asks (`who` opens the message); action_out is looked at only
// where the entry `wants_action`.  The arguments before the handle: a CPU test drives these refusals with env == NULL.
template <class Cfg>
static int validate_walk(const Cfg *cfg, bool wants_action, const void *action_out, const char *who) {
    if (!cfg) return fail(ABR_E_INVALID, "%s: cfg is NULL", who);
    if (wants_action && !action_out) return fail(ABR_E_INVALID, "%s: action_out_dev is NULL", who);
    if (cfg->horizon < 1 || cfg->horizon > ABR_MAX_HORIZON)
        return fail(ABR_E_INVALID, "%s: horizon %d outside 1..%d", who, cfg->horizon, ABR_MAX_HORIZON);
    if (cfg->reserved_ != 0) return fail(ABR_E_INVALID, "%s: reserved_ must be 0, got %d", who, cfg->reserved_);
    if (cfg->max_nodes_per_launch < 0)
        return fail(ABR_E_INVALID, "%s: max_nodes_per_launch must be >= 0, got %lld", who, (long long)cfg->max_nodes_per_launch);
    return ABR_OK;
}

// what the walk cannot serve (ABR_E_UNSUPPORTED), for the lookahead and for the forecast planner (`who` opens the message)
static int look_supported(const abr_env *env, int32_t H, const char *who) {
    const EnvParams &p = env->p;
    if (abrx::look_leaves(p.n_rates, H) > abrx::kLookMaxLeaves)
        return fail(ABR_E_UNSUPPORTED, "%s: %d rates ^ horizon %d is more than %lld leaves; larger trees are the beam "
                    "search's job", who, p.n_rates, H, (long long)abrx::kLookMaxLeaves);
    if (p.lane_speeds || (env->speeds_dirty && (env->pending_speeds || env->pending_rule_on)))
        return fail(ABR_E_UNSUPPORTED, "%s: per-lane speeds, a speed schedule or a speed rule are in force or pending: "
                    "the walk is built from the one-speed tables only", who);
    if (env->impl == 4 || env->impl == 6 || env->impl == 7)
        return fail(ABR_E_UNSUPPORTED, "%s: the diagnostic pipelines (impl 4, 6, 7) keep lane state outside the workspace", who);
    return ABR_OK;
}

extern "C" int abr_env_lookahead_select(abr_env *env, const abr_lookahead_config *cfg, int32_t *action_out_dev,
                                        double *key_out_dev, double *q_out_dev, void *stream) {
    int rc = validate_walk(cfg, true, action_out_dev, "lookahead");
    if (rc) return rc;
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if ((rc = look_supported(env, cfg->horizon, "lookahead"))) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (env->p.sz_table)
        return launch_walks<LookaheadKernels<true>>(env, cfg->horizon, cfg->max_nodes_per_launch, st, action_out_dev,
                                                    key_out_dev, q_out_dev);
    return launch_walks<LookaheadKernels<false>>(env, cfg->horizon, cfg->max_nodes_per_launch, st, action_out_dev, key_out_dev,
                                                 q_out_dev);
}

#ifdef ABR_SPLIT_STAMPS
extern "C" int abr_debug_read_stamps(unsigned long long *out32, int reset) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_st_acc), 32 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[32] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_st_acc), z, sizeof(z)); }
    return 0;
}
#endif

#ifdef ABR_SPLIT_STAMPS
extern "C" int abr_debug_read_stamps_xcd(unsigned long long *out8x32, int reset) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out8x32, HIP_SYMBOL(g_st_acc_xcd), 8 * 32 * sizeof(unsigned long long));
    if (reset) { static unsigned long long z[8 * 32]; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_st_acc_xcd), z, sizeof(z)); }
    return 0;
}
extern "C" int abr_debug_read_wg_times(unsigned long long *out, int n_wg) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wg_t), (size_t)n_wg * 10 * sizeof(unsigned long long));
    return 0;
}
#endif

#ifdef ABR_ASYNC_STATS
extern "C" int abr_debug_async_stats(unsigned long long *out48, int reset) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out48, HIP_SYMBOL(g_async_stats), 48 * sizeof(unsigned long long));
    if (reset) { unsigned long long z[48] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_async_stats), z, sizeof(z)); }
    return 0;
}
#endif

extern "C" int abr_env_get_state(abr_env *env, abr_env_state_view *v) {
    if (!env || !v) return fail(ABR_E_INVALID, "NULL argument");
    const EnvParams &p = env->p;
    v->n_lanes = p.n_lanes; v->chunk_id = p.chunk_id; v->last_bitrate = p.last_action;
    v->buffer_level = p.buf; v->hist_n = p.hist_n; v->hist_sum_inv = p.hist_s; v->done = p.done;
    v->action_hist = p.action_hist; v->bw_hist = p.bw_hist;
    return ABR_OK;
}

// ===========================================================================
// K3: MPC lookahead (mpc.py)
// ===========================================================================
struct MpcParams {
    int32_t B, H, V, clip;
    double L, max_buffer, wv, wr, ws;
    int64_t n_lanes;
    const int32_t *chunk, *prev;
    const double *buffer;
    double *hist_n, *hist_s;
    const double *br, *sz;
    // f4 (parity unpinned, see include/abr_env.h: abr_mpc_options)
    int32_t predictor;         // 0 harmonic (mpc.py:81-93), 1 exponential smoothing (mpc.py:72-79)
    int32_t utility;           // 0 identity (mpc.py:95-97), 1 log(bitrate / top bitrate) (mpc.py:99-102)
    const double *hist;        // predictor 1: previous_bandwidths, entry t of lane i at hist[t * hist_stride + i]
    int64_t hist_stride;
    const int32_t *hist_len;   // predictor 1: len(previous_bandwidths) per lane
    // phase 1 run ahead of the search kernel by mpc_predict_kernel (caller-provided scratch), or null
    const double *pre_pred;    // [H][n_lanes]
    const int32_t *pre_he, *pre_prev;
    double *pre_pred_w;        // the same arrays, writable, for mpc_predict_kernel
    int32_t *pre_he_w, *pre_prev_w;
    const uint8_t *mask;
    int32_t mask_is_done;      // mask[] holds ABR_DONE_* bits: a lane is active iff its byte is 0
    int32_t neg_to_zero;       // report "no decision" (-1: D13 / D12) as bitrate 0 in action_out
    int32_t careful_all;       // L, max_buffer or a weight is outside the fast path's range: every lane takes mpc_scan_careful
    int32_t *action_out, *flat_out;
    double *J_out;
};

__device__ inline double pymax0(double x) { return (x > 0.0) ? x : 0.0; }   // Python max(0, x)

// per-lane tables in LDS, [level][rate]:
//   brv[i][r] = bitrates[i][r]                      (chunk c+i's ladder, mpc.py:127-128)
//   rbt[i][r] = max(0, sizes[i][r], L) / C_hat[i]    (mpc.py:151-152, D10)
//   tdl[i][r] = sizes_of_CURRENT_chunk[r] / C_hat[i] (mpc.py:107,116 via :155-156, D11)
struct MpcLds {
    const double *brv, *rbt, *tdl;
    double L, max_buffer, wv, wr;
    int B, heff;
};

// Running best of one thread: x = -J (so the arg-min of J is the FIRST arg-max of x).
// idx is the flat index of the winning innermost GROUP (the B leaves that share their first
// H-1 digits) -- the winning leaf inside it is resolved once per lane at the end -- or, when
// a clipped horizon ends above the innermost level, of the winning leaf itself.
struct Best { double x; int32_t idx; double m; };    // m: the running maximum of the level-(H-2) node being enumerated

// Depth-first enumeration with prefix sharing: the partial sums of objective()
// (mpc.py:144-156) after level i depend only on R[0..i], and are formed in the
// same order as the reference forms them, so every leaf value is bit-identical
// to a from-scratch evaluation.  Leaves are visited in increasing flat index;
// strict `<` keeps the first minimum (numpy argmin on the raveled C-order grid).
//
// BC > 0: the number of rates is a compile-time constant: the two innermost
// levels are fully unrolled and the innermost level's tables (bl = bitrates,
// rl = max(0,size,L)/C_hat) live in registers instead of LDS.  BC == 0: generic.
// FULL: the lane's horizon is not clipped (heff == H), so no node below the prefix can be a
// leaf: the per-node `is this the clipped end?` test (and its exec-mask branch) disappears.
// WVM: how variance_weight enters a leaf (mpc.py:158): 0 = multiply; 1 = the weight is exactly
// 1.0, and x * 1.0 is x bit for bit, so the multiplication is dropped; 2 = the weight is
// exactly 0.0 (mpc_test.py's QOEMetric), 0.0 * v is +0.0 for the finite non-negative v that
// occur and q - 0.0 is q, so the whole variance term is dropped.
template <int LVL, int H, int BC, bool FULL, int WVM>
__device__ __forceinline__ void mpc_node(const MpcLds &t, const double *bl, const double *rl,
                                         int r, double q, double v, double rb, double buf,
                                         double br_prev, int pd, int32_t flat, Best &best);

template <int LVL, int H, int BC, bool FULL, int WVM>
__device__ __forceinline__ void mpc_dfs(const MpcLds &t, const double *bl, const double *rl,
                                        double q, double v, double rb, double buf,
                                        double br_prev, int pd, int32_t flat, Best &best) {
    // pd: the digit br_prev belongs to when the caller knows it at compile time (unrolled
    // levels), else -1.  The same digit one level down means |b - br_prev| is |b - b| = +0.0
    // and v + 0.0 is v (v >= +0.0): those two operations are skipped, bit for bit.
    const int B = BC ? BC : t.B;
    if constexpr (LVL == H - 1) {
        // innermost level: only the group maximum is tracked (v_max_f64 per leaf instead of
        // compare + three selects); ties inside the group are resolved by mpc_resolve_group
        double g = -INFINITY;
        if constexpr (BC > 0) {
#pragma unroll
            for (int r = 0; r < BC; r++) {
                const double b = bl[r];
                double a = q + b;                                                    // :146
                const double vv = (r == pd) ? v : v + fabs(b - br_prev);            // :148-149
                if (WVM == 0) a = a - t.wv * vv;                                     // :158
                if (WVM == 1) a = a - vv;
                const double x = a - t.wr * (rb + (rl[r] - buf));                    // :151-152,:159
                g = fmax(g, x);
            }
        } else {
#pragma unroll 1
            for (int r = 0; r < B; r++) {
                const double b = t.brv[LVL * B + r];
                const double x = ((q + b) - t.wv * (v + fabs(b - br_prev))) -
                                 t.wr * (rb + (t.rbt[LVL * B + r] - buf));
                g = fmax(g, x);
            }
        }
        // H >= 4: the B groups below one level-(H-2) node only feed that node's maximum (one v_max_f64
        // per group); the arg-max bookkeeping (compare, three selects, index) is paid once per NODE,
        // which is then named by its H-2 digits, and the first leaf below it that reaches the
        // lane's maximum is found afterwards (mpc_resolve_group, one thread per group)
        if constexpr (H >= 4) best.m = fmax(best.m, g);
        else if (g > best.x) { best.x = g; best.idx = flat; }
    } else {
        if constexpr (LVL == H - 2 && H >= 4) best.m = -INFINITY;
        if constexpr (BC > 0 && LVL >= H - 2) {
#pragma unroll
            for (int r = 0; r < BC; r++) mpc_node<LVL, H, BC, FULL, WVM>(t, bl, rl, r, q, v, rb, buf, br_prev, pd, flat, best);
        } else {
#pragma unroll 1
            for (int r = 0; r < B; r++) mpc_node<LVL, H, BC, FULL, WVM>(t, bl, rl, r, q, v, rb, buf, br_prev, pd, flat, best);
        }
        if constexpr (LVL == H - 2 && H >= 4) {
            if (best.m > best.x) { best.x = best.m; best.idx = flat; }
        }
    }
}

// inner node (LVL < H - 1)
template <int LVL, int H, int BC, bool FULL, int WVM>
__device__ __forceinline__ void mpc_node(const MpcLds &t, const double *bl, const double *rl,
                                         int r, double q, double v, double rb, double buf,
                                         double br_prev, int pd, int32_t flat, Best &best) {
    const int B = BC ? BC : t.B;
    const double b = t.brv[LVL * B + r];
    const double q2 = q + b;                                  // :146
    const double v2 = (r == pd) ? v : v + fabs(b - br_prev);  // :148-149
    const double rb2 = rb + (t.rbt[LVL * B + r] - buf);       // :151-152
    const int32_t f2 = flat * B + r;
    if (!FULL && LVL == t.heff - 1) {
        // a clipped horizon (D12) ends here: this node is a leaf
        const double x = (q2 - t.wv * v2) - t.wr * rb2;       // = -J, :158-162 (startup term is 0)
        if (x > best.x) { best.x = x; best.idx = f2; }
    } else {
        if constexpr (LVL + 1 < H) {
            const double tmp = pymax0(buf - t.tdl[LVL * B + r]);               // :107,:116
            const double wait = pymax0(tmp + t.L - t.max_buffer);              // :108-109
            const double nb = pymax0(tmp + t.L - wait);                        // :117
            // bitrates[LVL+1][R[LVL+1]] of the child's "previous" digit r (both from chunk LVL+1's ladder)
            const double bp = (LVL + 1 == H - 1 && BC > 0) ? bl[r] : t.brv[(LVL + 1) * B + r];
            // the child level sees this node's digit as its "previous" one; only worth telling
            // it when this level is unrolled (r is then a compile-time constant)
            mpc_dfs<LVL + 1, H, BC, FULL, WVM>(t, bl, rl, q2, v2, rb2, nb, bp,
                                               (BC > 0 && LVL >= H - 2) ? r : -1, f2, best);
        }
    }
}

// The first leaf of innermost group `gflat` whose x equals the lane's maximum `xbest`
// (INT32_MAX: none): re-walks the H-1 fixed digits with the same operation sequence as the
// search, then scans the B leaves in order.  Runs once per lane (H < 4) or once per group of
// the winning level-(H-2) node.
__device__ inline int32_t mpc_resolve_group(const MpcLds &t, int H, int32_t gflat, int prev0,
                                            double buf, double xbest) {
    const int B = t.B;
    int32_t pw = 1;
    for (int i = 0; i < H - 2; i++) pw *= B;
    double q = 0.0, v = 0.0, rb = 0.0;
    double bp = t.brv[prev0];
    for (int lvl = 0; lvl < H - 1; lvl++) {
        const int r = (gflat / pw) % B;
        pw = (pw >= B) ? pw / B : 1;
        const double b = t.brv[lvl * B + r];
        q = q + b; v = v + fabs(b - bp); rb = rb + (t.rbt[lvl * B + r] - buf);
        const double tmp = pymax0(buf - t.tdl[lvl * B + r]);
        const double wait = pymax0(tmp + t.L - t.max_buffer);
        buf = pymax0(tmp + t.L - wait);
        bp = t.brv[(lvl + 1) * B + r];
    }
    const int lvl = H - 1;
    for (int r = 0; r < B; r++) {
        const double b = t.brv[lvl * B + r];
        const double x = ((q + b) - t.wv * (v + fabs(b - bp))) - t.wr * (rb + (t.rbt[lvl * B + r] - buf));
        if (x == xbest) return gflat * B + r;
    }
    return 0x7fffffff;    // not in this group
}

// The search above keeps x = -J in registers with fmax and strict `>`: exact while every x is finite,
// but fmax drops a NaN and an all -inf lane never takes a winner.  It is used only where every value
// it forms is provably finite: each table entry and the buffer at most 2^960 in magnitude, L and
// max_buffer too, and each weight at most 2^40 (then no partial sum of the H <= 8 levels, nor a
// weighted one, exceeds 2^1010).  Every other lane takes this scan.
constexpr double kMpcFastEntryMax = 0x1p960;
constexpr double kMpcFastWeightMax = 0x1p40;
constexpr int kMpcCareful = 0x100;    // flag bit beside the effective horizon (heff_s) of a lane that takes the scan below

// The careful scan: thread `pre` of the lane's T evaluates its contiguous share of the B^heff
// combinations, each from scratch in objective()'s operation order (mpc.py:144-162, the startup
// term included), and keeps what numpy's argmin over the raveled grid keeps (scipy brute,
// finish=None): its first NaN, else its first maximum of x = -J (the first leaf is always taken,
// so an all -inf share has a winner).  best.idx is the leaf itself; phase 4 ranks a NaN above
// every number.
__device__ inline void mpc_scan_careful(const MpcLds &t, double ws, int prev0, double buf0, int pre, int T,
                                        Best &best) {
    const int B = t.B, he = t.heff;
    int32_t total = 1;
    for (int i = 0; i < he; i++) total *= B;                 // <= 2e9 (validate_mpc)
    const int32_t share = total / T + (total % T != 0);
    const int32_t f0 = (int32_t)min((int64_t)pre * share, (int64_t)total);
    const int32_t f1 = (int32_t)min((int64_t)f0 + share, (int64_t)total);
    for (int32_t f = f0; f < f1; f++) {
        int32_t pw = total / B;
        double q = 0.0, v = 0.0, rb = 0.0, buf = buf0;
        double bp = t.brv[prev0];
        for (int lvl = 0; lvl < he; lvl++) {
            const int r = (f / pw) % B;
            pw = (pw >= B) ? pw / B : 1;
            const double b = t.brv[lvl * B + r];
            q = q + b; v = v + fabs(b - bp); rb = rb + (t.rbt[lvl * B + r] - buf);
            if (lvl + 1 < he) {
                const double tmp = pymax0(buf - t.tdl[lvl * B + r]);
                const double wait = pymax0(tmp + t.L - t.max_buffer);
                buf = pymax0(tmp + t.L - wait);
                bp = t.brv[(lvl + 1) * B + r];
            }
        }
        const double x = ((q - t.wv * v) - t.wr * rb) - ws * 0.0;
        if (x != x) { best.x = x; best.idx = f; return; }
        if (best.idx == 0x7fffffff || x > best.x) { best.x = x; best.idx = f; }
    }
}

// Phase 1 of K3 for one lane: validates chunk / previous_bitrate, runs the throughput predictor
// (growing the caller's history, D9, in the harmonic branch) and writes the H predictions to
// pred[i * stride].  Returns the effective horizon (0 = no decision); prev_out = previous_bitrate
// as the index Python would use.
__device__ inline int mpc_predict_lane(const MpcParams &p, int64_t lane, int B, int H, double *pred,
                                       int64_t stride, int &prev_out) {
    double n = p.hist_n[lane], S = p.hist_s[lane];
    int c = p.chunk[lane];
    int he = H;
    if (c + H > p.V) he = p.clip ? (p.V - c) : 0;  // D12
    if (he < 0) he = 0;
    // R[0] = previous_bitrate indexes bitrates[i] (mpc.py:132,148): Python wraps -B..-1 to
    // the top of the ladder (the env's "no previous chunk" value -1 -> the highest rate) and
    // raises IndexError outside [-B, B)
    int pv = p.prev[lane];
    const bool prev_ok = (pv >= -B) && (pv < B);
    if (pv < 0) pv += B;
    prev_out = prev_ok ? pv : 0;
    if (p.predictor == 1) {
        // method="expsmoothing" (mpc.py:72-79): SimpleExpSmoothing(data).fit(0.5), then the
        // H out-of-sample forecasts -- all equal to the last smoothed level.  statsmodels is
        // not available to pin this against (PARITY UNPINNED); the rule implemented is the
        // documented one: smoothing level 0.5, initial level = the least-squares optimum of
        // the one-step-ahead errors (what fit()'s default `estimated` initialisation
        // approximates numerically), in closed form.  With l(t-1) = a + b*l0 the level before
        // observation y(t):  l0 = sum b (y - a) / sum b^2.  The history is NOT grown (the
        // reference's branch returns before the append of mpc.py:92).
        const int32_t hl = p.hist_len ? p.hist_len[lane] : 0;
        if (hl <= 0 || c < 0 || !prev_ok) return 0;
        double a = 0.0, b = 1.0, num = 0.0, den = 0.0;
        for (int32_t tt = 0; tt < hl; tt++) {
            const double y = p.hist[(int64_t)tt * p.hist_stride + lane];
            num = num + b * (y - a);
            den = den + b * b;
            a = 0.5 * y + 0.5 * a;
            b = 0.5 * b;
        }
        const double level = a + b * (num / den);
        if (!(level > 0.0)) return 0;
        for (int i = 0; i < H; i++) pred[(int64_t)i * stride] = level;
        return he;
    }
    if (!(n > 0.0) || !(S > 0.0) || c < 0 || !prev_ok) {
        // D13: empty / zero throughput history -- the reference raises ZeroDivisionError
        // (mpc.py:88,90); likewise an out-of-range previous_bitrate (IndexError).  Defined
        // here as "no decision": history untouched, action -1.
        return 0;
    }
    bool zero = false;
    for (int i = 0; i < H; i++) {
        double tp = n / S;            // history_size / sum_inverse  (:90)
        zero = zero || !(tp > 0.0);
        pred[(int64_t)i * stride] = tp;
        S = S + 1.0 / tp;             // throughput_values.append(tp): next pass sums it last
        n = n + 1.0;
    }
    // a zero prediction (S overflowed to inf): the reference divides by it -- 1/x of the appended value on
    // the next pass (:88) or size/bandwidth in objective() (:151) -- and raises ZeroDivisionError.  Defined
    // as for D13: no decision, history untouched.
    if (zero) return 0;
    p.hist_n[lane] = n; p.hist_s[lane] = S;    // D9: the caller's list has grown by H
    return he;
}

// Phase 1 for every lane ahead of the search kernel (one thread per lane): ten dependent IEEE
// divisions that would otherwise run on 1 of a lane's 36 threads while the other 35 wait.
__global__ void mpc_predict_kernel(MpcParams p) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= p.n_lanes) return;
    if (p.mask && ((p.mask[lane] != 0) == (p.mask_is_done != 0))) return;
    int pv;
    const int he = mpc_predict_lane(p, lane, p.B, p.H, p.pre_pred_w + lane, p.n_lanes, pv);
    p.pre_he_w[lane] = he; p.pre_prev_w[lane] = pv;
}

constexpr int kMpcLanesPerBlock = 16;

// Threads of a block: (lane-in-block, prefix) pairs.  D = number of leading
// levels fixed per thread (2 when H >= 3, else 1) -> T = B^D threads per lane.
template <int H, int BC, int WVM>
__global__ __launch_bounds__(256, 4)
void mpc_select_kernel(MpcParams p, int T, int D, int LPB) {
    extern __shared__ double lds[];
    const int B = BC ? BC : p.B;
    const int HB = H * B;
    // layout per lane-in-block: brv[HB] rbt[HB] tdl[HB] pred[H]
    const int per_lane = 3 * HB + H;
    double *tab = lds;
    __shared__ int32_t heff_s[16];    // effective horizon; phase 2 sets the kMpcCareful bit of a lane that takes mpc_scan_careful
    __shared__ int32_t prev_s[16];    // previous_bitrate as the index Python would use (mpc.py:132,148)
    __shared__ unsigned long long bestK[16];   // phase 4: the lane's maximum of x = -J as an ordered key
    __shared__ int32_t bestF[16];              //          and the smallest flat index that reaches it
    __shared__ int32_t bestL[16];              // phase 5 (H >= 4): the first leaf below the winning node that reaches it
    const int tid = threadIdx.x;
    const int li = tid / T;               // lane in block
    const int pre = tid - li * T;         // prefix id
    if (threadIdx.x < 16) { bestK[threadIdx.x] = 0; bestF[threadIdx.x] = 0x7fffffff; bestL[threadIdx.x] = 0x7fffffff; }
    const int64_t lane = (int64_t)blockIdx.x * LPB + li;
    const bool valid = (li < LPB) && (lane < p.n_lanes) &&
                       !(p.mask && ((p.mask[lane] != 0) == (p.mask_is_done != 0)));
    double *my = tab + (li < LPB ? li : 0) * per_lane;

    K3_STAMP_DECL
    // ---- phase 1: the predictor, one thread per lane (mpc.py:81-93 / :72-79) -- or its result, when
    //      mpc_predict_kernel already ran it for every lane (p.pre_pred != nullptr) ----
    if (valid && pre == 0) {
        if (p.pre_pred) {
            const int he = p.pre_he[lane];
            for (int i = 0; i < H; i++) my[3 * HB + i] = p.pre_pred[(int64_t)i * p.n_lanes + lane];
            prev_s[li] = p.pre_prev[lane];
            heff_s[li] = he;
        } else {
            int pv;
            heff_s[li] = mpc_predict_lane(p, lane, B, H, my + 3 * HB, 1, pv);
            prev_s[li] = pv;
        }
    }
    __syncthreads();
    K3_STAMP(26);
    // ---- phase 2: the per-(level, rate) tables, 60 divisions per lane spread over T threads ----
    if (valid) {
        const int c = p.chunk[lane];
        const int he = heff_s[li] & (kMpcCareful - 1);
        bool careful = p.careful_all || (pre == 0 && !(fabs(p.buffer[lane]) <= kMpcFastEntryMax));
        for (int e = pre; e < HB; e += T) {
            const int i = e / B, r = e - i * B;
            if (i < he) {
                const double pr = my[3 * HB + i];
                const double s_i = p.sz[(int64_t)(c + i) * B + r];
                double m = 0.0;
                if (s_i > m) m = s_i;
                if (p.L > m) m = p.L;                      // max(0, size, chunk_length)
                const double bre = p.br[(int64_t)(c + i) * B + r];
                // utility 1: log_bitrate_utility with the arity its call sites need (mpc.py:99-102,
                // :146-149): u = log(bitrate / top bitrate of that chunk).  PARITY UNPINNED.
                const double u = p.utility == 1 ? log(bre / p.br[(int64_t)(c + i) * B + (B - 1)]) : bre;
                const double rt = m / pr, td = p.sz[(int64_t)c * B + r] / pr;
                my[e] = u; my[HB + e] = rt; my[2 * HB + e] = td;
                careful |= !(fabs(u) <= kMpcFastEntryMax) | !(rt <= kMpcFastEntryMax) | !(fabs(td) <= kMpcFastEntryMax);
            }
        }
        // (every writer stores the same value; an LDS atomic here measured 3 % slower on the whole kernel)
        if (careful && he > 0) heff_s[li] = he | kMpcCareful;
    }
    __syncthreads();
    K3_STAMP(27);
    // ---- phase 3: each thread walks its prefix, then enumerates its subtree ----
    Best best; best.x = -INFINITY; best.idx = 0x7fffffff; best.m = -INFINITY;
    if (valid && heff_s[li] > kMpcCareful) {
        MpcLds t;
        t.brv = my; t.rbt = my + HB; t.tdl = my + 2 * HB;
        t.L = p.L; t.max_buffer = p.max_buffer; t.wv = p.wv; t.wr = p.wr; t.B = B;
        t.heff = heff_s[li] - kMpcCareful;
        mpc_scan_careful(t, p.ws, prev_s[li], p.buffer[lane], pre, T, best);
    } else if (valid && heff_s[li] > 0) {
        MpcLds t;
        t.brv = my; t.rbt = my + HB; t.tdl = my + 2 * HB;
        t.L = p.L; t.max_buffer = p.max_buffer; t.wv = p.wv; t.wr = p.wr; t.B = B;
        t.heff = heff_s[li];
        double q = 0.0, v = 0.0, rb = 0.0, buf = p.buffer[lane];
        int prev_r = prev_s[li];
        int32_t flat = 0;
        bool ok = true, is_leaf = false;
        // digits of the prefix, most significant first (two scalars, not an array: indexed by the loop variable an array went
        // to scratch -- the 12 B of private memory per lane of rounds 4-5, four scratch instructions per thread, here and not in
        // the enumeration)
        const int dig0 = (D == 2) ? pre / B : pre, dig1 = (D == 2) ? pre - dig0 * B : 0;
        for (int lvl = 0; lvl < D && ok && !is_leaf; lvl++) {
            const int r = lvl == 0 ? dig0 : dig1;
            const double *brv = t.brv + lvl * B;
            const double b = brv[r];
            const double bp = brv[prev_r];
            q = q + b; v = v + fabs(b - bp); rb = rb + (t.rbt[lvl * B + r] - buf);
            flat = flat * B + r;
            if (lvl == t.heff - 1) {
                // clipped horizon ends inside the prefix: only all-zero remainders are real combos
                if (lvl == 0 && D == 2 && dig1 != 0) ok = false;
                is_leaf = true;
            } else {
                const double tmp = pymax0(buf - t.tdl[lvl * B + r]);
                const double wait = pymax0(tmp + t.L - t.max_buffer);
                buf = pymax0(tmp + t.L - wait);
                prev_r = r;
            }
        }
        if (ok) {
            // innermost level's tables in registers (BC > 0)
            double bl[BC ? BC : 1], rl[BC ? BC : 1];
            if constexpr (BC > 0) {
#pragma unroll
                for (int r = 0; r < BC; r++) { bl[r] = t.brv[(H - 1) * B + r]; rl[r] = t.rbt[(H - 1) * B + r]; }
            }
            if (is_leaf) {
                best.x = (q - t.wv * v) - t.wr * rb; best.idx = flat;
            } else if (D == 2) {
                if constexpr (H >= 3) {
                    if (t.heff == H)
                        mpc_dfs<2, H, BC, true, WVM>(t, bl, rl, q, v, rb, buf, t.brv[2 * B + prev_r], -1, flat, best);
                    else    // clipped horizons (the last H-1 chunks of a video): compact generic code
                        mpc_dfs<2, H, 0, false, 0>(t, bl, rl, q, v, rb, buf, t.brv[2 * B + prev_r], -1, flat, best);
                }
            } else {
                if constexpr (H >= 2) {
                    if (t.heff == H)
                        mpc_dfs<1, H, BC, true, WVM>(t, bl, rl, q, v, rb, buf, t.brv[1 * B + prev_r], -1, flat, best);
                    else
                        mpc_dfs<1, H, 0, false, 0>(t, bl, rl, q, v, rb, buf, t.brv[1 * B + prev_r], -1, flat, best);
                }
            }
        }
    }
    K3_STAMP(28);
    // ---- phase 4: first arg-max of x = -J over the T prefixes of a lane (ascending prefix =
    //      ascending flat index); the winning leaf is found in phase 5.  Two LDS atomics
    //      and two barriers: the maximum of x as an order-preserving 64-bit key (ds_max_u64), then
    //      the smallest flat index among the threads that hold it (ds_min_i32) -- the same winner
    //      as a left-to-right scan with strict `>` (round 2 used a pairwise tree: six barriers).
    //      x + 0.0 folds -0.0 into +0.0 so that equal values have equal keys.  A NaN (only the careful
    //      scan keeps one) takes the largest key: numpy's argmin returns the first NaN. ----
    if (!valid && pre == 0 && li < LPB && lane < p.n_lanes && p.mask_is_done)
        p.action_out[lane] = -1;          // a finished lane of the fused rollout takes no decision
    unsigned long long key = 0;
    {
        const double xc = best.x + 0.0;
        const unsigned long long u = (unsigned long long)__double_as_longlong(xc);
        key = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
        if (!(xc == xc)) key = ~0ull;
        if (best.idx == 0x7fffffff) key = 0;
    }
    if (li < LPB && key) atomicMax(&bestK[li], key);
    __syncthreads();
    if (li < LPB && key && key == bestK[li]) atomicMin(&bestF[li], best.idx);
    __syncthreads();
    K3_STAMP(29);
    // ---- phase 5: the lanes' results, by the first threads of the block (with `pre == 0` every wave
    //      held one such thread and walked through the resolve; now the other waves skip it).
    //      H >= 4: bestF names the winning level-(H-2) node; thread (lane i, group r) looks through
    //      one of its B innermost groups for the first leaf that reaches the maximum. ----
    if (H >= 4) {
        if (tid < LPB * B) {
            const int l2 = tid / B, r = tid - l2 * B;
            const int64_t lane2 = (int64_t)blockIdx.x * LPB + l2;
            const unsigned long long bk = bestK[l2];
            const int32_t bf = bestF[l2];
            // (a masked or out-of-range lane has bk == 0: none of its threads entered a key)
            if (bk != 0 && bf != 0x7fffffff && heff_s[l2] == H) {     // (never a careful lane: its bestF is the leaf)
                const unsigned long long bu = (bk >> 63) ? (bk & 0x7fffffffffffffffull) : ~bk;
                const double *my2 = tab + l2 * per_lane;
                MpcLds t;
                t.brv = my2; t.rbt = my2 + HB; t.tdl = my2 + 2 * HB;
                t.L = p.L; t.max_buffer = p.max_buffer; t.wv = p.wv; t.wr = p.wr; t.B = B; t.heff = H;
                const int32_t first = mpc_resolve_group(t, H, bf * B + r, prev_s[l2], p.buffer[lane2],
                                                        __longlong_as_double((long long)bu));
                if (first != 0x7fffffff) atomicMin(&bestL[l2], first);
            }
        }
        __syncthreads();
    }
    if (tid < LPB) {
        const int l2 = tid;
        const int64_t lane2 = (int64_t)blockIdx.x * LPB + l2;
        const bool valid2 = (lane2 < p.n_lanes) && !(p.mask && ((p.mask[lane2] != 0) == (p.mask_is_done != 0)));
        if (valid2) {
            const unsigned long long bk = bestK[l2];
            const unsigned long long bu = (bk >> 63) ? (bk & 0x7fffffffffffffffull) : ~bk;
            const double bx = __longlong_as_double((long long)bu);
            int32_t bf = bestF[l2];
            const bool have = bk != 0 && bf != 0x7fffffff;
            const int he = heff_s[l2];
            int32_t act = -1;
            if (have) {
                if (he == H) {                      // (not a careful lane: its bestF is the leaf itself)
                    if (H >= 4) {
                        // always found: the maximum came out of this very arithmetic (else: the node's first leaf)
                        const int32_t fl = bestL[l2];
                        bf = (fl != 0x7fffffff) ? fl : bf * B * B;
                    } else {
                        const double *my2 = tab + l2 * per_lane;
                        MpcLds t;
                        t.brv = my2; t.rbt = my2 + HB; t.tdl = my2 + 2 * HB;
                        t.L = p.L; t.max_buffer = p.max_buffer; t.wv = p.wv; t.wr = p.wr; t.B = B; t.heff = he;
                        const int32_t fl = mpc_resolve_group(t, H, bf, prev_s[l2], p.buffer[lane2], bx);
                        bf = (fl != 0x7fffffff) ? fl : bf * B;
                    }
                }
                int32_t lead = 1;
                for (int i = 1; i < (he & (kMpcCareful - 1)); i++) lead *= B;
                act = bf / lead;                                   // int(result[0])  mpc.py:186
            }
            p.action_out[lane2] = (p.neg_to_zero && act < 0) ? 0 : act;
            if (p.flat_out) p.flat_out[lane2] = have ? bf : -1;
            if (p.J_out) p.J_out[lane2] = have ? -bx : NAN;
        }
    }
    K3_STAMP(30);
    K3_STAMP_FLUSH();
}

static int validate_mpc(const abr_mpc_config *c) {
    if (!c) return fail(ABR_E_INVALID, "mpc config is NULL");
    if (c->n_rates < 1 || c->n_rates > ABR_MAX_RATES)
        return fail(ABR_E_INVALID, "n_rates %d outside 1..%d", c->n_rates, ABR_MAX_RATES);
    if (c->horizon < 2 || c->horizon > ABR_MAX_HORIZON)
        return fail(ABR_E_INVALID, "horizon %d outside 2..%d", c->horizon, ABR_MAX_HORIZON);
    double combos = pow((double)c->n_rates, (double)c->horizon);
    if (combos > 2.0e9) return fail(ABR_E_UNSUPPORTED, "n_rates^horizon = %g exceeds int32", combos);
    if (c->video_length < 1) return fail(ABR_E_INVALID, "video_length must be >= 1");
    return ABR_OK;
}

template <int H, int BC, int WVM>
static void launch_mpc_b(const MpcParams &p, int T, int D, hipStream_t st) {
    // lanes per workgroup: as many as fit 256 threads (4 waves).  Measured on MI355X at B=6,H=5
    // (T=36): 7 lanes/WG 319 us, 16 lanes/WG (9 waves) 481 us, 3 lanes/WG 365 us per 65 536 lanes.
    int lpb = 256 / T;
    if (lpb > kMpcLanesPerBlock) lpb = kMpcLanesPerBlock;
    if (lpb < 1) lpb = 1;
    const int threads = ((lpb * T + 63) / 64) * 64;
    const size_t per_lane = (size_t)(3 * H * p.B + H) * sizeof(double);
    const size_t lds = lpb * per_lane;
    // (a persistent grid striding over the lane groups was measured and lost: -8 % at 1 024 workgroups,
    // -2 % at 2 048 -- the hardware's dynamic dispatch fills the tail better; profiles/r03_ab_mpc.txt)
    const unsigned grid = (unsigned)((p.n_lanes + lpb - 1) / lpb);
    hipLaunchKernelGGL((mpc_select_kernel<H, BC, WVM>), dim3(grid), dim3(threads), lds, st, p, T, D, lpb);
}

// compile-time rate count for the common ladders (6 and 4 rates with exact-weight variants; 3, 5, 7 and 8 rates) up to horizon 6
template <int H>
static void launch_mpc(const MpcParams &p, int T, int D, hipStream_t st) {
    if constexpr (H <= 6) {
        // exact-weight specialisations (see WVM above) for the six-rate ladder
        if (p.B == 6 && p.wv == 1.0) { launch_mpc_b<H, 6, 1>(p, T, D, st); return; }
        if (p.B == 6 && p.wv == 0.0) { launch_mpc_b<H, 6, 2>(p, T, D, st); return; }
        if (p.B == 6) { launch_mpc_b<H, 6, 0>(p, T, D, st); return; }
        if (p.B == 4 && p.wv == 0.0) { launch_mpc_b<H, 4, 2>(p, T, D, st); return; }
        if (p.B == 4) { launch_mpc_b<H, 4, 0>(p, T, D, st); return; }
#ifndef ABR_MPC_FEW_LADDERS
        // round 5: the other ladder sizes from 3 to 8 rates get the compile-time rate count too (the generic path
        // runs 30 - 40 % below the specialised one per combination: profiles/r05_mpc_other_shapes.txt)
        if (p.B == 5) { launch_mpc_b<H, 5, 0>(p, T, D, st); return; }
        if (p.B == 3) { launch_mpc_b<H, 3, 0>(p, T, D, st); return; }
        if (p.B == 8) { launch_mpc_b<H, 8, 0>(p, T, D, st); return; }
        if (p.B == 7) { launch_mpc_b<H, 7, 0>(p, T, D, st); return; }
#endif
    }
    launch_mpc_b<H, 0, 0>(p, T, D, st);
}

static size_t mpc_scratch_bytes(int H, int64_t n_lanes) {
    return (size_t)n_lanes * ((size_t)H * sizeof(double) + 2 * sizeof(int32_t));
}

static int apply_mpc_options(MpcParams &p, const abr_mpc_options *opt) {
    if (!opt) return ABR_OK;
    if (opt->predictor != ABR_PREDICT_HARMONIC && opt->predictor != ABR_PREDICT_EXPSMOOTHING)
        return fail(ABR_E_INVALID, "predictor must be ABR_PREDICT_HARMONIC or ABR_PREDICT_EXPSMOOTHING");
    if (opt->utility != ABR_UTILITY_IDENTITY && opt->utility != ABR_UTILITY_LOG)
        return fail(ABR_E_INVALID, "utility must be ABR_UTILITY_IDENTITY or ABR_UTILITY_LOG");
    if (opt->predictor == ABR_PREDICT_EXPSMOOTHING && (!opt->hist_dev || !opt->hist_len_dev || opt->hist_stride < 1))
        return fail(ABR_E_INVALID, "exponential smoothing needs the history itself: hist_dev, hist_stride, hist_len_dev");
    p.predictor = opt->predictor; p.utility = opt->utility;
    p.mask_is_done = opt->mask_is_done != 0;
    p.hist = opt->hist_dev; p.hist_stride = opt->hist_stride; p.hist_len = opt->hist_len_dev;
    if (opt->scratch_dev && opt->scratch_bytes < mpc_scratch_bytes(p.H, p.n_lanes))
        return fail(ABR_E_WORKSPACE, "MPC scratch has %zu bytes, need %zu", (size_t)opt->scratch_bytes,
                    mpc_scratch_bytes(p.H, p.n_lanes));
    if (opt->scratch_dev && ((uintptr_t)opt->scratch_dev & 7))
        return fail(ABR_E_WORKSPACE, "MPC scratch must be 8-byte aligned");
    return ABR_OK;
}

extern "C" int abr_mpc_scratch_bytes(const abr_mpc_config *cfg, int64_t n_lanes, size_t *bytes_out) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if (n_lanes < 1 || !bytes_out) return fail(ABR_E_INVALID, "n_lanes must be >= 1 and bytes_out non-NULL");
    *bytes_out = mpc_scratch_bytes(cfg->horizon, n_lanes);
    return ABR_OK;
}

// ===========================================================================
// RobustMPC (include/abr_env.h: abr_mpc_robust): the same search, fed by an error-discounted estimate
// ===========================================================================
// The robust predictor for every lane ahead of the unchanged search kernel (one thread per lane): updates the lane's
// state rows in place (abr_lane_jump.h: robust_estimate) and fills the pre_pred / pre_he / pre_prev scratch exactly as
// mpc_predict_kernel does -- H_eff 0 is "no decision", previous_bitrate normalised as Python indexes it.  The robust
// parameters are arguments of this kernel only; MpcParams and the search instances are untouched.
__global__ __launch_bounds__(256) void mpc_robust_predict_kernel(MpcParams p, int32_t window, uint8_t *__restrict__ state,
                                                                 const double *__restrict__ hist, int64_t hist_stride) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= p.n_lanes) return;
    if (p.mask && ((p.mask[lane] != 0) == (p.mask_is_done != 0))) return;
    const int64_t N = p.n_lanes;
    int32_t *cs1_row = (int32_t *)state, *cnt_row = cs1_row + N;
    double *ps_row = (double *)(state + 2 * sizeof(int32_t) * N), *err_rows = ps_row + N;
    int32_t cs1 = cs1_row[lane], cnt = cnt_row[lane];
    double ps = ps_row[lane];
    const int c = p.chunk[lane];
    const auto hf = [&](int32_t j) { return hist[(int64_t)j * hist_stride + lane]; };
    const auto ef = [&](int32_t k) -> double & { return err_rows[(int64_t)k * N + lane]; };
    const double P = abrx::robust_estimate(window, c, hf, cs1, cnt, ps, ef);
    cs1_row[lane] = cs1; cnt_row[lane] = cnt; ps_row[lane] = ps;
    // D12 and previous_bitrate as mpc_predict_lane
    int he = p.H;
    if (c + p.H > p.V) he = p.clip ? (p.V - c) : 0;
    if (he < 0) he = 0;
    int pv = p.prev[lane];
    const bool prev_ok = (pv >= -p.B) && (pv < p.B);
    if (pv < 0) pv += p.B;
    if (!(P > 0.0) || !prev_ok) he = 0;
    else
        for (int i = 0; i < p.H; i++) p.pre_pred_w[(int64_t)i * N + lane] = P;
    p.pre_he_w[lane] = he; p.pre_prev_w[lane] = prev_ok ? pv : 0;
}

static size_t robust_state_bytes(int32_t window, int64_t n_lanes) {
    return (size_t)n_lanes * (2 * sizeof(int32_t) + (size_t)(1 + window) * sizeof(double));
}

// the checks that need no lane count: window, utility, state pointer
static int validate_robust(const abr_mpc_robust *r) {
    if (!r) return fail(ABR_E_INVALID, "robust options are NULL");
    if (r->window < 1 || r->window > ABR_ROBUST_MAX_WINDOW)
        return fail(ABR_E_INVALID, "robust window %d outside 1..%d", r->window, ABR_ROBUST_MAX_WINDOW);
    if (r->utility != ABR_UTILITY_IDENTITY && r->utility != ABR_UTILITY_LOG)
        return fail(ABR_E_INVALID, "utility must be ABR_UTILITY_IDENTITY or ABR_UTILITY_LOG");
    if (!r->state_dev) return fail(ABR_E_INVALID, "robust state_dev is NULL");
    if ((uintptr_t)r->state_dev & 7) return fail(ABR_E_INVALID, "robust state must be 8-byte aligned");
    return ABR_OK;
}

// the checks against the lane count; scratch == NULL is accepted only when `scratch_optional`
static int validate_robust_sizes(const abr_mpc_robust *r, int H, int64_t n_lanes, bool scratch_optional) {
    if (r->state_bytes < robust_state_bytes(r->window, n_lanes))
        return fail(ABR_E_INVALID, "robust state has %zu bytes, need %zu", (size_t)r->state_bytes,
                    robust_state_bytes(r->window, n_lanes));
    if (!r->scratch_dev && scratch_optional) return ABR_OK;
    if (!r->scratch_dev) return fail(ABR_E_INVALID, "robust scratch_dev is NULL");
    if (r->scratch_bytes < mpc_scratch_bytes(H, n_lanes))
        return fail(ABR_E_INVALID, "robust scratch has %zu bytes, need %zu", (size_t)r->scratch_bytes,
                    mpc_scratch_bytes(H, n_lanes));
    if ((uintptr_t)r->scratch_dev & 7) return fail(ABR_E_INVALID, "robust scratch must be 8-byte aligned");
    return ABR_OK;
}

extern "C" int abr_mpc_robust_state_bytes(int32_t window, int64_t n_lanes, size_t *bytes_out) {
    if (window < 1 || window > ABR_ROBUST_MAX_WINDOW)
        return fail(ABR_E_INVALID, "robust window %d outside 1..%d", window, ABR_ROBUST_MAX_WINDOW);
    if (n_lanes < 1 || !bytes_out) return fail(ABR_E_INVALID, "n_lanes must be >= 1 and bytes_out non-NULL");
    *bytes_out = robust_state_bytes(window, n_lanes);
    return ABR_OK;
}

// ===========================================================================
// The host side of K3: the selects, and the rollouts that interleave them with K1
// ===========================================================================
// The search's parameters for n_lanes lanes: the config, the decision state (hist_n / hist_s: the harmonic history
// summary, NULL under the robust predictor, which reads the history itself), the tables, the lane mask and the outputs.
static MpcParams mpc_params(const abr_mpc_config *cfg, int64_t n_lanes, const int32_t *chunk, const int32_t *prev,
                            const double *buffer, double *hist_n, double *hist_s, const double *br, const double *sz,
                            const uint8_t *mask, int32_t *action_out, int32_t *flat_out, double *J_out) {
    MpcParams p;
    p.B = cfg->n_rates; p.H = cfg->horizon; p.V = cfg->video_length; p.clip = cfg->clip_horizon;
    p.L = cfg->chunk_length; p.max_buffer = cfg->max_buffer; p.wv = cfg->variance_weight;
    p.wr = cfg->rebuffer_weight; p.ws = cfg->startup_weight; p.n_lanes = n_lanes;
    p.mask_is_done = 0; p.neg_to_zero = 0;
    p.careful_all = !(fabs(p.L) <= kMpcFastEntryMax && fabs(p.max_buffer) <= kMpcFastEntryMax &&
                      fabs(p.wv) <= kMpcFastWeightMax && fabs(p.wr) <= kMpcFastWeightMax &&
                      fabs(p.ws) <= kMpcFastWeightMax);
    p.predictor = 0; p.utility = 0; p.hist = nullptr; p.hist_stride = 0; p.hist_len = nullptr;
    p.pre_pred = nullptr; p.pre_he = nullptr; p.pre_prev = nullptr;
    p.pre_pred_w = nullptr; p.pre_he_w = nullptr; p.pre_prev_w = nullptr;
    p.chunk = chunk; p.prev = prev; p.buffer = buffer; p.hist_n = hist_n; p.hist_s = hist_s; p.br = br; p.sz = sz;
    p.mask = mask; p.action_out = action_out; p.flat_out = flat_out; p.J_out = J_out;
    return p;
}

// The predictor, then the search.  scratch == nullptr: the search kernel predicts itself (harmonic or exponential
// smoothing); otherwise the predictor runs first as its own kernel into `scratch`: mpc_predict_kernel, or, with `robust`,
// mpc_robust_predict_kernel on the throughput history `hist` (row stride hist_stride).
static int launch_mpc_select(MpcParams p, hipStream_t st, void *scratch, const abr_mpc_robust *robust = nullptr,
                             const double *hist = nullptr, int64_t hist_stride = 0) {
    if (scratch) {
        p.pre_pred_w = (double *)scratch;
        p.pre_he_w = (int32_t *)(p.pre_pred_w + (size_t)p.H * p.n_lanes);
        p.pre_prev_w = p.pre_he_w + p.n_lanes;
        p.pre_pred = nullptr;                      // the predictor kernel itself must not read "pre"
        const dim3 grid((unsigned)((p.n_lanes + 255) / 256));
        if (robust)
            hipLaunchKernelGGL(mpc_robust_predict_kernel, grid, dim3(256), 0, st, p, robust->window,
                               (uint8_t *)robust->state_dev, hist, hist_stride);
        else
            hipLaunchKernelGGL(mpc_predict_kernel, grid, dim3(256), 0, st, p);
        p.pre_pred = p.pre_pred_w; p.pre_he = p.pre_he_w; p.pre_prev = p.pre_prev_w;
    }
    const int D = (p.H >= 3) ? 2 : 1;
    int T = p.B; if (D == 2) T *= p.B;
    switch (p.H) {
        case 2: launch_mpc<2>(p, T, D, st); break;
        case 3: launch_mpc<3>(p, T, D, st); break;
        case 4: launch_mpc<4>(p, T, D, st); break;
        case 5: launch_mpc<5>(p, T, D, st); break;
        case 6: launch_mpc<6>(p, T, D, st); break;
        case 7: launch_mpc<7>(p, T, D, st); break;
        case 8: launch_mpc<8>(p, T, D, st); break;
        default: return fail(ABR_E_INVALID, "horizon %d", p.H);
    }
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

extern "C" int abr_mpc_select_opt(const abr_mpc_config *cfg, const abr_mpc_options *opt,
                                  const int32_t *chunk_dev, const int32_t *prev_bitrate_dev,
                                  const double *buffer_dev, double *hist_n_dev,
                                  double *hist_sum_inv_dev, const double *br_table_dev,
                                  const double *sz_table_dev, const uint8_t *lane_mask_dev,
                                  int32_t *action_out_dev, int32_t *best_flat_out_dev,
                                  double *best_J_out_dev, int64_t n_lanes, void *stream) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if (!chunk_dev || !prev_bitrate_dev || !buffer_dev || !hist_n_dev || !hist_sum_inv_dev ||
        !br_table_dev || !sz_table_dev || !action_out_dev)
        return fail(ABR_E_INVALID, "NULL device pointer");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "n_lanes must be >= 1");
    MpcParams p = mpc_params(cfg, n_lanes, chunk_dev, prev_bitrate_dev, buffer_dev, hist_n_dev, hist_sum_inv_dev,
                             br_table_dev, sz_table_dev, lane_mask_dev, action_out_dev, best_flat_out_dev, best_J_out_dev);
    rc = apply_mpc_options(p, opt);
    if (rc) return rc;
    return launch_mpc_select(p, (hipStream_t)stream, opt ? opt->scratch_dev : nullptr);
}

extern "C" int abr_mpc_select(const abr_mpc_config *cfg, const int32_t *chunk_dev,
                              const int32_t *prev_bitrate_dev, const double *buffer_dev,
                              double *hist_n_dev, double *hist_sum_inv_dev,
                              const double *br_table_dev, const double *sz_table_dev,
                              const uint8_t *lane_mask_dev, int32_t *action_out_dev,
                              int32_t *best_flat_out_dev, double *best_J_out_dev, int64_t n_lanes,
                              void *stream) {
    return abr_mpc_select_opt(cfg, nullptr, chunk_dev, prev_bitrate_dev, buffer_dev, hist_n_dev, hist_sum_inv_dev,
                              br_table_dev, sz_table_dev, lane_mask_dev, action_out_dev, best_flat_out_dev,
                              best_J_out_dev, n_lanes, stream);
}

extern "C" int abr_mpc_select_robust(const abr_mpc_config *cfg, const abr_mpc_robust *robust,
                                     const int32_t *chunk_dev, const int32_t *prev_bitrate_dev,
                                     const double *buffer_dev, const double *br_table_dev,
                                     const double *sz_table_dev, const uint8_t *lane_mask_dev,
                                     int32_t *action_out_dev, int32_t *best_flat_out_dev, double *best_J_out_dev,
                                     int64_t n_lanes, void *stream) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if ((rc = validate_robust(robust))) return rc;
    if (!robust->hist_dev || robust->hist_stride < 1)
        return fail(ABR_E_INVALID, "the robust select needs the history: hist_dev and hist_stride >= 1");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "n_lanes must be >= 1");
    if ((rc = validate_robust_sizes(robust, cfg->horizon, n_lanes, false))) return rc;
    if (!chunk_dev || !prev_bitrate_dev || !buffer_dev || !br_table_dev || !sz_table_dev || !action_out_dev)
        return fail(ABR_E_INVALID, "NULL device pointer");
    MpcParams p = mpc_params(cfg, n_lanes, chunk_dev, prev_bitrate_dev, buffer_dev, nullptr, nullptr, br_table_dev,
                             sz_table_dev, lane_mask_dev, action_out_dev, best_flat_out_dev, best_J_out_dev);
    p.utility = robust->utility;
    p.mask_is_done = robust->mask_is_done != 0;
    return launch_mpc_select(p, (hipStream_t)stream, robust->scratch_dev, robust, robust->hist_dev, robust->hist_stride);
}

// The composition the reference leaves unwired (D5/D6), behind abr_env_step_mpc (robust == nullptr: the harmonic
// predictor on the workspace's scratch) and abr_env_step_mpc_robust, whose arguments have been checked up to the
// handle: for n_steps decisions, action = MPCBitrateController.next_bitrate() on the lane's own state (mpc.py:181-186
// reading chunk_number / previous_bitrate / buffer_level / previous_bandwidths straight from the environment's
// workspace, history mutation D9 included), then Simulator.run()'s download of that chunk (Simulator.py:155-170).
// Per decision the predictor, the search and K1 MODE 1, enqueued back to back on `st`: finished lanes are masked by
// their done bits and "no decision" (empty history at chunk 0, D13) downloads bitrate 0.
static int mpc_rollout(abr_env *env, const abr_mpc_config *cfg, const abr_mpc_robust *robust, const double *br_table_dev,
                       const double *sz_table_dev, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                       uint8_t *done_out_dev, int32_t *actions_out_dev, hipStream_t st) {
    const EnvParams &e = env->p;
    const int64_t N = e.n_lanes;
    if (cfg->n_rates != e.n_rates || cfg->video_length != e.video_length)
        return fail(ABR_E_INVALID, "MPC tables are [%d][%d], the environment has video_length %d, n_rates %d",
                    cfg->video_length, cfg->n_rates, e.video_length, e.n_rates);
    int rc;
    if (robust && (rc = validate_robust_sizes(robust, cfg->horizon, N, true))) return rc;
    MpcParams p = mpc_params(cfg, N, e.chunk_id, e.last_action, e.buf, robust ? nullptr : e.hist_n,
                             robust ? nullptr : e.hist_s, br_table_dev, sz_table_dev, e.done, nullptr, nullptr, nullptr);
    p.mask_is_done = 1; p.neg_to_zero = 1;
    if (robust) p.utility = robust->utility;
    void *scratch = robust && robust->scratch_dev ? robust->scratch_dev : env->mpc_scratch;
    return rollout_per_launch(env, kMpcRollout, n_steps, actions_out_dev, st, obs_out_dev, reward_out_dev, done_out_dev,
                              [&](int32_t, int32_t *action) {
        p.action_out = action;
        return launch_mpc_select(p, st, scratch, robust, e.bw_hist, N);
    });
}

extern "C" int abr_env_step_mpc(abr_env *env, const abr_mpc_config *cfg,
                                const double *br_table_dev, const double *sz_table_dev,
                                int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                                uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream) {
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if (!br_table_dev || !sz_table_dev) return fail(ABR_E_INVALID, "NULL device pointer");
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    return mpc_rollout(env, cfg, nullptr, br_table_dev, sz_table_dev, n_steps, obs_out_dev, reward_out_dev, done_out_dev,
                       actions_out_dev, (hipStream_t)stream);
}

// abr_env_step_mpc with the robust predictor (reading the lane's bw_hist rows): the options before the handle
extern "C" int abr_env_step_mpc_robust(abr_env *env, const abr_mpc_config *cfg, const abr_mpc_robust *robust,
                                       const double *br_table_dev, const double *sz_table_dev, int32_t n_steps,
                                       float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                       int32_t *actions_out_dev, void *stream) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if ((rc = validate_robust(robust))) return rc;
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (!br_table_dev || !sz_table_dev) return fail(ABR_E_INVALID, "NULL device pointer");
    return mpc_rollout(env, cfg, robust, br_table_dev, sz_table_dev, n_steps, obs_out_dev, reward_out_dev, done_out_dev,
                       actions_out_dev, (hipStream_t)stream);
}

// ===========================================================================
// Forecast MPC (include/abr_env.h: abr_plan_config): the lookahead's walk on a predicted bandwidth
// ===========================================================================
// The built-in forecast, one thread per lane: RobustMPC's estimate on the environment's own chunk_id and bw_hist rows
// (state != nullptr: the robust state, updated in place as mpc_robust_predict_kernel does; nullptr: no error is ever
// stored, P = hm).  Every lane's P is written, 0.0 for "no decision" and for a lane whose done bits are set.
__global__ __launch_bounds__(256) void plan_forecast_kernel(EnvParams p, int32_t window, uint8_t *__restrict__ state,
                                                            double *__restrict__ P_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_lanes) return;
    const auto hf = [&](int32_t j) { return p.bw_hist[(int64_t)j * p.n_lanes + i]; };
    // read by the planning kernel that follows: a plain store
    P_out[i] = abrx::plan_forecast(window, p.done[i] != 0, p.chunk_id[i], hf, state, p.n_lanes, i);
}

// lookahead_kernel with the cursor replaced at the root: lane i's trace is the one sample P[i].  A kernel of its own around
// the shared look_subtree, so that the lookahead's instances stay what they are (profiles/plan_isa_diff.txt).  A P that
// is not finite or not > 0 is "no decision"; forecast_out (nullable) receives the P the walk used, else 0.0.
template <int H, int W, bool SIZED>
__global__ __launch_bounds__(64 * look_waves(H, W)) void plan_kernel(
    EnvParams p, abrx::EpisodeQuality ql, int64_t lane0, int64_t lane_end, const double *__restrict__ P, int32_t neg_to_zero,
    int32_t *__restrict__ action_out, double *__restrict__ key_out, double *__restrict__ q_out,
    double *__restrict__ forecast_out) {
    __shared__ double s_q[look_waves(H, W)][64];
    const int32_t m = __builtin_amdgcn_readfirstlane((int32_t)(threadIdx.x >> 6));
    const int32_t l = (int32_t)(threadIdx.x & 63);
    const int64_t i = lane0 + (int64_t)blockIdx.x * 64 + l;
    const abrx::TablesChecked tb = make_tables<false, abrx::TablesChecked>(p);   // any handle: the checked chains
    LaneJ s{};
    int32_t n_su_obs = 0, n_rb_obs = 0;
    bool live = false;
    double f = 0.0;
    if (i < lane_end && p.done[i] == 0) {
        f = P[i];
        if (abrx::plan_usable(f)) {
            live = true;
            lanej_load<false>(s, p, i);
            abrx::plan_cursor(s.cur, P + i);
            n_su_obs = p.n_su_obs[i]; n_rb_obs = p.n_rb_obs[i];
        }
    }
    abrx::LookWeights w;
    w.wr = p.wr; w.ws = p.ws; w.wv = p.wv; w.wl = p.wl; w.M = p.n_rates; w.quality = ql.base != nullptr;
    const auto br = [&](int32_t chunk, int32_t rate) { return chunk_bitrate(p, chunk, rate); };
    // the step's target: the size table's entry (abr_env_set_size_table), else rate x chunk_length
    const auto sz = [&](int32_t chunk, int32_t a, double rate) {
        if constexpr (SIZED) return p.sz_table[(int64_t)chunk * p.n_rates + a];
        else return rate * tb.L;
    };
    const auto G = [&](int32_t n) { return p.G[n]; };
    const auto lat = [&](const LaneJ &x) { return lane_avg_latency(p, x.sumk, x.n_play); };
    const auto qt = [&](int32_t chunk, int32_t rate) { return abrx::quality_peek(ql, p.n_rates, chunk, rate); };
    const auto any = [](bool fl) { return __any(fl) != 0; };
    const double q = abrx::look_subtree<H>(w, tb, br, sz, G, lat, qt, any, s, live, n_rb_obs, n_su_obs, m);
    s_q[m][l] = q;
    if (q_out && i < lane_end) ABR_OUT(q_out[(int64_t)m * p.n_lanes + i], q);
    __syncthreads();
    if (m == 0 && i < lane_end) {
        int32_t action;
        double key;
        abrx::look_pick([&](int32_t r) { return s_q[r][l]; }, p.n_rates, action, key);
        ABR_OUT(action_out[i], (neg_to_zero && action < 0) ? 0 : action);
        if (key_out) ABR_OUT(key_out[i], key);
        if (forecast_out) ABR_OUT(forecast_out[i], live ? f : 0.0);
    }
}

template <bool SIZED>
struct PlanKernels { template <int H, int W> static constexpr auto kernel = plan_kernel<H, W, SIZED>; };

struct PlanOut {
    int32_t *action;
    double *key, *q, *forecast;
    int32_t neg_to_zero;
};

// One decision of every lane: the built-in forecast into `scratch` (skipped when the caller brought one), then the walk.
static int plan_decide(const abr_env *env, const abr_plan_config *cfg, double *scratch, PlanOut o, hipStream_t st) {
    const EnvParams &p = env->p;
    const double *P = cfg->forecast_dev;
    if (!P) {
        hipLaunchKernelGGL(plan_forecast_kernel, dim3((unsigned)((p.n_lanes + 255) / 256)), dim3(256), 0, st, p, cfg->window,
                           cfg->robust ? (uint8_t *)cfg->state_dev : nullptr, scratch);
        P = scratch;
        if (o.forecast == scratch) o.forecast = nullptr;     // the forecast kernel has written the caller's copy already
    }
    if (env->p.sz_table)
        return launch_walks<PlanKernels<true>>(env, cfg->horizon, cfg->max_nodes_per_launch, st, P, o.neg_to_zero, o.action,
                                               o.key, o.q, o.forecast);
    return launch_walks<PlanKernels<false>>(env, cfg->horizon, cfg->max_nodes_per_launch, st, P, o.neg_to_zero, o.action, o.key,
                                            o.q, o.forecast);
}

// The refusals of both entry points in the documented order; `select`: abr_env_plan_select (else abr_env_step_plan).
static int validate_plan(const abr_env *env, const abr_plan_config *cfg, bool select, const void *action_out,
                         int32_t n_steps) {
    if (const int rc = validate_walk(cfg, select, action_out, "plan")) return rc;
    if (cfg->robust != 0 && cfg->robust != 1) return fail(ABR_E_INVALID, "plan: robust must be 0 or 1, got %d", cfg->robust);
    if (!cfg->forecast_dev && (cfg->window < 1 || cfg->window > ABR_ROBUST_MAX_WINDOW))
        return fail(ABR_E_INVALID, "plan: window %d outside 1..%d", cfg->window, ABR_ROBUST_MAX_WINDOW);
    if (!select && n_steps < 1) return fail(ABR_E_INVALID, "plan: n_steps must be >= 1");
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if (cfg->robust == 1 && !cfg->forecast_dev) {
        if (!cfg->state_dev) return fail(ABR_E_INVALID, "plan: robust state_dev is NULL");
        if ((uintptr_t)cfg->state_dev & 7) return fail(ABR_E_INVALID, "plan: robust state must be 8-byte aligned");
        if (cfg->state_bytes < robust_state_bytes(cfg->window, env->p.n_lanes))
            return fail(ABR_E_INVALID, "plan: robust state has %zu bytes, need %zu", (size_t)cfg->state_bytes,
                        robust_state_bytes(cfg->window, env->p.n_lanes));
    }
    return look_supported(env, cfg->horizon, "plan");
}

extern "C" int abr_env_plan_select(abr_env *env, const abr_plan_config *cfg, int32_t *action_out_dev, double *key_out_dev,
                                   double *q_out_dev, double *forecast_out_dev, void *stream) {
    if (const int rc = validate_plan(env, cfg, true, action_out_dev, 1)) return rc;
    // the forecast's n_lanes doubles: the caller's output; the workspace's MPC scratch only when there is none
    double *scratch = forecast_out_dev ? forecast_out_dev : (double *)env->mpc_scratch;
    return plan_decide(env, cfg, scratch, PlanOut{action_out_dev, key_out_dev, q_out_dev, forecast_out_dev, 0},
                       (hipStream_t)stream);
}

extern "C" int abr_env_step_plan(abr_env *env, const abr_plan_config *cfg, int32_t n_steps, float *obs_out_dev,
                                 float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream) {
    if (const int rc = validate_plan(env, cfg, false, nullptr, n_steps)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    return rollout_per_launch(env, kMpcRollout, n_steps, actions_out_dev, st, obs_out_dev, reward_out_dev, done_out_dev,
                              [&](int32_t, int32_t *action) {
        return plan_decide(env, cfg, (double *)env->mpc_scratch, PlanOut{action, nullptr, nullptr, nullptr, 1}, st);
    });
}

// ===========================================================================
// FastMPC (include/abr_env.h: abr_fastmpc): the search over a quantised state space, then a lookup per decision
// ===========================================================================
// The build: per slice of grid entries, fastmpc_grid_kernel writes each entry's chunk / previous bitrate / buffer and the
// pre_pred / pre_he / pre_prev scratch exactly as mpc_robust_predict_kernel does, the unchanged mpc_select_kernel
// instances search it (launch_mpc_select without a predictor), and fastmpc_pack_kernel stores the first actions as uint8.
// The grids reach the device as kernel arguments (fastmpc_copy_kernel): no host copy, nothing synchronises.
constexpr int64_t kFastMpcSlice = 131072;      // grid entries per slice: bounds the scratch (~9 MB at H = 5)
constexpr int kFastMpcCopy = 128;              // doubles per fastmpc_copy_kernel launch

struct FastMpcCopy {
    int32_t n;
    double v[kFastMpcCopy];
};

__global__ __launch_bounds__(kFastMpcCopy) void fastmpc_copy_kernel(double *__restrict__ dst, FastMpcCopy a) {
    const int k = threadIdx.x;
    if (k < a.n) dst[k] = a.v[k];
}

// entries [first, first + p.n_lanes) of the table; lane = entry - first
__global__ __launch_bounds__(256) void fastmpc_grid_kernel(MpcParams p, int64_t first, int32_t uniform, int32_t nb,
                                                           int32_t nq, const double *__restrict__ bp,
                                                           const double *__restrict__ tp, int32_t *__restrict__ chunk_w,
                                                           int32_t *__restrict__ prev_w, double *__restrict__ buf_w) {
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= p.n_lanes) return;
    const int64_t N = p.n_lanes;
    int64_t e = first + lane;
    const int32_t qi = (int32_t)(e % nq); e /= nq;
    const int32_t bi = (int32_t)(e % nb); e /= nb;
    const int32_t pv = (int32_t)(e % p.B);
    const int32_t row = (int32_t)(e / p.B);
    const int32_t c = uniform ? p.V - 1 - row : row;           // 0 <= c < V: the host checked the layout
    chunk_w[lane] = c; prev_w[lane] = pv; buf_w[lane] = bp[bi];
    // D12 as mpc_predict_lane; the previous bitrate is a valid index and the prediction > 0 by construction
    int he = p.H;
    if (c + p.H > p.V) he = p.clip ? (p.V - c) : 0;
    const double P = tp[qi];
    for (int i = 0; i < p.H; i++) p.pre_pred_w[(int64_t)i * N + lane] = P;
    p.pre_he_w[lane] = he; p.pre_prev_w[lane] = pv;
}

// "no decision" (-1) is stored as 0: what abr_env_step_mpc downloads for it
__global__ __launch_bounds__(256) void fastmpc_pack_kernel(const int32_t *__restrict__ act, uint8_t *__restrict__ table,
                                                           int64_t first, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t a = act[i];
    table[first + i] = (uint8_t)(a < 0 ? 0 : a);
}

// the standalone lookup: one thread per player
__global__ __launch_bounds__(256) void fastmpc_select_kernel(abrx::RuleParams r, int32_t M, int32_t V,
                                                             const int32_t *__restrict__ chunk,
                                                             const int32_t *__restrict__ prev,
                                                             const double *__restrict__ buffer,
                                                             const double *__restrict__ hist, int64_t hist_stride,
                                                             const uint8_t *__restrict__ mask, int32_t mask_is_done,
                                                             int32_t *__restrict__ action_out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && ((mask[i] != 0) == (mask_is_done != 0))) {
        if (mask_is_done) action_out[i] = -1;
        return;
    }
    const auto hf = [&](int32_t j) { return hist[(int64_t)j * hist_stride + i]; };
    action_out[i] = abrx::fastmpc_lookup(r, hf, M, V, chunk[i], prev[i], buffer[i]);
}

// one grid: count, finiteness, order, the points' sign, and every point in its own cell
static int validate_fastmpc_grid(const char *what, int32_t n, const double *pt, const double *ed, bool positive) {
    if (n < 1 || n > ABR_FASTMPC_MAX_POINTS)
        return fail(ABR_E_INVALID, "%s grid has %d points, allowed 1..%d", what, n, ABR_FASTMPC_MAX_POINTS);
    if (!pt) return fail(ABR_E_INVALID, "%s points are NULL", what);
    if (n > 1 && !ed) return fail(ABR_E_INVALID, "%s edges are NULL", what);
    for (int32_t k = 0; k < n; k++) {
        if (!std::isfinite(pt[k])) return fail(ABR_E_INVALID, "%s point %d is not finite", what, k);
        if (k > 0 && !(pt[k] > pt[k - 1])) return fail(ABR_E_INVALID, "%s points are not strictly ascending at %d", what, k);
    }
    if (positive ? !(pt[0] > 0.0) : !(pt[0] >= 0.0))
        return fail(ABR_E_INVALID, "%s points must be %s (got %g)", what, positive ? "> 0" : ">= 0", pt[0]);
    for (int32_t k = 0; k + 1 < n; k++) {
        if (!std::isfinite(ed[k])) return fail(ABR_E_INVALID, "%s edge %d is not finite", what, k);
        if (k > 0 && !(ed[k] > ed[k - 1])) return fail(ABR_E_INVALID, "%s edges are not strictly ascending at %d", what, k);
    }
    for (int32_t k = 0; k < n; k++) {
        const bool lo_ok = k == 0 || ed[k - 1] <= pt[k], hi_ok = k + 1 == n || pt[k] < ed[k];
        if (!lo_ok || !hi_ok) return fail(ABR_E_INVALID, "%s point %d (%g) lies outside its cell", what, k, pt[k]);
    }
    return ABR_OK;
}

// the options every entry point checks: window, utility, layout, grid counts; `grids`: the points and edges too
static int validate_fastmpc(const abr_mpc_config *cfg, const abr_fastmpc *fm, bool grids) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if (!fm) return fail(ABR_E_INVALID, "fastmpc options are NULL");
    if (fm->window < 1 || fm->window > ABR_ROBUST_MAX_WINDOW)
        return fail(ABR_E_INVALID, "fastmpc window %d outside 1..%d", fm->window, ABR_ROBUST_MAX_WINDOW);
    if (fm->utility != ABR_UTILITY_IDENTITY && fm->utility != ABR_UTILITY_LOG)
        return fail(ABR_E_INVALID, "utility must be ABR_UTILITY_IDENTITY or ABR_UTILITY_LOG");
    if (fm->n_rows != cfg->video_length && fm->n_rows != cfg->horizon)
        return fail(ABR_E_INVALID, "fastmpc n_rows %d is neither video_length %d nor horizon %d", fm->n_rows,
                    cfg->video_length, cfg->horizon);
    if (fm->n_rows != cfg->video_length && cfg->horizon > cfg->video_length)
        return fail(ABR_E_INVALID, "the uniform layout (n_rows = horizon %d) needs horizon < video_length %d",
                    cfg->horizon, cfg->video_length);
    for (int32_t n : {fm->n_buffer, fm->n_tput})
        if (n < 1 || n > ABR_FASTMPC_MAX_POINTS)
            return fail(ABR_E_INVALID, "fastmpc grid has %d points, allowed 1..%d", n, ABR_FASTMPC_MAX_POINTS);
    if (!grids) return ABR_OK;
    if ((rc = validate_fastmpc_grid("buffer", fm->n_buffer, fm->buffer_points, fm->buffer_edges, false))) return rc;
    return validate_fastmpc_grid("throughput", fm->n_tput, fm->tput_points, fm->tput_edges, true);
}

static int64_t fastmpc_entries(const abr_mpc_config *cfg, const abr_fastmpc *fm) {
    return (int64_t)fm->n_rows * cfg->n_rates * fm->n_buffer * fm->n_tput;
}
static size_t fastmpc_table_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm) {
    return (size_t)abrx::fastmpc_entry_bytes(fm->n_rows, cfg->n_rates, fm->n_buffer, fm->n_tput) +
           (size_t)(fm->n_buffer - 1 + fm->n_tput - 1) * sizeof(double);
}
// the grid points, then per slice: pre_pred [H][S] and buffer [S] float64, pre_he, pre_prev, chunk, prev, action [S] int32
static int64_t fastmpc_slice(const abr_mpc_config *cfg, const abr_fastmpc *fm) {
    const int64_t n = fastmpc_entries(cfg, fm);
    return n < kFastMpcSlice ? n : kFastMpcSlice;
}
static size_t fastmpc_scratch_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm) {
    return (size_t)(fm->n_buffer + fm->n_tput) * sizeof(double) +
           (size_t)fastmpc_slice(cfg, fm) * ((size_t)(cfg->horizon + 1) * sizeof(double) + 5 * sizeof(int32_t));
}

extern "C" int abr_fastmpc_table_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm, size_t *bytes_out) {
    int rc = validate_fastmpc(cfg, fm, true);
    if (rc) return rc;
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    *bytes_out = fastmpc_table_bytes(cfg, fm);
    return ABR_OK;
}

extern "C" int abr_fastmpc_build_scratch_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm, size_t *bytes_out) {
    int rc = validate_fastmpc(cfg, fm, true);
    if (rc) return rc;
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    *bytes_out = fastmpc_scratch_bytes(cfg, fm);
    return ABR_OK;
}

static int fastmpc_table_check(const void *table_dev) {
    if (!table_dev || ((uintptr_t)table_dev & 7)) return fail(ABR_E_INVALID, "fastmpc table must be non-NULL and 8-byte aligned");
    return ABR_OK;
}

// host array -> device, in kernel-argument slices on `st`
static void fastmpc_copy(double *dst, const double *src, int32_t n, hipStream_t st) {
    for (int32_t k0 = 0; k0 < n; k0 += kFastMpcCopy) {
        FastMpcCopy a;
        a.n = n - k0 < kFastMpcCopy ? n - k0 : kFastMpcCopy;
        for (int32_t k = 0; k < a.n; k++) a.v[k] = src[k0 + k];
        hipLaunchKernelGGL(fastmpc_copy_kernel, dim3(1), dim3(kFastMpcCopy), 0, st, dst + k0, a);
    }
}

extern "C" int abr_fastmpc_build(const abr_mpc_config *cfg, const abr_fastmpc *fm, const double *br_table_dev,
                                 const double *sz_table_dev, void *table_dev, size_t table_bytes, void *scratch_dev,
                                 size_t scratch_bytes, void *stream) {
    int rc = validate_fastmpc(cfg, fm, true);
    if (rc) return rc;
    if ((rc = fastmpc_table_check(table_dev))) return rc;
    if (table_bytes < fastmpc_table_bytes(cfg, fm))
        return fail(ABR_E_INVALID, "fastmpc table has %zu bytes, need %zu", table_bytes, fastmpc_table_bytes(cfg, fm));
    if (!scratch_dev || ((uintptr_t)scratch_dev & 7))
        return fail(ABR_E_INVALID, "fastmpc scratch must be non-NULL and 8-byte aligned");
    if (scratch_bytes < fastmpc_scratch_bytes(cfg, fm))
        return fail(ABR_E_INVALID, "fastmpc scratch has %zu bytes, need %zu", scratch_bytes, fastmpc_scratch_bytes(cfg, fm));
    if (!br_table_dev || !sz_table_dev) return fail(ABR_E_INVALID, "NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int32_t M = cfg->n_rates, nb = fm->n_buffer, nq = fm->n_tput, H = cfg->horizon;
    const int32_t uniform = fm->n_rows != cfg->video_length;
    uint8_t *table = (uint8_t *)table_dev;
    double *be = (double *)(table + abrx::fastmpc_entry_bytes(fm->n_rows, M, nb, nq)), *te = be + (nb - 1);
    fastmpc_copy(be, fm->buffer_edges, nb - 1, st);
    fastmpc_copy(te, fm->tput_edges, nq - 1, st);
    double *bp = (double *)scratch_dev, *tp = bp + nb;
    fastmpc_copy(bp, fm->buffer_points, nb, st);
    fastmpc_copy(tp, fm->tput_points, nq, st);
    HIP_TRY(hipGetLastError());
    const int64_t S = fastmpc_slice(cfg, fm), total = fastmpc_entries(cfg, fm);
    double *pre_pred = tp + nq, *buf = pre_pred + (size_t)H * S;
    int32_t *pre_he = (int32_t *)(buf + S), *pre_prev = pre_he + S, *chunk = pre_prev + S, *prev = chunk + S,
            *act = prev + S;
    for (int64_t first = 0; first < total; first += S) {
        const int64_t n = total - first < S ? total - first : S;
        MpcParams p = mpc_params(cfg, n, chunk, prev, buf, nullptr, nullptr, br_table_dev, sz_table_dev, nullptr, act,
                                 nullptr, nullptr);
        p.utility = fm->utility;
        p.pre_pred_w = pre_pred; p.pre_he_w = pre_he; p.pre_prev_w = pre_prev;
        const dim3 grid((unsigned)((n + 255) / 256));
        hipLaunchKernelGGL(fastmpc_grid_kernel, grid, dim3(256), 0, st, p, first, uniform, nb, nq, bp, tp, chunk, prev,
                           buf);
        p.pre_pred = pre_pred; p.pre_he = pre_he; p.pre_prev = pre_prev;
        if ((rc = launch_mpc_select(p, st, nullptr))) return rc;
        hipLaunchKernelGGL(fastmpc_pack_kernel, grid, dim3(256), 0, st, act, table, first, n);
        HIP_TRY(hipGetLastError());
    }
    return ABR_OK;
}

static abrx::RuleParams fastmpc_rule(const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev) {
    abrx::RuleParams r{};
    r.kind = abrx::kRuleFastMpc; r.window = fm->window;
    r.fm_table = (const uint8_t *)table_dev;
    r.fm_uniform = fm->n_rows != cfg->video_length;
    r.fm_horizon = cfg->horizon; r.fm_nb = fm->n_buffer; r.fm_nq = fm->n_tput;
    return r;
}

extern "C" int abr_fastmpc_select(const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev,
                                  size_t table_bytes, const int32_t *chunk_dev, const int32_t *prev_bitrate_dev,
                                  const double *buffer_dev, const double *hist_dev, int64_t hist_stride,
                                  const uint8_t *lane_mask_dev, int32_t mask_is_done, int32_t *action_out_dev,
                                  int64_t n_lanes, void *stream) {
    int rc = validate_fastmpc(cfg, fm, false);
    if (rc) return rc;
    if ((rc = fastmpc_table_check(table_dev))) return rc;
    if (table_bytes < fastmpc_table_bytes(cfg, fm))
        return fail(ABR_E_INVALID, "fastmpc table has %zu bytes, need %zu", table_bytes, fastmpc_table_bytes(cfg, fm));
    if (!hist_dev || hist_stride < 1) return fail(ABR_E_INVALID, "the lookup needs the history: hist_dev and hist_stride >= 1");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "n_lanes must be >= 1");
    if (!chunk_dev || !prev_bitrate_dev || !buffer_dev || !action_out_dev) return fail(ABR_E_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(fastmpc_select_kernel, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fastmpc_rule(cfg, fm, table_dev), cfg->n_rates, cfg->video_length, chunk_dev, prev_bitrate_dev,
                       buffer_dev, hist_dev, hist_stride, lane_mask_dev, mask_is_done, action_out_dev, n_lanes);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// the env entry points' checks after the handle: the tables' shape, the layout against a per-chunk bitrate table
static int fastmpc_env_check(const abr_env *env, const abr_mpc_config *cfg, const abr_fastmpc *fm) {
    if (cfg->n_rates != env->p.n_rates || cfg->video_length != env->p.video_length)
        return fail(ABR_E_INVALID, "the FastMPC table is for video_length %d, n_rates %d; the environment has %d, %d",
                    cfg->video_length, cfg->n_rates, env->p.video_length, env->p.n_rates);
    const bool per_chunk = env->br_table_dirty ? env->pending_br_table != nullptr : env->p.br_table != nullptr;
    if (fm->n_rows != cfg->video_length && per_chunk)
        return fail(ABR_E_INVALID, "the uniform FastMPC layout needs one ladder, but a per-chunk bitrate table is in force");
    return ABR_OK;
}

extern "C" int abr_env_step_fastmpc(abr_env *env, const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev,
                                    int32_t n_steps, float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                    int32_t *actions_out_dev, void *stream) {
    int rc = validate_fastmpc(cfg, fm, false);
    if (rc) return rc;
    if ((rc = fastmpc_table_check(table_dev))) return rc;
    if (n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    if (!env) return fail(ABR_E_INVALID, "env is NULL");
    if ((rc = fastmpc_env_check(env, cfg, fm))) return rc;
    if ((rc = require(kRuleRollout, env->impl))) return rc;
    return launch_env<4>(env, launch_impl<4>(env, n_steps), (hipStream_t)stream, nullptr, obs_out_dev, reward_out_dev,
                         done_out_dev, actions_out_dev, n_steps, 0ull, fastmpc_rule(cfg, fm, table_dev));
}

extern "C" int abr_env_fastmpc_select(abr_env *env, const abr_mpc_config *cfg, const abr_fastmpc *fm,
                                      const void *table_dev, int32_t *action_out_dev, void *stream) {
    int rc = validate_fastmpc(cfg, fm, false);
    if (rc) return rc;
    if ((rc = fastmpc_table_check(table_dev))) return rc;
    if (!env || !action_out_dev) return fail(ABR_E_INVALID, "NULL argument (env or action_out_dev)");
    if ((rc = fastmpc_env_check(env, cfg, fm))) return rc;
    return launch_rule_select(env, fastmpc_rule(cfg, fm, table_dev), action_out_dev, stream);
}

// ===========================================================================
// Learned policy (include/abr_env.h: abr_policy): an MLP forward pass per lane, then K1 MODE 1 (as mpc_rollout)
// ===========================================================================
// One thread per lane, 256 per workgroup.  The weights are the same for every lane: the workgroup stages them in LDS once,
// in the padded layout of abr_lane_jump.h (policy_layout: at most 30 272 B), and every read of a weight is then a
// wave-uniform broadcast of a fixed-length row.  The
// arithmetic is abr_lane_jump.h's (policy_features, policy_forward, policy_explore), which tests/native compiles for the host.
constexpr int kPolicyBlock = 256;

struct PolicyArgs {
    abrx::PolicyNet net;
    const float *weights;
    int32_t *action_out;              // [N]
    float *features_out, *scores_out; // [F][N], [M][N], nullable
    float *probs_out;                 // [M][N], nullable (SAMPLED instance only)
    int32_t mode;                     // abr_policy_sampling (SAMPLED instance only)
    float inv_temperature;
};

// the VALUE instances' arguments (abr_policy_value): PolicyArgs itself stays what the other instances were compiled for
struct PolicyValueArgs : PolicyArgs {
    const float *head;                // [in + 1]: Wv then bv
    float *value_out;                 // [N], nullable
};

// the POP instances' arguments (abr_policy_pop): the member stride of the blob and of the heads, in floats
struct PolicyPopArgs : PolicyValueArgs {
    int32_t group, blob_words, head_words;
};

static_assert(sizeof(EnvParams) + sizeof(PolicyArgs) == 984 && sizeof(EnvParams) + sizeof(PolicyValueArgs) == 1000 &&
              sizeof(EnvParams) + sizeof(PolicyPopArgs) == 1016, "policy_select_kernel's kernarg segments");

// SAMPLED: the instance behind abr_env_policy_select_sampled.  It keeps each lane's scores in its own column of LDS past
// the weights (M * kPolicyBlock floats; the score loops run to a runtime M), where the draw turns them into e_m.
// VALUE: the instances behind the _ac entries.  The value head is one more row of the staged layout and one more fmaf
// chain of the forward pass; with a NULL action_out the launch stores no decision: a value evaluation only.
// POP: the instances behind the _pop entries (abr_policy_pop).  The workgroup computes the member it serves once, from its
// first lane, and offsets the blob and the head before anything is staged; the rest is the single-network kernel.
template <bool SAMPLED = false, bool VALUE = false, bool POP = false>
__global__ __launch_bounds__(kPolicyBlock) void policy_select_kernel(
    EnvParams p, std::conditional_t<POP, PolicyPopArgs, std::conditional_t<VALUE, PolicyValueArgs, PolicyArgs>> a) {
    extern __shared__ float w_lds[];
    const abrx::PolicyLayout lay = abrx::policy_layout<VALUE>(a.net);
    const float *weights = a.weights;
    [[maybe_unused]] const float *head = nullptr;
    if constexpr (VALUE) head = a.head;
    if constexpr (POP) {
        const int64_t member = abrx::pop_member((int64_t)blockIdx.x * kPolicyBlock, a.group);
        weights += abrx::pop_blob_offset(member, a.blob_words);
        if constexpr (VALUE) head += abrx::pop_head_offset(member, a.head_words);
    }
    if constexpr (VALUE) {
        for (int32_t d = threadIdx.x; d < lay.total; d += kPolicyBlock)
            w_lds[d] = abrx::policy_padded<true>(a.net, lay, weights, d, head);
    } else {
        for (int32_t d = threadIdx.x; d < lay.total; d += kPolicyBlock) w_lds[d] = abrx::policy_padded(a.net, lay, weights, d);
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kPolicyBlock + threadIdx.x;
    if (i >= p.n_lanes) return;
    const int64_t N = p.n_lanes;
    const abrx::PolicyNet &n = a.net;
    const int32_t c = p.chunk_id[i];
    if (p.done[i] || c < 0 || c >= p.video_length) {
        if constexpr (VALUE) {
            if (a.value_out) a.value_out[i] = 0.0f;
            if (!a.action_out) return;
        }
        a.action_out[i] = -1;
        if (a.features_out)
            for (int32_t f = 0; f < n.F; f++) a.features_out[f * N + i] = 0.0f;
        if (a.scores_out)
            for (int32_t m = 0; m < n.M; m++) a.scores_out[m * N + i] = 0.0f;
        if constexpr (SAMPLED) {
            if (a.probs_out)
                for (int32_t m = 0; m < n.M; m++) a.probs_out[m * N + i] = 0.0f;
        }
        return;
    }
    const double G = p.G[p.k[i]];
    const double P = p.lane_speeds ? p.pt_lane[i] : p.GP[p.n_play[i]];   // play_time as abr_env_observe_f64
    const auto hist = [&](int32_t j) { return p.bw_hist[j * N + i]; };
    const auto br = [&](int32_t r, int32_t m) { return chunk_bitrate(p, r, m); };
    const auto nx = [&](int32_t r, int32_t m) { return chunk_next_size(p, r, m); };
    float x[abrx::kPolicyMaxF];
    abrx::policy_features(n, hist, br, nx, p.video_length, c, p.last_action[i], p.buf[i], G, P, x);
    if (a.features_out) {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) {
            if (f < n.F) {
                a.features_out[f * N + i] = x[f];
            }
        }
    }
    float *so = a.scores_out;
    [[maybe_unused]] float value = 0.0f;
    const auto forward = [&](const auto &emit) {
        if constexpr (VALUE) return abrx::policy_forward<true>(n, w_lds, x, emit, &value);
        else return abrx::policy_forward(n, w_lds, x, emit);
    };
    int32_t action;
    if constexpr (!SAMPLED) {
        const auto emit = [&](int32_t m, float v) { if (so) so[m * N + i] = v; };
        const int32_t g = forward(emit);
        action = abrx::policy_explore(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g);
    } else {
        float *col = w_lds + lay.total + threadIdx.x;            // this lane's scores, stride kPolicyBlock
        const auto emit = [&](int32_t m, float v) {
            col[m * kPolicyBlock] = v;
            if (so) so[m * N + i] = v;
        };
        const int32_t g = forward(emit);
        float *po = a.probs_out;
        const auto buf = [&](int32_t m) -> float & { return col[m * kPolicyBlock]; };
        const auto prob = [&](int32_t m, float v) { if (po) po[m * N + i] = v; };
        action = abrx::policy_decide(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g, a.mode, a.inv_temperature,
                                     buf, prob);
    }
    if constexpr (VALUE) {
        if (a.action_out) a.action_out[i] = action;
        if (a.value_out) a.value_out[i] = value;
    } else {
        a.action_out[i] = action;
    }
}

// The struct's shape alone: the size query checks no more, the entries go on to policy_fields (before the handle).  The
// two MLP structs share one set of checks and the two recurrent ones another; an engine's limits are the parameters.
template <class Pol>
constexpr bool kRecurrent = std::is_same_v<Pol, abr_policy_gru> || std::is_same_v<Pol, abr_policy_gru_mx>;

template <class Pol>
static int validate_window(const Pol *pol) {
    if (!pol) return fail(ABR_E_INVALID, "policy is NULL");
    if (pol->window < 0 || pol->window > ABR_POLICY_MAX_WINDOW)
        return fail(ABR_E_INVALID, "policy window %d outside 0..%d", pol->window, ABR_POLICY_MAX_WINDOW);
    return ABR_OK;
}

// n_widths: how many width[] words the struct's contract covers
template <class Pol>
static int validate_mlp_shape(const Pol *pol, int max_hidden, int n_widths, int max_width) {
    int rc = validate_window(pol);
    if (rc) return rc;
    if (pol->n_hidden < 0 || pol->n_hidden > max_hidden)
        return fail(ABR_E_INVALID, "policy n_hidden %d outside 0..%d", pol->n_hidden, max_hidden);
    for (int l = 0; l < n_widths; l++) {
        const int32_t wl = pol->width[l];
        if (l < pol->n_hidden && (wl < 1 || wl > max_width))
            return fail(ABR_E_INVALID, "policy width[%d] = %d outside 1..%d", l, wl, max_width);
        if (l >= pol->n_hidden && wl != 0) return fail(ABR_E_INVALID, "policy width[%d] must be 0 past n_hidden", l);
    }
    return ABR_OK;
}

template <class Pol>
static int validate_gru_shape(const Pol *pol, int max_hidden) {
    int rc = validate_window(pol);
    if (rc) return rc;
    if (pol->hidden < 1 || pol->hidden > max_hidden)
        return fail(ABR_E_INVALID, "policy hidden %d outside 1..%d", pol->hidden, max_hidden);
    return ABR_OK;
}

static int validate_policy_shape(const abr_policy *pol) {
    return validate_mlp_shape(pol, ABR_POLICY_MAX_HIDDEN, ABR_POLICY_MAX_HIDDEN, ABR_POLICY_MAX_WIDTH);
}
static int validate_policy_shape(const abr_policy_mx *pol) {
    return validate_mlp_shape(pol, ABR_POLICY_MX_MAX_HIDDEN, ABR_POLICY_MX_MAX_HIDDEN + 1, ABR_POLICY_MX_MAX_WIDTH);
}
static int validate_policy_shape(const abr_policy_gru *pol) { return validate_gru_shape(pol, ABR_POLICY_GRU_MAX_HIDDEN); }
static int validate_policy_shape(const abr_policy_gru_mx *pol) { return validate_gru_shape(pol, ABR_POLICY_GRU_MX_MAX_HIDDEN); }

// One member's blob.  An MLP's, which abr_policy and abr_policy_mx lay out alike: per layer W [out][in], then b [out].
// A GRU cell's, which abr_policy_gru and abr_policy_gru_mx lay out alike: the three gates' W_ih, W_hh, b_ih, b_hh, then
// the output layer over h'.
template <class Pol>
static size_t policy_weights_bytes(const Pol *pol, int32_t M) {
    const size_t F = 4 + (size_t)pol->window + (size_t)M;
    if constexpr (kRecurrent<Pol>) {
        const size_t h = (size_t)pol->hidden;
        return (3 * h * (F + h + 2) + (size_t)M * (h + 1)) * sizeof(float);
    } else {
        size_t in = F, words = 0;
        for (int l = 0; l <= pol->n_hidden; l++) {
            const size_t out = l < pol->n_hidden ? (size_t)pol->width[l] : (size_t)M;
            words += out * in + out;
            in = out;
        }
        return words * sizeof(float);
    }
}

// the four abr_policy_*_weights_bytes queries
template <class Pol>
static int policy_weights_query(const Pol *pol, int32_t n_rates, size_t *bytes_out) {
    int rc = validate_policy_shape(pol);
    if (rc) return rc;
    if (!bytes_out) return fail(ABR_E_INVALID, "bytes_out is NULL");
    if (n_rates < 1 || n_rates > ABR_MAX_RATES) return fail(ABR_E_INVALID, "n_rates %d outside 1..%d", n_rates, ABR_MAX_RATES);
    *bytes_out = policy_weights_bytes(pol, n_rates);
    return ABR_OK;
}

extern "C" int abr_policy_feature_dim(int32_t window, int32_t n_rates, int32_t *dim_out) {
    if (!dim_out) return fail(ABR_E_INVALID, "dim_out is NULL");
    if (window < 0 || window > ABR_POLICY_MAX_WINDOW) return fail(ABR_E_INVALID, "window %d outside 0..%d", window, ABR_POLICY_MAX_WINDOW);
    if (n_rates < 1 || n_rates > ABR_MAX_RATES) return fail(ABR_E_INVALID, "n_rates %d outside 1..%d", n_rates, ABR_MAX_RATES);
    *dim_out = 4 + window + n_rates;
    return ABR_OK;
}

extern "C" int abr_policy_weights_bytes(const abr_policy *pol, int32_t n_rates, size_t *bytes_out) {
    return policy_weights_query(pol, n_rates, bytes_out);
}
extern "C" int abr_policy_mx_weights_bytes(const abr_policy_mx *pol, int32_t n_rates, size_t *bytes_out) {
    return policy_weights_query(pol, n_rates, bytes_out);
}
extern "C" int abr_policy_gru_weights_bytes(const abr_policy_gru *pol, int32_t n_rates, size_t *bytes_out) {
    return policy_weights_query(pol, n_rates, bytes_out);
}
extern "C" int abr_policy_gru_mx_weights_bytes(const abr_policy_gru_mx *pol, int32_t n_rates, size_t *bytes_out) {
    return policy_weights_query(pol, n_rates, bytes_out);
}

// What the engines' argument builders (policy_lane_args, policy_mx_args, policy_gru_args) share.  A builder runs
// after the handle: it checks the byte counts that depend on the environment, then fills its kernel's struct from the
// policy struct and from smp / val / pop where the entry has them (NULL otherwise).
template <class Pol>
static abrx::PolicyNet policy_net(const Pol *pol, int32_t M) {
    abrx::PolicyNet net{};
    net.window = pol->window; net.M = M; net.F = 4 + pol->window + M;
    net.norm = pol->norm_dev; net.seed = pol->seed; net.thr = pol->explore_threshold;
    return net;
}

static int check_weights_bytes(size_t got, size_t want, int32_t M) {
    if (got != want) return fail(ABR_E_INVALID, "policy weights_bytes %zu, the shape needs %zu at n_rates %d", got, want, M);
    return ABR_OK;
}

// the value head over a layer of `in` units: Wv [in], then bv
static int check_head_bytes(const abr_policy_value *val, size_t in) {
    if (val && val->head_bytes != (in + 1) * sizeof(float))
        return fail(ABR_E_INVALID, "value head_bytes %zu, the shape needs %zu", val->head_bytes, (in + 1) * sizeof(float));
    return ABR_OK;
}

// after the one-member byte counts: a population's members cover the environment's lanes exactly
static int pop_covers(const abr_env *env, const abr_policy_pop *pop) {
    if (!pop) return ABR_OK;
    const int64_t want = (env->p.n_lanes + pop->group - 1) / pop->group;
    if ((int64_t)pop->n_members != want)
        return fail(ABR_E_INVALID, "population n_members %d, %lld lanes in groups of %d need %lld", pop->n_members,
                    (long long)env->p.n_lanes, pop->group, (long long)want);
    return ABR_OK;
}

// what every kernel's struct takes from smp / val / pop as they are: the draw, the head, the members' strides in floats
template <class Args>
static void policy_shared_args(Args *a, size_t weights_bytes, const abr_policy_sampling *smp, const abr_policy_value *val,
                               const abr_policy_pop *pop) {
    if (smp) { a->mode = smp->mode; a->inv_temperature = smp->inv_temperature; }
    if (val) a->head = val->head_dev;
    if (pop) {
        a->group = pop->group;
        a->blob_words = (int32_t)(weights_bytes / sizeof(float));
        a->head_words = val ? (int32_t)(val->head_bytes / sizeof(float)) : 0;
    }
}

// The one chooser of a kernel's instances.  SAMPLED: a softmax draw or probs need the score columns in LDS; the argmax
// without probs needs none, and the plain instance decides exactly as the sampled one in mode 0.  VALUE: the launch has a
// head.  A rollout's bootstrap launch (argmax, no probs, a head) is therefore <false, true> whatever the entry's mode.
// launch(S, V) gets the two as std::bool_constants.
template <class Args, class Launch>
static hipError_t policy_instance(const Args &a, bool always_sampled, const Launch &launch) {
    const bool sampled = always_sampled || a.mode != ABR_POLICY_ARGMAX || a.probs_out, value = a.head != nullptr;
    if (sampled && value) return launch(std::true_type{}, std::true_type{});
    if (sampled) return launch(std::true_type{}, std::false_type{});
    if (value) return launch(std::false_type{}, std::true_type{});
    return launch(std::false_type{}, std::false_type{});
}

// One workgroup of BLOCK per BLOCK lanes.  `a` is the widest struct of its engine on the host: an instance compiled for
// a base of it takes `a` sliced.  most: the largest dynamic LDS the contract lets a launch of this kernel ask for, where
// that passes the 64 KiB a kernel may take by default -- the instance's limit is then raised to it, once.
template <auto Kernel, int BLOCK, class Args>
static hipError_t policy_launch(const abr_env *env, const Args &a, size_t lds, hipStream_t st, int most = 0) {
    static bool raised = false;
    if (most && !raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, most);
        if (e != hipSuccess) return e;
        raised = true;
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)((env->p.n_lanes + BLOCK - 1) / BLOCK)), dim3(BLOCK), lds, st, env->p, a);
    return hipGetLastError();
}

// The lane engine's struct is the widest one on the host whatever the entry: launch_policy_lane hands each instance the
// base it was compiled for.
static int policy_lane_args(const abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                            const abr_policy_value *val, const abr_policy_pop *pop, PolicyPopArgs *a) {
    const int32_t M = env->p.n_rates;
    int rc = check_weights_bytes(pol->weights_bytes, policy_weights_bytes(pol, M), M);
    if (rc) return rc;
    *a = PolicyPopArgs{};
    a->net = policy_net(pol, M);
    a->net.n_hidden = pol->n_hidden;
    a->net.w0 = pol->n_hidden >= 1 ? pol->width[0] : 0; a->net.w1 = pol->n_hidden >= 2 ? pol->width[1] : 0;
    a->weights = pol->weights_dev;
    if ((rc = check_head_bytes(val, pol->n_hidden == 0 ? (size_t)a->net.F : (size_t)pol->width[pol->n_hidden - 1]))) return rc;
    if ((rc = pop_covers(env, pop))) return rc;
    policy_shared_args(a, pol->weights_bytes, smp, val, pop);
    return ABR_OK;
}

// policy_select_kernel's instances.  The _sampled entries (ALWAYS_SAMPLED) run the sampled ones in every mode.
template <bool POP, bool ALWAYS_SAMPLED = false>
static hipError_t launch_policy_lane(const abr_env *env, const PolicyPopArgs &a, hipStream_t st) {
    return policy_instance(a, ALWAYS_SAMPLED, [&](auto S, auto V) {
        constexpr bool sampled = decltype(S)::value, value = decltype(V)::value;
        const size_t lds = ((size_t)abrx::policy_layout<value>(a.net).total + (sampled ? (size_t)a.net.M * kPolicyBlock : 0)) *
                           sizeof(float);
        return policy_launch<&policy_select_kernel<sampled, value, POP>, kPolicyBlock>(env, a, lds, st);
    });
}

// ---------------------------------------------------------------------------
// The matrix engine of the learned policy (include/abr_env.h: abr_policy_mx): the same chains on v_mfma_f32_32x32x2_f32
// ---------------------------------------------------------------------------
// One thread per env lane for the prologue (policy_features) and the epilogue (policy_explore / policy_decide), as
// policy_select_kernel; in between the wave is a matrix engine: the units of a layer are the rows of the product, its 64
// env lanes are two tiles of 32 columns, and a layer is tiles x steps MFMAs per column tile, k ascending, on an
// accumulator that starts as the bias (abr_lane_jump.h: the index maps and why the activations stay in registers).
// 32x32x2 rather than 16x16x4: its K of 2 wastes at most one padded k per layer (the 16x16 form pads to 4), one
// instruction covers 32 units x 32 lanes with a single A and B register, and its 64-cycle issue interval equals its
// dependent latency, so the k chain of one accumulator already runs at the issue rate with one wave per SIMD.
// Weights: the workgroup stages one layer at a time in LDS in operand order ([tile][step][wave lane], at most 64 KB: a
// read is one conflict-free ds_read_b32 per MFMA), between two barriers; biases are read from the blob when an
// accumulator is initialised.  No thread leaves before the last MFMA: a lane past n_lanes or a finished lane carries a
// zero column (columns are independent) and is masked at the stores.
constexpr int kMxBlock = 256;
typedef float mx_acc_t __attribute__((ext_vector_type(16)));

struct PolicyMxArgs {
    abrx::PolicyNet net;              // window, M, F, norm, seed, thr (n_hidden, w0, w1 unused: the shape is below)
    int32_t n_hidden, width[abrx::kMxMaxHidden];
    const float *weights, *head;      // head: [in + 1] (VALUE instances only)
    int32_t *action_out;              // [N]; NULL (VALUE only): a value evaluation that stores no decision
    float *features_out, *scores_out, *probs_out, *value_out;
    int32_t mode;
    float inv_temperature;
};

// One layer on one column tile: acc[T] = bias, then the k chain; b[s] is this lane's B register of step s.  The steps are
// taken in groups of kMxGroup: a group's A registers are all read from LDS before its first MFMA (one wait per group,
// and the next group's reads are issued while the last MFMA of this one runs); a step of the group past the layer's
// last one is an exact no-op, -0.0f against +0.0f.
constexpr int kMxGroup = 4;

template <int MAXT, int MAXS>
__device__ __forceinline__ void mx_run_layer(const abrx::MxLayer &y, const float *__restrict__ a_lds, int32_t lane,
                                             const float *b, mx_acc_t *acc) {
    const int32_t tiles = abrx::mx_tiles(y), steps = abrx::mx_steps(y.in);
#pragma unroll
    for (int T = 0; T < MAXT; T++) {                         // every tile's biases are in flight before the first chain
        if (T < tiles) {
#pragma unroll
            for (int r = 0; r < abrx::kMxRegs; r++) acc[T][r] = abrx::mx_bias(y, abrx::kMxTile * T + abrx::mx_acc_unit(lane, r));
        }
    }
#pragma unroll
    for (int T = 0; T < MAXT; T++) {
        if (T < tiles) {
            const float *at = a_lds + T * steps * abrx::kMxWave + lane;
#pragma unroll
            for (int g = 0; g < (MAXS + kMxGroup - 1) / kMxGroup; g++) {
                if (g * kMxGroup < steps) {
                    float av[kMxGroup], bv[kMxGroup];
#pragma unroll
                    for (int j = 0; j < kMxGroup; j++) {
                        const int s = g * kMxGroup + j;
                        const bool on = s < steps;
                        const float w = at[(on ? s : steps - 1) * abrx::kMxWave];
                        av[j] = on ? w : -0.0f;
                        bv[j] = on ? b[s] : 0.0f;
                    }
#pragma unroll
                    for (int j = 0; j < kMxGroup; j++)
                        acc[T] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc[T], 0, 0, 0);
                }
            }
        }
    }
}

// the POP instances' arguments (abr_policy_pop), as PolicyPopArgs
struct PolicyMxPopArgs : PolicyMxArgs {
    int32_t group, blob_words, head_words;
};
static_assert(sizeof(EnvParams) + sizeof(PolicyMxArgs) == 1016 && sizeof(EnvParams) + sizeof(PolicyMxPopArgs) == 1032,
              "policy_mx_kernel's kernarg segments");

// POP: as policy_select_kernel's -- one scalar adjustment of the blob and head pointers, made once, before the first
// layer is staged; biases (mx_bias) and the head's row are read through the adjusted pointers as well.
template <bool SAMPLED, bool VALUE, bool POP = false>
__global__ __launch_bounds__(kMxBlock) void policy_mx_kernel(EnvParams p,
                                                             std::conditional_t<POP, PolicyMxPopArgs, PolicyMxArgs> a) {
    extern __shared__ float w_lds[];
    constexpr int kMaxSteps = abrx::kMxMaxWidth / 2, kMaxTiles = abrx::kMxMaxWidth / abrx::kMxTile;
    constexpr int kXSteps = abrx::kPolicyMaxF / 2;
    const int64_t N = p.n_lanes;
    const int64_t i = (int64_t)blockIdx.x * kMxBlock + threadIdx.x;
    const int32_t lane = threadIdx.x & (abrx::kMxWave - 1);
    const abrx::PolicyNet &n = a.net;
    const bool inside = i < N;
    int32_t c = 0;
    bool live = false;
    if (inside) {
        c = p.chunk_id[i];
        live = !(p.done[i] || c < 0 || c >= p.video_length);
    }
    const bool decide = !VALUE || a.action_out;              // false: a value evaluation only
    float x[abrx::kPolicyMaxF];
    if (live) {
        const double G = p.G[p.k[i]];
        const double P = p.lane_speeds ? p.pt_lane[i] : p.GP[p.n_play[i]];   // play_time as abr_env_observe_f64
        const auto hist = [&](int32_t j) { return p.bw_hist[j * N + i]; };
        const auto br = [&](int32_t r, int32_t m) { return chunk_bitrate(p, r, m); };
        const auto nx = [&](int32_t r, int32_t m) { return chunk_next_size(p, r, m); };
        abrx::policy_features(n, hist, br, nx, p.video_length, c, p.last_action[i], p.buf[i], G, P, x);
    } else {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) x[f] = 0.0f;
    }
    if (inside && decide && a.features_out) {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) {
            if (f < n.F) {
                a.features_out[f * N + i] = x[f];
            }
        }
    }
    // this lane's B registers of the first layer, per column tile: input 2 s + (lane >> 5) of env lane 32 t + (lane & 31)
    float h[2][kMaxSteps] = {};                              // a group's steps past the layer's last one read these: +0
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int32_t src = abrx::kMxTile * t + abrx::mx_b_col(lane);
#pragma unroll
        for (int s = 0; s < kXSteps; s++) {
            const float k0 = __shfl(x[2 * s], src), k1 = __shfl(x[2 * s + 1], src);
            h[t][s] = abrx::mx_b_k(lane) ? k1 : k0;
        }
    }
    const auto stage = [&](const abrx::MxLayer &y) {
        __syncthreads();                                     // every wave has left the layer staged before
        const int32_t tiles = abrx::mx_tiles(y), steps = abrx::mx_steps(y.in);
        // A wave takes kBatch consecutive steps of a tile at a time: 16 consecutive k of 32 rows, so the 64-byte lines
        // its gathers touch are used up within the batch (rows are unaligned, `in` apart: no wider read fits), and the
        // batch's gathers are all issued before its first store.  No division: (tile, step) are the loop counters.
        constexpr int kBatch = 8;
        for (int32_t T = 0; T < tiles; T++) {
            for (int32_t s0 = kBatch * (threadIdx.x / abrx::kMxWave); s0 < steps; s0 += kBatch * (kMxBlock / abrx::kMxWave)) {
                float v[kBatch];
#pragma unroll
                for (int j = 0; j < kBatch; j++) v[j] = s0 + j < steps ? abrx::mx_staged_at(y, T, s0 + j, lane) : 0.0f;
#pragma unroll
                for (int j = 0; j < kBatch; j++) {
                    if (s0 + j < steps) w_lds[abrx::mx_staged_slot(y, T, s0 + j, lane)] = v[j];
                }
            }
        }
        __syncthreads();
    };
    const float *head = VALUE ? a.head : nullptr;
    [[maybe_unused]] const float *member_blob = nullptr;
    if constexpr (POP) {
        const int64_t member = abrx::pop_member((int64_t)blockIdx.x * kMxBlock, a.group);
        member_blob = a.weights + abrx::pop_blob_offset(member, a.blob_words);
        if constexpr (VALUE) head += abrx::pop_head_offset(member, a.head_words);
    }
    mx_acc_t acc[kMaxTiles];
    const auto activate = [&](const abrx::MxLayer &y) {      // the ReLU, into the next layer's B registers
        const int32_t tiles = abrx::mx_tiles(y);
        return [&, tiles](int t) {
#pragma unroll
            for (int T = 0; T < kMaxTiles; T++) {
                if (T < tiles) {
#pragma unroll
                    for (int r = 0; r < abrx::kMxRegs; r++) h[t][abrx::kMxRegs * T + r] = abrx::relu_f32(acc[T][r]);
                }
            }
        };
    };
    if (a.n_hidden >= 1) {
        const abrx::MxLayer y = abrx::mx_layer(POP ? member_blob : a.weights, head, n.F, n.M, a.n_hidden, a.width, 0);
        stage(y);
        const auto relu = activate(y);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            mx_run_layer<kMaxTiles, kXSteps>(y, w_lds, lane, h[t], acc);
            relu(t);
        }
    }
#pragma unroll 1
    for (int32_t li = 1; li < a.n_hidden; li++) {
        const abrx::MxLayer y = abrx::mx_layer(POP ? member_blob : a.weights, head, n.F, n.M, a.n_hidden, a.width, li);
        stage(y);
        const auto relu = activate(y);
#pragma unroll
        for (int t = 0; t < 2; t++) {
            mx_run_layer<kMaxTiles, kMaxSteps>(y, w_lds, lane, h[t], acc);
            relu(t);
        }
    }
    // the output layer (and the value head, one more row of its tile)
    mx_acc_t out[2];
    {
        const abrx::MxLayer y = abrx::mx_layer(POP ? member_blob : a.weights, head, n.F, n.M, a.n_hidden, a.width, a.n_hidden);
        stage(y);
#pragma unroll
        for (int t = 0; t < 2; t++) mx_run_layer<1, kMaxSteps>(y, w_lds, lane, h[t], &out[t]);
    }
    // unit u of env lane 32 t + j sits in register mx_unit_reg(u) of wave lane j + 32 mx_unit_half(u) of tile t: back to
    // the thread that owns the env lane
    const auto unit = [&](auto U) {
        constexpr int u = decltype(U)::value;
        const int32_t src = abrx::mx_d_col(lane) + abrx::kMxTile * abrx::mx_unit_half(u);
        const float t0 = __shfl(out[0][abrx::mx_unit_reg(u)], src), t1 = __shfl(out[1][abrx::mx_unit_reg(u)], src);
        return lane >> 5 ? t1 : t0;
    };
    float sc[abrx::kPolicyMaxRates];
    [[maybe_unused]] float value = 0.0f;
#define ABR_MX_UNIT(U) sc[U] = unit(std::integral_constant<int, U>{});
    ABR_MX_UNIT(0) ABR_MX_UNIT(1) ABR_MX_UNIT(2) ABR_MX_UNIT(3) ABR_MX_UNIT(4) ABR_MX_UNIT(5) ABR_MX_UNIT(6) ABR_MX_UNIT(7)
    ABR_MX_UNIT(8) ABR_MX_UNIT(9) ABR_MX_UNIT(10) ABR_MX_UNIT(11) ABR_MX_UNIT(12) ABR_MX_UNIT(13) ABR_MX_UNIT(14) ABR_MX_UNIT(15)
#undef ABR_MX_UNIT
    if constexpr (VALUE) value = unit(std::integral_constant<int, abrx::kMxValueUnit>{});
    if (!inside) return;
    if (!live) {
        if constexpr (VALUE) {
            if (a.value_out) a.value_out[i] = 0.0f;
        }
        if (!decide) return;
        a.action_out[i] = -1;
        if (a.scores_out)
            for (int32_t m = 0; m < n.M; m++) a.scores_out[m * N + i] = 0.0f;
        if constexpr (SAMPLED) {
            if (a.probs_out)
                for (int32_t m = 0; m < n.M; m++) a.probs_out[m * N + i] = 0.0f;
        }
        return;
    }
    if constexpr (VALUE) {
        if (a.value_out) a.value_out[i] = value;
    }
    if (!decide) return;
    float *so = a.scores_out;
    [[maybe_unused]] float *col = w_lds + abrx::mx_score_offset(n.F, a.n_hidden, a.width) + threadIdx.x;
    int32_t g = 0;
    float best = 0.0f;
#pragma unroll
    for (int m = 0; m < abrx::kPolicyMaxRates; m++) {
        if (m < n.M) {
            const float v = sc[m];
            if (so) so[m * N + i] = v;
            if constexpr (SAMPLED) col[m * kMxBlock] = v;
            if (m == 0) best = v;
            else if (v > best) { best = v; g = m; }
        }
    }
    int32_t action;
    if constexpr (!SAMPLED) {
        action = abrx::policy_explore(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g);
    } else {
        float *po = a.probs_out;
        const auto buf = [&](int32_t m) -> float & { return col[m * kMxBlock]; };
        const auto prob = [&](int32_t m, float v) { if (po) po[m * N + i] = v; };
        action = abrx::policy_decide(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g, a.mode, a.inv_temperature,
                                     buf, prob);
    }
    a.action_out[i] = action;
}

// the matrix engine's builder (as policy_lane_args: the widest struct, sliced at the launch)
static int policy_mx_args(const abr_env *env, const abr_policy_mx *pol, const abr_policy_sampling *smp,
                          const abr_policy_value *val, const abr_policy_pop *pop, PolicyMxPopArgs *a) {
    const int32_t M = env->p.n_rates;
    int rc = check_weights_bytes(pol->weights_bytes, policy_weights_bytes(pol, M), M);
    if (rc) return rc;
    *a = PolicyMxPopArgs{};
    a->net = policy_net(pol, M);
    a->n_hidden = pol->n_hidden;
    for (int l = 0; l < ABR_POLICY_MX_MAX_HIDDEN; l++) a->width[l] = pol->width[l];
    a->weights = pol->weights_dev;
    if ((rc = check_head_bytes(val, pol->n_hidden == 0 ? (size_t)a->net.F : (size_t)pol->width[pol->n_hidden - 1]))) return rc;
    if ((rc = pop_covers(env, pop))) return rc;
    policy_shared_args(a, pol->weights_bytes, smp, val, pop);
    return ABR_OK;
}

// policy_mx_kernel's instances
template <bool POP>
static hipError_t launch_policy_mx(const abr_env *env, const PolicyMxPopArgs &a, hipStream_t st) {
    return policy_instance(a, false, [&](auto S, auto V) {
        constexpr bool sampled = decltype(S)::value, value = decltype(V)::value;
        const size_t lds = (size_t)abrx::mx_lds_floats(a.net.F, a.net.M, a.n_hidden, a.width, sampled, kMxBlock) * sizeof(float);
        return policy_launch<&policy_mx_kernel<sampled, value, POP>, kMxBlock>(env, a, lds, st);
    });
}

// ---------------------------------------------------------------------------
// The recurrent policy (include/abr_env.h: abr_policy_gru): a GRU cell per lane whose state lives in the caller's slab
// ---------------------------------------------------------------------------
// One thread per lane, 256 per workgroup; the prologue and the epilogue are policy_select_kernel's.  The workgroup stages
// the padded blob (abr_lane_jump.h: policy_gru_layout -- H x 324 + 16 floats, + 68 with a value head: 83 280 B at H = 64) in
// dynamic LDS once, so every weight read is a wave-uniform broadcast of a fixed-length row.  A thread owns its column of
// the state: it reads all of h_in into registers (coalesced [H][N] column reads) before unit 0's h' is stored, so a
// commit in place is safe.  Unit j's six chains advance side by side in a software pipeline over the row's quads
// (policy_gru_forward), which bounds the reads in flight: two waves per SIMD fit the register file (__launch_bounds__).
struct PolicyGruArgs {
    abrx::PolicyNet net;              // n_hidden = 1, w0 = H
    const float *weights, *head;      // the blob; [H + 1] Wv then bv (VALUE instances)
    float *state;                     // [H][N]
    int32_t *action_out;              // [N]; NULL (VALUE instances): a value evaluation only
    float *features_out, *scores_out, *probs_out, *value_out, *hidden_out;   // nullable
    int32_t mode;                     // abr_policy_sampling (SAMPLED instances)
    float inv_temperature;
    int32_t commit;
};

// the POP instances' arguments (abr_policy_pop), as PolicyPopArgs: both recurrent kernels take them
struct PolicyGruPopArgs : PolicyGruArgs {
    int32_t group, blob_words, head_words;
};
static_assert(sizeof(EnvParams) + sizeof(PolicyGruArgs) == 1024 && sizeof(EnvParams) + sizeof(PolicyGruPopArgs) == 1040,
              "the kernarg segments of policy_gru_kernel and policy_gru_mx_kernel");

// POP: the instances behind abr_env_gru_select_pop / abr_env_gru_step_pop (abr_policy_pop), as policy_select_kernel's.  The
// workgroup computes the member it serves once, from its first lane, and stages that member's blob and head; the state
// slab is one slab whatever the population (members own disjoint columns), and the rest is the single-network kernel.
template <bool SAMPLED, bool VALUE, bool POP = false>
__global__ __launch_bounds__(kPolicyBlock, 2) void policy_gru_kernel(
    EnvParams p, std::conditional_t<POP, PolicyGruPopArgs, PolicyGruArgs> a) {
    extern __shared__ __attribute__((aligned(16))) float gru_lds[];   // rows are read as 128-bit quads
    float *w_lds = gru_lds;
    const abrx::PolicyGruLayout lay = abrx::policy_gru_layout<VALUE>(a.net);
    [[maybe_unused]] const float *member_blob = nullptr, *member_head = nullptr;
    if constexpr (POP) {
        const int64_t member = abrx::pop_member((int64_t)blockIdx.x * kPolicyBlock, a.group);
        member_blob = a.weights + abrx::pop_blob_offset(member, a.blob_words);
        if constexpr (VALUE) member_head = a.head + abrx::pop_head_offset(member, a.head_words);
    }
    for (int32_t d = threadIdx.x; d < lay.total; d += kPolicyBlock)
        w_lds[d] = abrx::policy_gru_padded<VALUE>(a.net, lay, POP ? member_blob : a.weights, d, POP ? member_head : a.head);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kPolicyBlock + threadIdx.x;
    if (i >= p.n_lanes) return;
    const int64_t N = p.n_lanes;
    const abrx::PolicyNet &n = a.net;
    const int32_t H = n.w0;
    const int32_t c = p.chunk_id[i];
    if (p.done[i] || c < 0 || c >= p.video_length) {
        if constexpr (VALUE) {
            if (a.value_out) a.value_out[i] = 0.0f;
            if (!a.action_out) return;
        }
        a.action_out[i] = -1;
        if (a.features_out)
            for (int32_t f = 0; f < n.F; f++) a.features_out[f * N + i] = 0.0f;
        if (a.scores_out)
            for (int32_t m = 0; m < n.M; m++) a.scores_out[m * N + i] = 0.0f;
        if constexpr (SAMPLED) {
            if (a.probs_out)
                for (int32_t m = 0; m < n.M; m++) a.probs_out[m * N + i] = 0.0f;
        }
        if (a.hidden_out)
            for (int32_t j = 0; j < H; j++) a.hidden_out[j * N + i] = 0.0f;
        return;
    }
    // h_in: the lane's column, or +0 at the first chunk of an episode
    float *st = a.state + i;
    float h[abrx::kPolicyRowH];
    {
        const float *row = st;                                   // a running pointer: no 64-bit scalar product per unit
#pragma unroll
        for (int k = 0; k < abrx::kPolicyRowH; k++) {
            float v = 0.0f;
            if (k < H) {
                v = *row;
                if (c == 0) v = 0.0f;
            }
            h[k] = v;
            row += N;
        }
    }
    if (a.hidden_out) {
        float *row = a.hidden_out + i;
#pragma unroll
        for (int k = 0; k < abrx::kPolicyRowH; k++) {
            if (k < H) {
                *row = h[k];
            }
            row += N;
        }
    }
    const double G = p.G[p.k[i]];
    const double P = p.lane_speeds ? p.pt_lane[i] : p.GP[p.n_play[i]];   // play_time as abr_env_observe_f64
    const auto hist = [&](int32_t j) { return p.bw_hist[j * N + i]; };
    const auto br = [&](int32_t r, int32_t m) { return chunk_bitrate(p, r, m); };
    const auto nx = [&](int32_t r, int32_t m) { return chunk_next_size(p, r, m); };
    float x[abrx::kPolicyMaxF];
    abrx::policy_features(n, hist, br, nx, p.video_length, c, p.last_action[i], p.buf[i], G, P, x);
    if (a.features_out) {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) {
            if (f < n.F) {
                a.features_out[f * N + i] = x[f];
            }
        }
    }
    const bool commit = a.commit != 0;
    const auto hin = [&](int32_t j) { return c == 0 ? 0.0f : st[j * N]; };   // read before store(j) overwrites it
    const auto store = [&](int32_t j, float v) { if (commit) st[j * N] = v; };
    float *so = a.scores_out;
    [[maybe_unused]] float value = 0.0f;
    int32_t action;
    if constexpr (!SAMPLED) {
        const auto emit = [&](int32_t m, float v) { if (so) so[m * N + i] = v; };
        const int32_t g = abrx::policy_gru_forward<VALUE>(n, w_lds, x, h, hin, store, emit, &value);
        action = abrx::policy_explore(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g);
    } else {
        float *col = w_lds + lay.total + threadIdx.x;            // this lane's scores, stride kPolicyBlock
        const auto emit = [&](int32_t m, float v) {
            col[m * kPolicyBlock] = v;
            if (so) so[m * N + i] = v;
        };
        const int32_t g = abrx::policy_gru_forward<VALUE>(n, w_lds, x, h, hin, store, emit, &value);
        float *po = a.probs_out;
        const auto buf = [&](int32_t m) -> float & { return col[m * kPolicyBlock]; };
        const auto prob = [&](int32_t m, float v) { if (po) po[m * N + i] = v; };
        action = abrx::policy_decide(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g, a.mode, a.inv_temperature,
                                     buf, prob);
    }
    if (a.action_out) a.action_out[i] = action;
    if constexpr (VALUE) {
        if (a.value_out) a.value_out[i] = value;
    }
}

// The recurrent engines' builder (Pol: abr_policy_gru or abr_policy_gru_mx; the kernels share PolicyGruPopArgs): one
// member's blob and head and the whole state slab against the environment, then the population's cover.  The struct is
// the widest one on the host whatever the entry, as policy_lane_args'.
template <class Pol>
static int policy_gru_args(const abr_env *env, const Pol *pol, const abr_policy_sampling *smp, const abr_policy_value *val,
                           const abr_policy_pop *pop, PolicyGruPopArgs *a) {
    const int32_t M = env->p.n_rates, H = pol->hidden;
    int rc = check_weights_bytes(pol->weights_bytes, policy_weights_bytes(pol, M), M);
    if (rc) return rc;
    const size_t state = (size_t)H * (size_t)env->p.n_lanes * sizeof(float);
    if (pol->state_bytes != state)
        return fail(ABR_E_INVALID, "policy state_bytes %zu, %d units x %lld lanes need %zu", pol->state_bytes, H,
                    (long long)env->p.n_lanes, state);
    if ((rc = check_head_bytes(val, (size_t)H))) return rc;
    if ((rc = pop_covers(env, pop))) return rc;
    *a = PolicyGruPopArgs{};
    a->net = policy_net(pol, M);
    a->net.n_hidden = 1; a->net.w0 = H;
    a->weights = pol->weights_dev; a->state = pol->state_dev;
    policy_shared_args(a, pol->weights_bytes, smp, val, pop);
    return ABR_OK;
}

// policy_gru_kernel's instances.  The staged blob passes the 64 KiB a kernel may take by default; the largest launch the
// contract allows is H = 64, 16 rates, a value head, the score columns: 99 664 B.
template <bool POP>
static hipError_t launch_policy_gru(const abr_env *env, const PolicyGruPopArgs &a, hipStream_t st) {
    return policy_instance(a, false, [&](auto S, auto V) {
        constexpr bool sampled = decltype(S)::value, value = decltype(V)::value;
        const size_t lds = ((size_t)abrx::policy_gru_layout<value>(a.net).total + (sampled ? (size_t)a.net.M * kPolicyBlock : 0)) *
                           sizeof(float);
        abrx::PolicyNet top{};
        top.w0 = ABR_POLICY_GRU_MAX_HIDDEN;
        const int most = (int)(((size_t)abrx::policy_gru_layout<true>(top).total + (size_t)ABR_MAX_RATES * kPolicyBlock) *
                               sizeof(float));
        return policy_launch<&policy_gru_kernel<sampled, value, POP>, kPolicyBlock>(env, a, lds, st, most);
    });
}

// ---------------------------------------------------------------------------
// The matrix engine of the recurrent policy (include/abr_env.h: abr_policy_gru_mx): abr_policy_gru's chains on
// v_mfma_f32_32x32x2_f32, H up to 128
// ---------------------------------------------------------------------------
// The prologue and the epilogue are policy_mx_kernel's: one thread per env lane, a wave's 64 env lanes as two column tiles
// of 32.  In between (abr_lane_jump.h: gru_mx_*) the 3H gate rows are the rows of the product, 32 units at a time.  A
// lane's B registers of h_in come straight from the slab -- input 2 s + (lane >> 5) of env lane 32 t + (lane & 31), all of
// them before the first store of h' -- and register r of unit tile U's accumulators holds the unit that B register
// 16 U + r holds, so the gates are element-wise on registers, the lane that loaded h_in[j] of a column is the lane that
// stores its h'[j] (a commit in place is safe), and a tile's h' is as it stands the B operand of output steps
// 16 U .. 16 U + 15: it is folded into the output accumulator at once, U ascending, so every output stays a k-ordered
// chain.  The workgroup stages one unit tile at a time in LDS in operand order (gru_mx_staged_at: per gate the W_ih
// steps, the W_hh steps, each padded to whole groups, then the tile's slice of the output rows; at most 68 608 B, one
// ds_read_b32 per MFMA) between two barriers.  The column tiles are the outer loop and the unit tiles the inner one,
// both rolled: one column tile's B operands are resident at a time (64 of h_in, 18 of x) and a unit tile is staged again
// for the second column tile; the gates retire one after another (r, z, then n with h'), two accumulators live at a
// time.  One wave per SIMD has the whole unified register file.  Biases are read from the blob when an accumulator is
// initialised.  No thread leaves before the last MFMA; a lane past n_lanes or a finished lane carries a zero column and
// is masked at every store.
// The arguments are the lane engine's (PolicyGruArgs).
// One chain of one accumulator: `steps` MFMAs, k ascending, a group of kGruMxGroup at a time.  at = the chain's first
// staged row + lane, b[s] the B register of step s.  A step of the last group past `steps` reads a pad row (-0.0f) against a
// B register that is +0.0f: an exact no-op, and no step needs a predicate of its own.
static_assert(kMxGroup == abrx::kGruMxGroup, "one group size");
template <int MAXS>
__device__ __forceinline__ void gru_mx_chain(const float *__restrict__ at, int32_t steps, const float *b, mx_acc_t &acc) {
#pragma unroll
    for (int g = 0; g < MAXS / kMxGroup; g++) {
        if (g * kMxGroup < steps) {
            float av[kMxGroup];
#pragma unroll
            for (int j = 0; j < kMxGroup; j++) av[j] = at[(g * kMxGroup + j) * abrx::kMxWave];
#pragma unroll
            for (int j = 0; j < kMxGroup; j++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[g * kMxGroup + j], acc, 0, 0, 0);
        }
    }
}

// POP: as policy_gru_kernel's -- the member's blob and head are what gru_mx() lays out at every unit tile, so the staged
// operands, the biases and the output and value rows are all the member's.
template <bool SAMPLED, bool VALUE, bool POP = false>
__global__ __launch_bounds__(kMxBlock) void policy_gru_mx_kernel(
    EnvParams p, std::conditional_t<POP, PolicyGruPopArgs, PolicyGruArgs> a) {
    extern __shared__ float gmx_lds[];
    constexpr int kHSteps = abrx::kGruMxMaxHidden / 2;
    constexpr int kXSteps = (abrx::kPolicyMaxF / 2 + kMxGroup - 1) / kMxGroup * kMxGroup;   // whole groups
    static_assert(kHSteps % kMxGroup == 0 && kHSteps == abrx::kGruMxMaxTiles * abrx::kMxRegs, "groups and tiles");
    const int64_t N = p.n_lanes;
    const int64_t i = (int64_t)blockIdx.x * kMxBlock + threadIdx.x;
    const int32_t lane = threadIdx.x & (abrx::kMxWave - 1), half = abrx::mx_b_k(lane);
    const abrx::PolicyNet &n = a.net;
    const int32_t H = n.w0;
    const bool inside = i < N;
    int32_t c = 0;
    bool live = false;
    if (inside) {
        c = p.chunk_id[i];
        live = !(p.done[i] || c < 0 || c >= p.video_length);
    }
    const bool decide = !VALUE || a.action_out;              // false: a value evaluation only
    float x[abrx::kPolicyMaxF];
    if (live) {
        const double G = p.G[p.k[i]];
        const double P = p.lane_speeds ? p.pt_lane[i] : p.GP[p.n_play[i]];   // play_time as abr_env_observe_f64
        const auto hist = [&](int32_t j) { return p.bw_hist[j * N + i]; };
        const auto br = [&](int32_t r, int32_t m) { return chunk_bitrate(p, r, m); };
        const auto nx = [&](int32_t r, int32_t m) { return chunk_next_size(p, r, m); };
        abrx::policy_features(n, hist, br, nx, p.video_length, c, p.last_action[i], p.buf[i], G, P, x);
    } else {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) x[f] = 0.0f;
    }
    // One column tile at a time (a loop, not an unrolled pair: the registers of one tile's B operands are live, 64 of
    // h_in and 18 of x), and within it the unit tiles, each staged again for the second column tile from what the first
    // left in the cache.  This lane's B registers for column tile t, whose env lane is `col`: xb[s] = x[2 s + half],
    // h[s] = h_in[2 s + half] -- +0.0f where c == 0, where the column's lane takes no decision and past H.
    const int32_t tiles = abrx::gru_mx_tiles(H);
    const bool commit = a.commit != 0;
    [[maybe_unused]] const float *member_blob = nullptr, *member_head = nullptr;
    if constexpr (POP) {
        const int64_t member = abrx::pop_member((int64_t)blockIdx.x * kMxBlock, a.group);
        member_blob = a.weights + abrx::pop_blob_offset(member, a.blob_words);
        if constexpr (VALUE) member_head = a.head + abrx::pop_head_offset(member, a.head_words);
    }
    float sc[abrx::kPolicyMaxRates] = {};
    [[maybe_unused]] float value = 0.0f;
#pragma unroll 1
    for (int32_t t = 0; t < 2; t++) {
        // Ht and Nt are H and N behind an empty statement: what follows is the same for both column tiles and for every
        // unit tile, and the compiler would otherwise compute its predicates, offsets and addresses once, ahead of the
        // loops, and keep them all (the same again at the top of the unit-tile loop).
        int32_t Ht = H;
        int64_t Nt = N;
        asm volatile("" : "+s"(Ht), "+s"(Nt));
        const int32_t src = abrx::kMxTile * t + abrx::mx_b_col(lane);
        const int64_t col = i - lane + src;
        const bool col_live = __shfl((int32_t)live, src) != 0;
        const bool col_read = col_live && __shfl(c, src) != 0;
        float xb[kXSteps] = {}, h[kHSteps];
#pragma unroll
        for (int s = 0; s < abrx::kPolicyMaxF / 2; s++) {
            const float k0 = __shfl(x[2 * s], src), k1 = __shfl(x[2 * s + 1], src);
            xb[s] = half ? k1 : k0;
        }
        // The slab, a tile of units at a time (a uniform branch each, then a scheduling fence, so that the addresses of
        // one tile's reads are in flight at a time).  Every read is unconditional and inside the slab -- a column past
        // n_lanes reads column 0, the odd half past an odd H reads the even row -- and hmax discards what the lane may
        // not use.  All of them are issued before this column tile's first store of h'.
        {
            const bool in = col < Nt, report = decide && a.hidden_out && in;
            const int32_t hmax = col_read ? Ht : 0;
            const int64_t hoff = half ? Nt : 0;
            const float *row = a.state + (in ? col : 0);         // running pointers, two rows a step
            float *orow = a.hidden_out + col + hoff;
#pragma unroll
            for (int T = 0; T < abrx::kGruMxMaxTiles; T++) {
                if (abrx::kMxTile * T < Ht) {
#pragma unroll
                    for (int r = 0; r < abrx::kMxRegs; r++) {
                        const int s = abrx::kMxRegs * T + r;
                        const float v = row[2 * s + 1 < Ht ? hoff : 0];
                        h[s] = 2 * s + half < hmax ? v : 0.0f;
                        if (2 * s + 2 < Ht) row += 2 * Nt;
                    }
                    if (report) {
#pragma unroll
                        for (int r = 0; r < abrx::kMxRegs; r++) {
                            const int s = abrx::kMxRegs * T + r;
                            if (2 * s + half < Ht) {
                                *orow = h[s];
                            }
                            orow += 2 * Nt;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                } else {
#pragma unroll
                    for (int r = 0; r < abrx::kMxRegs; r++) h[abrx::kMxRegs * T + r] = 0.0f;
                }
            }
        }
        mx_acc_t out;
        {
            const abrx::GruMx y = abrx::gru_mx(POP ? member_blob : a.weights, VALUE ? (POP ? member_head : a.head) : nullptr,
                                               n.F, Ht, n.M);
#pragma unroll
            for (int r = 0; r < abrx::kMxRegs; r++) out[r] = abrx::gru_mx_b_out(y, abrx::mx_acc_unit(lane, r));
        }
#pragma unroll 1
        for (int32_t U = 0; U < tiles; U++) {
            int32_t Hu = H;
            asm volatile("" : "+s"(Hu));
            const abrx::GruMx y = abrx::gru_mx(POP ? member_blob : a.weights, VALUE ? (POP ? member_head : a.head) : nullptr,
                                               n.F, Hu, n.M);
            const int32_t rows = abrx::gru_mx_rows(n.F, Hu), sF = abrx::mx_steps(n.F), sH = abrx::mx_steps(Hu);
            __syncthreads();                                 // every wave has left the tile staged before
            {
                // a wave takes kBatch consecutive rows at a time and issues their gathers before its first store
                constexpr int kBatch = 8;
                for (int32_t q0 = kBatch * (threadIdx.x / abrx::kMxWave); q0 < rows; q0 += kBatch * (kMxBlock / abrx::kMxWave)) {
                    float v[kBatch];
#pragma unroll
                    for (int j = 0; j < kBatch; j++) v[j] = q0 + j < rows ? abrx::gru_mx_staged_at(y, U, q0 + j, lane) : 0.0f;
#pragma unroll
                    for (int j = 0; j < kBatch; j++) {
                        if (q0 + j < rows) gmx_lds[(q0 + j) * abrx::kMxWave + lane] = v[j];
                    }
                }
            }
            __syncthreads();
            const int32_t j0 = abrx::kMxTile * U;            // register r holds unit j0 + mx_acc_unit(lane, r)
            // gate by gate, so that two accumulators are live at a time: r, z, then n and with it h'
            float rz[2][abrx::kMxRegs];
            mx_acc_t hp;
#pragma unroll
            for (int g = 0; g < 3; g++) {
                mx_acc_t gi, gh;
#pragma unroll
                for (int r = 0; r < abrx::kMxRegs; r++) {
                    gi[r] = abrx::gru_mx_b_ih(y, g, j0 + abrx::mx_acc_unit(lane, r));
                    gh[r] = abrx::gru_mx_b_hh(y, g, j0 + abrx::mx_acc_unit(lane, r));
                }
                gru_mx_chain<kXSteps>(gmx_lds + abrx::gru_mx_ih_row(n.F, Hu, g) * abrx::kMxWave + lane, sF, xb, gi);
                gru_mx_chain<kHSteps>(gmx_lds + abrx::gru_mx_hh_row(n.F, Hu, g) * abrx::kMxWave + lane, sH, h, gh);
#pragma unroll
                for (int r = 0; r < abrx::kMxRegs; r++) {
                    if (g < 2) {
                        rz[g][r] = abrx::gru_mx_gate(gi[r], gh[r]);
                    } else {
                        // h_in of the unit: B register 16 U + r (U is a loop counter: a select, not an index)
                        const float hj = U == 0 ? h[r] : U == 1 ? h[abrx::kMxRegs + r]
                                       : U == 2 ? h[2 * abrx::kMxRegs + r] : h[3 * abrx::kMxRegs + r];
                        hp[r] = abrx::gru_mx_unit(rz[0][r], rz[1][r], gi[r], gh[r], hj, j0 + abrx::mx_acc_unit(lane, r) < Hu);
                    }
                }
            }
            if (commit && col_live) {
                float *srow = a.state + col + (int64_t)(j0 + half) * Nt;
#pragma unroll
                for (int r = 0; r < abrx::kMxRegs; r++) {
                    if (j0 + abrx::mx_acc_unit(lane, r) < Hu) {
                        *srow = hp[r];
                    }
                    srow += 2 * Nt;
                }
            }
            const float *ao = gmx_lds + abrx::gru_mx_out_row(n.F, Hu) * abrx::kMxWave + lane;
            float av[abrx::kMxRegs];
#pragma unroll
            for (int s = 0; s < abrx::kMxRegs; s++) av[s] = ao[s * abrx::kMxWave];
#pragma unroll
            for (int s = 0; s < abrx::kMxRegs; s++) out = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], hp[s], out, 0, 0, 0);
        }
        // Unit u of env lane 32 t + j sits in register mx_unit_reg(u) of wave lane j + 32 mx_unit_half(u): back to the
        // thread that owns the env lane, which is in this column tile when lane >> 5 == t.
        const bool mine = (lane >> 5) == t;
        const auto unit = [&](auto Uc, float old) {
            constexpr int u = decltype(Uc)::value;
            const float v = __shfl(out[abrx::mx_unit_reg(u)], abrx::mx_d_col(lane) + abrx::kMxTile * abrx::mx_unit_half(u));
            return mine ? v : old;
        };
#define ABR_MX_UNIT(U) sc[U] = unit(std::integral_constant<int, U>{}, sc[U]);
        ABR_MX_UNIT(0) ABR_MX_UNIT(1) ABR_MX_UNIT(2) ABR_MX_UNIT(3) ABR_MX_UNIT(4) ABR_MX_UNIT(5) ABR_MX_UNIT(6) ABR_MX_UNIT(7)
        ABR_MX_UNIT(8) ABR_MX_UNIT(9) ABR_MX_UNIT(10) ABR_MX_UNIT(11) ABR_MX_UNIT(12) ABR_MX_UNIT(13) ABR_MX_UNIT(14) ABR_MX_UNIT(15)
#undef ABR_MX_UNIT
        if constexpr (VALUE) value = unit(std::integral_constant<int, abrx::kMxValueUnit>{}, value);
    }
    if (!inside) return;
    // every output pointer is first read here, after the loops: none of them is live across the MFMAs
    if (decide && a.features_out) {
#pragma unroll
        for (int f = 0; f < abrx::kPolicyMaxF; f++) {
            if (f < n.F) {
                a.features_out[f * N + i] = x[f];
            }
        }
    }
    if (!live) {
        if constexpr (VALUE) {
            if (a.value_out) a.value_out[i] = 0.0f;
        }
        if (!decide) return;
        a.action_out[i] = -1;
        if (a.scores_out)
            for (int32_t m = 0; m < n.M; m++) a.scores_out[m * N + i] = 0.0f;
        if constexpr (SAMPLED) {
            if (a.probs_out)
                for (int32_t m = 0; m < n.M; m++) a.probs_out[m * N + i] = 0.0f;
        }
        return;
    }
    if constexpr (VALUE) {
        if (a.value_out) a.value_out[i] = value;
    }
    if (!decide) return;
    float *so = a.scores_out;
    [[maybe_unused]] float *scol = gmx_lds + abrx::gru_mx_score_offset(n.F, H) + threadIdx.x;
    int32_t g = 0;
    float best = 0.0f;
#pragma unroll
    for (int m = 0; m < abrx::kPolicyMaxRates; m++) {
        if (m < n.M) {
            const float v = sc[m];
            if (so) so[m * N + i] = v;
            if constexpr (SAMPLED) scol[m * kMxBlock] = v;
            if (m == 0) best = v;
            else if (v > best) { best = v; g = m; }
        }
    }
    int32_t action;
    if constexpr (!SAMPLED) {
        action = abrx::policy_explore(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g);
    } else {
        float *po = a.probs_out;
        const auto buf = [&](int32_t m) -> float & { return scol[m * kMxBlock]; };
        const auto prob = [&](int32_t m, float v) { if (po) po[m * N + i] = v; };
        action = abrx::policy_decide(n, (uint64_t)(p.lane_id_base + i), c, p.episode_no[i], g, a.mode, a.inv_temperature,
                                     buf, prob);
    }
    a.action_out[i] = action;
}

// policy_gru_mx_kernel's instances.  A unit tile at H = 128, W = 16, 16 rates is 68 608 B, past the 64 KiB a kernel may
// take by default; the largest launch the contract allows has the score columns as well: 84 992 B.
template <bool POP>
static hipError_t launch_policy_gru_mx(const abr_env *env, const PolicyGruPopArgs &a, hipStream_t st) {
    return policy_instance(a, false, [&](auto S, auto V) {
        constexpr bool sampled = decltype(S)::value, value = decltype(V)::value;
        const size_t lds = (size_t)abrx::gru_mx_lds_floats(a.net.F, a.net.w0, a.net.M, sampled, kMxBlock) * sizeof(float);
        const int most = (int)((size_t)abrx::gru_mx_lds_floats(abrx::kPolicyMaxF, ABR_POLICY_GRU_MX_MAX_HIDDEN, ABR_MAX_RATES,
                                                               true, kMxBlock) * sizeof(float));
        return policy_launch<&policy_gru_mx_kernel<sampled, value, POP>, kMxBlock>(env, a, lds, st, most);
    });
}

// ---------------------------------------------------------------------------
// The host path of the learned-policy entries: one validator, one select, one rollout, whatever the engine
// ---------------------------------------------------------------------------
// An engine is an argument struct, a builder that fills it after the handle (policy_lane_args, policy_mx_args,
// policy_gru_args for both recurrent engines) and a launcher that states its kernel template, LDS size and block
// (launch_policy_lane, launch_policy_mx, launch_policy_gru, launch_policy_gru_mx), next to its validate_policy_shape's
// limits.  Everything below is shared, as are policy_shared_args, policy_instance and policy_launch above.

// the sampling struct alone
static int validate_sampling(const abr_policy_sampling *smp) {
    if (!smp) return fail(ABR_E_INVALID, "sampling is NULL");
    if (smp->mode != ABR_POLICY_ARGMAX && smp->mode != ABR_POLICY_SOFTMAX)
        return fail(ABR_E_INVALID, "sampling mode %d is neither ABR_POLICY_ARGMAX nor ABR_POLICY_SOFTMAX", smp->mode);
    const float t = smp->inv_temperature;
    if (!(t > 0.0f && t <= 0x1.fffffep127f)) return fail(ABR_E_INVALID, "sampling inv_temperature must be finite and > 0");
    for (int32_t r : smp->reserved_)
        if (r) return fail(ABR_E_INVALID, "sampling reserved_ must be 0");
    return ABR_OK;
}

// the value struct alone
static int validate_value(const abr_policy_value *val) {
    if (!val) return fail(ABR_E_INVALID, "value is NULL");
    if (!val->head_dev || ((uintptr_t)val->head_dev & 3))
        return fail(ABR_E_INVALID, "value head must be non-NULL and 4-byte aligned");
    for (int32_t r : val->reserved_)
        if (r) return fail(ABR_E_INVALID, "value reserved_ must be 0");
    return ABR_OK;
}

// the population struct alone
static int validate_pop(const abr_policy_pop *pop) {
    if (!pop) return fail(ABR_E_INVALID, "population is NULL");
    if (pop->n_members < 1) return fail(ABR_E_INVALID, "population n_members %d must be >= 1", pop->n_members);
    if (pop->group < kPolicyBlock || pop->group % kPolicyBlock)
        return fail(ABR_E_INVALID, "population group %d must be a positive multiple of %d", pop->group, kPolicyBlock);
    for (int32_t r : pop->reserved_)
        if (r) return fail(ABR_E_INVALID, "population reserved_ must be 0");
    // a launch covers at most 2^32 - 1 workgroups of 256 lanes: no environment can have the lanes of a larger product
    if ((int64_t)pop->n_members * (int64_t)pop->group > (int64_t)UINT32_MAX * kPolicyBlock)
        return fail(ABR_E_INVALID, "population n_members %d x group %d overflows the lanes of a launch", pop->n_members,
                    pop->group);
    return ABR_OK;
}

// what abr_policy, abr_policy_mx, abr_policy_gru and abr_policy_gru_mx hold past their shape: reserved words, pointers, threshold
template <class Pol>
static int validate_policy_fields(const Pol *pol) {
    for (int32_t r : pol->reserved_)
        if (r) return fail(ABR_E_INVALID, "policy reserved_ must be 0");
    if (!pol->weights_dev || ((uintptr_t)pol->weights_dev & 3))
        return fail(ABR_E_INVALID, "policy weights must be non-NULL and 4-byte aligned");
    if ((uintptr_t)pol->norm_dev & 7) return fail(ABR_E_INVALID, "policy norm must be 8-byte aligned");
    if constexpr (kRecurrent<Pol>) {
        if (!pol->state_dev || ((uintptr_t)pol->state_dev & 3))
            return fail(ABR_E_INVALID, "policy state must be non-NULL and 4-byte aligned");
    }
    if (pol->explore_threshold > (1ull << 32))
        return fail(ABR_E_INVALID, "explore_threshold %llu above 2^32", (unsigned long long)pol->explore_threshold);
    return ABR_OK;
}

// The outputs of a select (one row of each) or of a rollout (n_steps rows; last_value one), nullable but a select's action.
struct PolicyOut {
    int32_t *action;
    float *features, *scores, *probs, *value, *hidden;
    float *last_value, *obs, *reward;   // rollouts only
    uint8_t *done;
};

// the structs an entry cannot do without (the others are checked where they are given)
enum : unsigned { kNeedsSmp = 1, kNeedsVal = 2, kNeedsPop = 4 };

// Everything an entry checks before it reads the handle, in the order include/abr_env.h documents for each of them: the
// policy struct, smp, val, the outputs that need a struct that is absent, pop, n_steps (NULL: a select), the handle.
template <class Pol>
static int validate_policy_call(const abr_env *env, const Pol *pol, unsigned needs, const abr_policy_sampling *smp,
                                const abr_policy_value *val, const abr_policy_pop *pop, const int32_t *n_steps,
                                const PolicyOut &o) {
    int rc = validate_policy_shape(pol);
    if (rc || (rc = validate_policy_fields(pol))) return rc;
    if ((smp || (needs & kNeedsSmp)) && (rc = validate_sampling(smp))) return rc;
    if ((val || (needs & kNeedsVal)) && (rc = validate_value(val))) return rc;
    if (!smp && o.probs) return fail(ABR_E_INVALID, "probs need a sampling struct");
    if (!val && (o.value || o.last_value)) return fail(ABR_E_INVALID, "values need a value struct");
    if ((needs & kNeedsPop) && (rc = validate_pop(pop))) return rc;
    if (!n_steps) return env && o.action ? ABR_OK : fail(ABR_E_INVALID, "NULL argument (env or action_out_dev)");
    if (*n_steps < 1) return fail(ABR_E_INVALID, "n_steps must be >= 1");
    return env ? ABR_OK : fail(ABR_E_INVALID, "env is NULL");
}

// the recurrent engine's part of a launch: where h_in is reported, and whether h' replaces it in the caller's slab
template <class Args>
static void set_recurrence(Args &, float *, int32_t) {}
static void set_recurrence(PolicyGruPopArgs &a, float *hidden_out, int32_t commit) {
    a.hidden_out = hidden_out;
    a.commit = commit;
}

// one decision per lane on the current state
template <class Args, class Launch>
static int policy_select_once(const abr_env *env, Args &a, const Launch &launch, const PolicyOut &o, void *stream) {
    a.action_out = o.action; a.features_out = o.features; a.scores_out = o.scores;
    a.probs_out = o.probs; a.value_out = o.value;
    HIP_TRY(launch(env, a, (hipStream_t)stream));
    return ABR_OK;
}

// Per decision the policy kernel on row s of the outputs, then K1 MODE 1 on its actions, back to back on the stream (as
// mpc_rollout); the recurrent kernel commits each h'.  Then, if asked for, the bootstrap value of the state the rollout
// leaves behind, which has one form for every engine: an argmax launch that stores no decision, no feature, score or prob
// and commits nothing, so the workspace and the state slab stay as the rollout left them.
template <class Args, class Launch>
static int policy_rollout(const abr_env *env, Args &a, const Launch &launch, int32_t n_steps, const PolicyOut &o,
                          void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    const int64_t N = env->p.n_lanes;
    const int rc = rollout_per_launch(env, kPolicyRollout, n_steps, o.action, st, o.obs, o.reward, o.done,
                                      [&](int32_t s, int32_t *action) {
        a.action_out = action;
        a.features_out = slab_row(o.features, s, a.net.F, N);
        a.scores_out = slab_row(o.scores, s, a.net.M, N);
        a.probs_out = slab_row(o.probs, s, a.net.M, N);
        a.value_out = slab_row(o.value, s, 1, N);
        set_recurrence(a, slab_row(o.hidden, s, a.net.w0, N), 1);
        HIP_TRY(launch(env, a, st));
        return ABR_OK;
    });
    if (rc) return rc;
    if (o.last_value) {
        a.action_out = nullptr; a.features_out = a.scores_out = a.probs_out = nullptr;
        a.mode = ABR_POLICY_ARGMAX;
        a.value_out = o.last_value;
        set_recurrence(a, nullptr, 0);
        HIP_TRY(launch(env, a, st));
    }
    return ABR_OK;
}

// An entry: the checks before the handle, the engine's builder, then the rollout (n_steps given) or the one select.
template <class Pol, class Args>
static int policy_entry(const abr_env *env, const Pol *pol, unsigned needs, const abr_policy_sampling *smp,
                        const abr_policy_value *val, const abr_policy_pop *pop,
                        int (*build)(const abr_env *, const Pol *, const abr_policy_sampling *, const abr_policy_value *,
                                     const abr_policy_pop *, Args *),
                        hipError_t (*launch)(const abr_env *, const Args &, hipStream_t), const int32_t *n_steps,
                        const PolicyOut &o, void *stream, int32_t commit = 0) {
    int rc = validate_policy_call(env, pol, needs, smp, val, pop, n_steps, o);
    if (rc) return rc;
    Args a;
    if ((rc = build(env, pol, smp, val, pop, &a))) return rc;
    if (n_steps) return policy_rollout(env, a, launch, *n_steps, o, stream);
    set_recurrence(a, o.hidden, commit);
    return policy_select_once(env, a, launch, o, stream);
}

extern "C" int abr_env_policy_select(abr_env *env, const abr_policy *pol, int32_t *action_out_dev, float *features_out_dev,
                                     float *scores_out_dev, void *stream) {
    return policy_entry(env, pol, 0, nullptr, nullptr, nullptr, policy_lane_args, launch_policy_lane<false>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev}, stream);
}

extern "C" int abr_env_step_policy(abr_env *env, const abr_policy *pol, int32_t n_steps, float *obs_out_dev,
                                   float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                   float *features_out_dev, float *scores_out_dev, void *stream) {
    return policy_entry(env, pol, 0, nullptr, nullptr, nullptr, policy_lane_args, launch_policy_lane<false>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, nullptr, nullptr, nullptr, nullptr, obs_out_dev,
                         reward_out_dev, done_out_dev}, stream);
}

extern "C" int abr_env_policy_select_sampled(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                                             int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                             float *probs_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsSmp, smp, nullptr, nullptr, policy_lane_args, launch_policy_lane<false, true>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev}, stream);
}

extern "C" int abr_env_step_policy_sampled(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                                           int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                                           uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev,
                                           float *scores_out_dev, float *probs_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsSmp, smp, nullptr, nullptr, policy_lane_args, launch_policy_lane<false, true>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, nullptr, nullptr, nullptr,
                         obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// Actor-critic rollouts (include/abr_env.h: abr_policy_value, abr_gae): the VALUE instances, and last_value
extern "C" int abr_env_policy_select_ac(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                                        const abr_policy_value *val, int32_t *action_out_dev, float *features_out_dev,
                                        float *scores_out_dev, float *probs_out_dev, float *value_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsSmp | kNeedsVal, smp, val, nullptr, policy_lane_args, launch_policy_lane<false>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev}, stream);
}

extern "C" int abr_env_step_policy_ac(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                                      const abr_policy_value *val, int32_t n_steps, float *obs_out_dev,
                                      float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                      float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                      float *values_out_dev, float *last_value_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsSmp | kNeedsVal, smp, val, nullptr, policy_lane_args, launch_policy_lane<false>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, nullptr,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// the matrix engine: one entry pair for every mode, smp and val nullable
extern "C" int abr_env_policy_select_mx(abr_env *env, const abr_policy_mx *pol, const abr_policy_sampling *smp,
                                        const abr_policy_value *val, int32_t *action_out_dev, float *features_out_dev,
                                        float *scores_out_dev, float *probs_out_dev, float *value_out_dev, void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_mx_args, launch_policy_mx<false>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev}, stream);
}

extern "C" int abr_env_step_policy_mx(abr_env *env, const abr_policy_mx *pol, const abr_policy_sampling *smp,
                                      const abr_policy_value *val, int32_t n_steps, float *obs_out_dev,
                                      float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                      float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                      float *values_out_dev, float *last_value_out_dev, void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_mx_args, launch_policy_mx<false>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, nullptr,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// populations (include/abr_env.h: abr_policy_pop): one weight set per lane group, both engines' POP instances
extern "C" int abr_env_policy_select_pop(abr_env *env, const abr_policy *pol, const abr_policy_pop *pop,
                                         const abr_policy_sampling *smp, const abr_policy_value *val,
                                         int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                         float *probs_out_dev, float *value_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_lane_args, launch_policy_lane<true>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev}, stream);
}

extern "C" int abr_env_step_policy_pop(abr_env *env, const abr_policy *pol, const abr_policy_pop *pop,
                                       const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                                       float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                       int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                                       float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                                       void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_lane_args, launch_policy_lane<true>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, nullptr,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

extern "C" int abr_env_policy_select_mx_pop(abr_env *env, const abr_policy_mx *pol, const abr_policy_pop *pop,
                                            const abr_policy_sampling *smp, const abr_policy_value *val,
                                            int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                            float *probs_out_dev, float *value_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_mx_args, launch_policy_mx<true>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev}, stream);
}

extern "C" int abr_env_step_policy_mx_pop(abr_env *env, const abr_policy_mx *pol, const abr_policy_pop *pop,
                                          const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                                          float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                          int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                                          float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                                          void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_mx_args, launch_policy_mx<true>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, nullptr,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// the recurrent engine: a select commits h' only when asked to, a rollout at every decision
extern "C" int abr_env_policy_select_gru(abr_env *env, const abr_policy_gru *pol, const abr_policy_sampling *smp,
                                         const abr_policy_value *val, int32_t commit, int32_t *action_out_dev,
                                         float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                         float *value_out_dev, float *hidden_out_dev, void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_gru_args<abr_policy_gru>, launch_policy_gru<false>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev, hidden_out_dev},
                        stream, commit != 0);
}

extern "C" int abr_env_step_policy_gru(abr_env *env, const abr_policy_gru *pol, const abr_policy_sampling *smp,
                                       const abr_policy_value *val, int32_t n_steps, float *obs_out_dev,
                                       float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                       float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                       float *values_out_dev, float *last_value_out_dev, float *hidden_out_dev,
                                       void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_gru_args<abr_policy_gru>, launch_policy_gru<false>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, hidden_out_dev,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// the recurrent policy's matrix engine: the same pair, the wider struct
extern "C" int abr_env_gru_mx_select(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_sampling *smp,
                                     const abr_policy_value *val, int32_t commit, int32_t *action_out_dev,
                                     float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                     float *value_out_dev, float *hidden_out_dev, void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_gru_args<abr_policy_gru_mx>, launch_policy_gru_mx<false>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev, hidden_out_dev},
                        stream, commit != 0);
}

extern "C" int abr_env_gru_mx_step(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_sampling *smp,
                                   const abr_policy_value *val, int32_t n_steps, float *obs_out_dev,
                                   float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                   float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                   float *values_out_dev, float *last_value_out_dev, float *hidden_out_dev,
                                   void *stream) {
    return policy_entry(env, pol, 0, smp, val, nullptr, policy_gru_args<abr_policy_gru_mx>, launch_policy_gru_mx<false>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, hidden_out_dev,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// recurrent populations (include/abr_env.h: abr_policy_pop over abr_policy_gru / abr_policy_gru_mx): both engines' POP
// instances, one state slab
extern "C" int abr_env_gru_select_pop(abr_env *env, const abr_policy_gru *pol, const abr_policy_pop *pop,
                                             const abr_policy_sampling *smp, const abr_policy_value *val, int32_t commit,
                                             int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                             float *probs_out_dev, float *value_out_dev, float *hidden_out_dev,
                                             void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_gru_args<abr_policy_gru>, launch_policy_gru<true>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev, hidden_out_dev},
                        stream, commit != 0);
}

extern "C" int abr_env_gru_step_pop(abr_env *env, const abr_policy_gru *pol, const abr_policy_pop *pop,
                                           const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                                           float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                           int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                                           float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                                           float *hidden_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_gru_args<abr_policy_gru>, launch_policy_gru<true>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, hidden_out_dev,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

extern "C" int abr_env_gru_mx_select_pop(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_pop *pop,
                                         const abr_policy_sampling *smp, const abr_policy_value *val, int32_t commit,
                                         int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                         float *probs_out_dev, float *value_out_dev, float *hidden_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_gru_args<abr_policy_gru_mx>, launch_policy_gru_mx<true>, nullptr,
                        {action_out_dev, features_out_dev, scores_out_dev, probs_out_dev, value_out_dev, hidden_out_dev},
                        stream, commit != 0);
}

extern "C" int abr_env_gru_mx_step_pop(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_pop *pop,
                                       const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                                       float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                       int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                                       float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                                       float *hidden_out_dev, void *stream) {
    return policy_entry(env, pol, kNeedsPop, smp, val, pop, policy_gru_args<abr_policy_gru_mx>, launch_policy_gru_mx<true>, &n_steps,
                        {actions_out_dev, features_out_dev, scores_out_dev, probs_out_dev, values_out_dev, hidden_out_dev,
                         last_value_out_dev, obs_out_dev, reward_out_dev, done_out_dev}, stream);
}

// One thread per lane walks its column of the slabs from the last row to the first (abr_lane_jump.h: gae_lane): a row of
// any slab is contiguous across the wave, so every access is coalesced, and the loads of kGaeRows rows are issued before
// the dependent chain over them starts.  No LDS, no barrier.
constexpr int kGaeBlock = 256, kGaeRows = 8;

__global__ __launch_bounds__(kGaeBlock) void gae_kernel(const float *__restrict__ reward, const float *__restrict__ values,
                                                        const float *__restrict__ last_value,
                                                        const uint8_t *__restrict__ done, const int32_t *__restrict__ actions,
                                                        int32_t T, int64_t N, float gamma, float lam,
                                                        float *__restrict__ adv, float *__restrict__ ret) {
    const int64_t i = (int64_t)blockIdx.x * kGaeBlock + threadIdx.x;
    if (i >= N) return;
    const auto rew = [&](int32_t t) { return reward[(int64_t)t * N + i]; };
    const auto val = [&](int32_t t) { return values[(int64_t)t * N + i]; };
    const auto term = [&](int32_t t) { return done[(int64_t)t * N + i] != 0; };
    const auto out = [&](int32_t t, float a, float r) { adv[(int64_t)t * N + i] = a; ret[(int64_t)t * N + i] = r; };
    if (actions) {
        const auto dead = [&](int32_t t) { return actions[(int64_t)t * N + i] < 0; };
        abrx::gae_lane<kGaeRows>(T, gamma, lam, last_value[i], rew, val, term, dead, out);
    } else {
        const auto dead = [](int32_t) { return false; };
        abrx::gae_lane<kGaeRows>(T, gamma, lam, last_value[i], rew, val, term, dead, out);
    }
}

extern "C" int abr_gae(const float *reward_dev, const float *values_dev, const float *last_value_dev,
                       const uint8_t *done_dev, const int32_t *actions_dev, int32_t n_steps, int64_t n_lanes, float gamma,
                       float lam, float *adv_out_dev, float *ret_out_dev, void *stream) {
    if (n_steps < 1) return fail(ABR_E_INVALID, "gae n_steps must be >= 1");
    if (n_lanes < 1) return fail(ABR_E_INVALID, "gae n_lanes must be >= 1");
    if (!reward_dev || !values_dev || !last_value_dev || !done_dev || !adv_out_dev || !ret_out_dev)
        return fail(ABR_E_INVALID, "gae NULL argument (reward, values, last_value, done, adv_out or ret_out)");
    if (((uintptr_t)reward_dev | (uintptr_t)values_dev | (uintptr_t)last_value_dev | (uintptr_t)actions_dev |
         (uintptr_t)adv_out_dev | (uintptr_t)ret_out_dev) & 3)
        return fail(ABR_E_INVALID, "gae float32 and int32 slabs must be 4-byte aligned");
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(ABR_E_INVALID, "gae gamma must be in [0, 1]");
    if (!(lam >= 0.0f && lam <= 1.0f)) return fail(ABR_E_INVALID, "gae lam must be in [0, 1]");
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n_lanes + kGaeBlock - 1) / kGaeBlock)), dim3(kGaeBlock), 0,
                       (hipStream_t)stream, reward_dev, values_dev, last_value_dev, done_dev, actions_dev, n_steps, n_lanes,
                       gamma, lam, adv_out_dev, ret_out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// ---------------------------------------------------------------------------
// The trace generator (include/abr_env.h: abr_trace_synth; abr_lane_jump.h: trace_map, trace_compose, trace_value)
// ---------------------------------------------------------------------------
// One wave per trace, the waves grid-stride over the traces; a wave walks its trace in tiles of 64 consecutive samples.  In
// a tile every lane computes its sample's philox block and state map, the wave scans the maps by composition (inclusive
// Hillis-Steele over distances 1..32) and lane l applies its prefix to the state the previous tile left: s_i without a
// serial chain over the samples.  A lane past the trace's end carries the identity map and takes part in every shuffle; the
// trip counts depend on the wave's trace alone, so no lane leaves before the last tile's scan.  A tile is one coalesced
// 512-byte store.  No LDS, no barrier: the model is the by-value argument, read with static indices only.
static_assert(sizeof(abr_trace_model) == sizeof(abrx::TraceModel) && sizeof(abr_trace_model) == 776 &&
              offsetof(abr_trace_model, level) == offsetof(abrx::TraceModel, level) &&
              offsetof(abr_trace_model, spread) == offsetof(abrx::TraceModel, spread) &&
              offsetof(abr_trace_model, outage_thr) == offsetof(abrx::TraceModel, outage_thr) &&
              offsetof(abr_trace_model, init_cum) == offsetof(abrx::TraceModel, init_cum) &&
              offsetof(abr_trace_model, cum) == offsetof(abrx::TraceModel, cum) &&
              ABR_TRACE_MAX_STATES == abrx::kTraceMaxStates, "abr_trace_model and abrx::TraceModel must agree");
constexpr int kTraceBlock = 256, kTraceWaves = kTraceBlock / 64;
constexpr int kTraceMaxBlocks = 2048;       // 8 192 waves, a little over the 7 168 that 256 CUs hold at this kernel's 7 waves per SIMD; more traces than that stride

__global__ __launch_bounds__(kTraceBlock) void trace_synth_kernel(abrx::TraceModel m, uint64_t key, uint32_t generation,
                                                                  int64_t id_base, double *__restrict__ traces,
                                                                  const int64_t *__restrict__ trace_off,
                                                                  const int32_t *__restrict__ trace_len, int32_t n_traces) {
    const int32_t lane = (int32_t)(threadIdx.x & 63u);
    const int64_t stride = (int64_t)gridDim.x * kTraceWaves;
    for (int64_t t = (int64_t)blockIdx.x * kTraceWaves + (threadIdx.x >> 6); t < n_traces; t += stride) {
        const int32_t len = trace_len[t];
        if (len < 1) continue;                                   // the same for every lane of the wave
        const uint64_t g = (uint64_t)(id_base + t);
        double *__restrict__ row = traces + trace_off[t];
        uint32_t w[4];
        abrx::philox4(key, g, abrx::kTraceInitStep, generation, w);
        uint32_t carry = abrx::trace_initial(m, w[0]);
        for (uint32_t base = 0; base < (uint32_t)len; base += 64) {      // unsigned: base + 64 cannot overflow for any int32 len
            const uint32_t i = base + (uint32_t)lane;
            const bool live = i < (uint32_t)len;
            abrx::philox4(key, g, i, generation, w);
            uint32_t F = live ? abrx::trace_map(m, w[0]) : abrx::kTraceIdentity;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)F, d, 64);
                F = lane >= d ? abrx::trace_compose(F, up) : F;
            }
            const uint32_t s = abrx::trace_apply(F, carry);
            if (live) row[i] = abrx::trace_value(m, s, w[1], w[2]);
            carry = (uint32_t)__shfl((int)s, 63, 64);
        }
    }
}

extern "C" int abr_trace_synth(const abr_trace_model *model, uint64_t seed, uint32_t generation, int64_t trace_id_base,
                               double *traces_dev, const int64_t *trace_off_dev, const int32_t *trace_len_dev,
                               int32_t n_traces, void *stream) {
    constexpr uint64_t kOne = 1ull << 32;
    if (!model) return fail(ABR_E_INVALID, "trace model is NULL");
    const int32_t K = model->n_states;
    if (K < 1 || K > ABR_TRACE_MAX_STATES) return fail(ABR_E_INVALID, "trace model n_states must be in 1..%d, got %d", ABR_TRACE_MAX_STATES, K);
    if (model->reserved_ != 0) return fail(ABR_E_INVALID, "trace model reserved_ must be 0");
    bool alive = false;
    for (int s = 0; s < K; s++) {
        if (!std::isfinite(model->level[s]) || model->level[s] < 0.0)
            return fail(ABR_E_INVALID, "trace model level[%d] must be finite and >= 0", s);
        alive = alive || (model->level[s] > 0.0 && model->outage_thr[s] < kOne);
    }
    if (!alive) return fail(ABR_E_INVALID, "trace model needs a state with level > 0 and outage_thr < 2^32: no sample could be positive");
    for (int s = 0; s < K; s++)
        if (!(model->spread[s] >= 0.0 && model->spread[s] <= 1.0))
            return fail(ABR_E_INVALID, "trace model spread[%d] must be in [0, 1]", s);
    // of a cumulative row only [0, K - 1) is read, here as in the kernel: the last value is 2^32 whatever the entry holds
    for (int s = 0; s < K; s++) {
        if (model->outage_thr[s] > kOne) return fail(ABR_E_INVALID, "trace model outage_thr[%d] is above 2^32", s);
        if (s < K - 1 && model->init_cum[s] > kOne) return fail(ABR_E_INVALID, "trace model init_cum[%d] is above 2^32", s);
        for (int j = 0; j < K - 1; j++)
            if (model->cum[s][j] > kOne) return fail(ABR_E_INVALID, "trace model cum[%d][%d] is above 2^32", s, j);
    }
    for (int j = 1; j < K - 1; j++)
        if (model->init_cum[j] < model->init_cum[j - 1]) return fail(ABR_E_INVALID, "trace model init_cum decreases at [%d]", j);
    for (int s = 0; s < K; s++)
        for (int j = 1; j < K - 1; j++)
            if (model->cum[s][j] < model->cum[s][j - 1]) return fail(ABR_E_INVALID, "trace model cum[%d] decreases at [%d]", s, j);
    if (!traces_dev || !trace_off_dev || !trace_len_dev)
        return fail(ABR_E_INVALID, "trace synth NULL argument (traces, trace_off or trace_len)");
    if ((((uintptr_t)traces_dev | (uintptr_t)trace_off_dev) & 7) || ((uintptr_t)trace_len_dev & 3))
        return fail(ABR_E_INVALID, "trace synth: traces and trace_off must be 8-byte aligned, trace_len 4-byte aligned");
    if (n_traces < 1) return fail(ABR_E_INVALID, "trace synth n_traces must be >= 1");
    if (trace_id_base < 0) return fail(ABR_E_INVALID, "trace synth trace_id_base must be >= 0");
    abrx::TraceModel m;
    memcpy(&m, model, sizeof(m));
    const int64_t blocks = ((int64_t)n_traces + kTraceWaves - 1) / kTraceWaves;
    hipLaunchKernelGGL(trace_synth_kernel, dim3((unsigned)(blocks < kTraceMaxBlocks ? blocks : kTraceMaxBlocks)),
                       dim3(kTraceBlock), 0, (hipStream_t)stream, m, seed ^ abrx::kTraceKey, generation, trace_id_base,
                       traces_dev, trace_off_dev, trace_len_dev, n_traces);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// Diagnostic: the exact chain (abr_exact_jump.h) on arbitrary inputs, one case per thread, so
// tests can compare the DEVICE build of the jump arithmetic -- v_rcp_f64 estimate, saturating
// convert, and (with a biased estimate) the out-of-line exact search -- with the naive loop.
template <int STOP, int BIAS>
__global__ void chain_debug_kernel(const double *__restrict__ x0, const double *__restrict__ c,
                                   const double *__restrict__ thr, const int32_t *__restrict__ n,
                                   int64_t count, double *__restrict__ x_out,
                                   int32_t *__restrict__ a_out, uint8_t *__restrict__ hit_out, int32_t proven) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double x = x0[i];
    int32_t a = 0;
    // proven: the form of the chains without per-segment guards (abr_exact_jump.h: GUARDS_PROVEN); the caller keeps to P1-P3
    const bool hit = proven ? abrx::chain<STOP, BIAS, abrx::SETTLE_REMAINDER, abrx::GUARDS_PROVEN>(x, c[i], thr[i], n[i], a)
                            : abrx::chain<STOP, BIAS>(x, c[i], thr[i], n[i], a);
    x_out[i] = x; a_out[i] = a; hit_out[i] = hit ? 1 : 0;
}

template <int STOP>
static int launch_chain_debug(int32_t bias, const double *x0, const double *c, const double *thr,
                              const int32_t *n, int64_t count, double *x_out, int32_t *a_out,
                              uint8_t *hit_out, hipStream_t st, int32_t proven) {
    const dim3 g((unsigned)((count + 63) / 64)), b(64);
    if (bias == 0) hipLaunchKernelGGL((chain_debug_kernel<STOP, 0>), g, b, 0, st, x0, c, thr, n, count, x_out, a_out, hit_out, proven);
    else if (bias == 4) hipLaunchKernelGGL((chain_debug_kernel<STOP, 4>), g, b, 0, st, x0, c, thr, n, count, x_out, a_out, hit_out, proven);
    else if (bias == -4) hipLaunchKernelGGL((chain_debug_kernel<STOP, -4>), g, b, 0, st, x0, c, thr, n, count, x_out, a_out, hit_out, proven);
    else return fail(ABR_E_INVALID, "estimate_bias must be 0, 4 or -4");
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

extern "C" int abr_debug_chain(int32_t stop_kind, int32_t estimate_bias, const double *x0_dev,
                               const double *c_dev, const double *thr_dev, const int32_t *n_dev,
                               int64_t count, double *x_out_dev, int32_t *a_out_dev,
                               uint8_t *hit_out_dev, void *stream) {
    if (!x0_dev || !c_dev || !thr_dev || !n_dev || !x_out_dev || !a_out_dev || !hit_out_dev)
        return fail(ABR_E_INVALID, "NULL device pointer");
    if (count < 1) return fail(ABR_E_INVALID, "count must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    // bit 8 of stop_kind: the proven form of the chains.  Its preconditions are the caller's (every budget in 1..2^20,
    // finite values); the budgets are not readable here (device memory), so they are not checked.
    const int32_t proven = (stop_kind & 0x100) ? 1 : 0;
    stop_kind &= ~0x100;
    switch (stop_kind) {
        case abrx::STOP_GE: return launch_chain_debug<abrx::STOP_GE>(estimate_bias, x0_dev, c_dev, thr_dev, n_dev, count, x_out_dev, a_out_dev, hit_out_dev, st, proven);
        case abrx::STOP_LE: return launch_chain_debug<abrx::STOP_LE>(estimate_bias, x0_dev, c_dev, thr_dev, n_dev, count, x_out_dev, a_out_dev, hit_out_dev, st, proven);
        case abrx::STOP_LT: return launch_chain_debug<abrx::STOP_LT>(estimate_bias, x0_dev, c_dev, thr_dev, n_dev, count, x_out_dev, a_out_dev, hit_out_dev, st, proven);
        default: return fail(ABR_E_INVALID, "stop_kind must be 0 (>=), 1 (<=) or 2 (<)");
    }
}

// Diagnostic: the contract the role-split kernels' fresh_params() rests on -- `EnvParams p` is the FIRST by-value kernel
// argument, so the block at offset 0 of the kernarg segment is this launch's parameter block -- checked in the PRODUCT build:
// instance <9> of each of the two kernel templates (the product instances' signature, a body that only answers) is launched
// once (one workgroup) with a sentinel in its parameter block and says whether fresh_params() saw it.  result_dev: uint32 [2]
// device memory, entry 0 = env_split3_kernel, 1 = env_split_kernel: 1 (seen) or 2 (not).  Touches no lane state.
extern "C" int abr_debug_selfcheck(abr_env *env, uint32_t *result_dev, void *stream) {
    if (!env || !result_dev) return fail(ABR_E_INVALID, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(result_dev, 0, 2 * sizeof(uint32_t), st));
    EnvParams p = env->p;
    p.sentinel = 0x5eed0000c0ffee00ull ^ (uint64_t)(uintptr_t)env;
    p.selfcheck_out = result_dev;
    hipLaunchKernelGGL(env_split3_kernel<9>, dim3(1), dim3(192), 0, st, p, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0ull,
                       abrx::EpisodeSampler{}, abrx::EpisodeLedger{}, abrx::EpisodeQuality{});
    p.selfcheck_out = result_dev + 1;
    hipLaunchKernelGGL(env_split_kernel<9>, dim3(1), dim3(128), 0, st, p, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0ull,
                       abrx::EpisodeSampler{}, abrx::EpisodeLedger{}, abrx::EpisodeQuality{});
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// Diagnostic: the drain of ONE subtrahend -- buffer_level -= speed*dt until <= 0 (Simulator.py:184, :194) -- as the kernels
// run it (abr_lane_jump.h: lanej_drain: the per-binade cascade, or the general chain for a wave that holds a value above
// it), one case per thread.
__global__ void drain_debug_kernel(abrx::DrainTab tab, double sd, const double *__restrict__ x0,
                                   const int32_t *__restrict__ n, int64_t count, double *__restrict__ x_out,
                                   int32_t *__restrict__ a_out, uint8_t *__restrict__ hit_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    abrx::Tables t;
    t.G = nullptr; t.interval_tick = nullptr; t.avail_tick = nullptr;
    t.L = 0.0; t.sd = sd; t.max_buffer = 0.0; t.start_up_length = 0.0; t.V = 0; t.max_ticks = 0;
    t.per_lane_speed = false; t.speed_rows = 0; t.speed_stride = 0; t.speeds = nullptr;
    t.drain = tab;
    double x = x0[i];
    int32_t a = 0;
    const bool zero = abrx::lanej_drain(t, x, sd, n[i], a);
    x_out[i] = x; a_out[i] = a; hit_out[i] = zero ? 1 : 0;
}

extern "C" int abr_debug_drain(double sd, double max_level, const double *x0_dev, const int32_t *n_dev, int64_t count,
                               double *x_out_dev, int32_t *a_out_dev, uint8_t *hit_out_dev, int32_t *stages_out,
                               void *stream) {
    if (!x0_dev || !n_dev || !x_out_dev || !a_out_dev || !hit_out_dev) return fail(ABR_E_INVALID, "NULL device pointer");
    if (count < 1) return fail(ABR_E_INVALID, "count must be >= 1");
    const abrx::DrainTab tab = abrx::make_drain_tab(sd, max_level);
    if (stages_out) *stages_out = tab.n;
    if (tab.n == 0) return fail(ABR_E_UNSUPPORTED, "no cascade for sd %g below %g: the kernels use the general chains", sd, max_level);
    hipLaunchKernelGGL(drain_debug_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, (hipStream_t)stream, tab, sd,
                       x0_dev, n_dev, count, x_out_dev, a_out_dev, hit_out_dev);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}

// Diagnostic: every combo evaluated from scratch by its own thread, literally as
// objective() does (mpc.py:120-162) -- no tables, no prefix sharing.  Used by the
// tests as an independent check of the DFS kernel's arithmetic.
__global__ void mpc_grid_kernel(int B, int H, int V, double L, double max_buffer, double wv,
                                double wr, int chunk, int prev, double buffer,
                                const double *__restrict__ pred, const double *__restrict__ br,
                                const double *__restrict__ sz, double *__restrict__ J_out,
                                int64_t total) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= total) return;
    int R[ABR_MAX_HORIZON + 1];
    {
        int64_t t = f;
        for (int i = H; i >= 1; i--) { R[i] = (int)(t % B); t /= B; }
        R[0] = prev < 0 ? prev + B : prev;     // Python's negative index (mpc.py:148)
    }
    double q = 0.0, v = 0.0, rb = 0.0, buf = buffer;
    for (int i = 0; i < H; i++) {
        const double *bri = br + (int64_t)(chunk + i) * B;
        const double *szi = sz + (int64_t)(chunk + i) * B;
        q += bri[R[i + 1]];
        v += fabs(bri[R[i + 1]] - bri[R[i]]);
        double m = 0.0;
        if (szi[R[i + 1]] > m) m = szi[R[i + 1]];
        if (L > m) m = L;
        rb += (m / pred[i] - buf);
        if (i != H - 1) {
            const double cs = sz[(int64_t)chunk * B + R[i + 1]];
            const double nb0 = pymax0(buf - cs / pred[i]);
            const double wait = pymax0(nb0 + L - max_buffer);
            buf = pymax0(nb0 + L - wait);
        }
    }
    J_out[f] = -((q - wv * v) - wr * rb);
    (void)V;
}

extern "C" int abr_mpc_objective_grid(const abr_mpc_config *cfg, int32_t chunk,
                                      int32_t prev_bitrate, double buffer_level,
                                      const double *pred_dev, const double *br_table_dev,
                                      const double *sz_table_dev, double *J_out_dev, void *stream) {
    int rc = validate_mpc(cfg);
    if (rc) return rc;
    if (!pred_dev || !br_table_dev || !sz_table_dev || !J_out_dev)
        return fail(ABR_E_INVALID, "NULL device pointer");
    if (prev_bitrate < -cfg->n_rates || prev_bitrate >= cfg->n_rates)
        return fail(ABR_E_INVALID, "previous_bitrate %d outside [-%d, %d) (mpc.py:148 raises IndexError)",
                    prev_bitrate, cfg->n_rates, cfg->n_rates);
    if (chunk < 0 || chunk + cfg->horizon > cfg->video_length)
        return fail(ABR_E_INVALID, "chunk %d + horizon %d exceeds video_length %d (mpc.py:126 raises)",
                    chunk, cfg->horizon, cfg->video_length);
    int64_t total = 1;
    for (int i = 0; i < cfg->horizon; i++) total *= cfg->n_rates;
    hipLaunchKernelGGL(mpc_grid_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, cfg->n_rates, cfg->horizon, cfg->video_length,
                       cfg->chunk_length, cfg->max_buffer, cfg->variance_weight,
                       cfg->rebuffer_weight, chunk, prev_bitrate, buffer_level, pred_dev,
                       br_table_dev, sz_table_dev, J_out_dev, total);
    HIP_TRY(hipGetLastError());
    return ABR_OK;
}
