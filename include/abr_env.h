/*
 * abr_env.h -- C ABI of the MI355X-native batched ABR environment and MPC lookahead.
 *
 * This is the drop-in boundary for the one hot path BASELINE.json names: the
 * tick loop of the reference's Simulator.run() (Simulator.py:135-208) and the
 * exhaustive lookahead of its MPCBitrateController (mpc.py:120-186), vectorised
 * over independent (trace, start-offset) lanes.
 *
 * The reference is pure Python with no FFI; its plugin boundary is inversion of
 * control: run() calls abr_controller.get_next_bitrate(chunk_id,
 * previous_bitrates, previous_bandwidths, buffer_level) once per chunk
 * (Simulator.py:155).  This ABI turns that inside out: abr_env_reset() runs each
 * lane up to its first get_next_bitrate() call site and hands back exactly the
 * call's arguments as the observation; abr_env_step(actions) supplies the return
 * value and runs to the next call site (or to simulation_end, Simulator.py:207).
 *
 * Conventions
 *  - Every function returns 0 on success or a negative ABR_E_* code; nothing
 *    throws across the boundary.  abr_last_error() gives the message of the
 *    calling thread's last failure.
 *  - Every *_dev pointer is device memory owned by the CALLER (the data_ptr()
 *    of a PyTorch-ROCm tensor).  The library allocates no device memory: its
 *    per-lane state and lookup tables live in the caller-provided workspace.
 *  - Work is only enqueued on the `stream` argument (a hipStream_t passed as
 *    void*; NULL = the default stream).  No call synchronises, except
 *    abr_env_create (one-time table upload).
 *  - Re-entrant per handle, no globals.  Lane arrays are struct-of-arrays with
 *    row stride n_lanes: field f of lane i is at base[f * n_lanes + i].
 */
#ifndef ABR_ENV_H
#define ABR_ENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: the workspace carries a LAYOUT TAG in its last 256 bytes (magic, ABI version, lane count, configuration, size), written by
 * abr_env_create; abr_env_notify_restore reads it back (it synchronises the device, once per restore) and answers
 * ABR_E_WORKSPACE when the restored bytes were laid out by another ABI version or for another lane count / configuration --
 * before this, such a workspace was reinterpreted with shifted offsets and no error.  abr_env_workspace_bytes grew by 256.
 * CHECKPOINTS DO NOT CARRY OVER: a workspace saved under version 2 or 3 cannot be restored (version 3 itself changed the lane
 * state -- ep_actions gone, a running variance sum added, 8 float64 state arrays -- without saying so; it has no tag and is
 * refused).  New diagnostic entry points: abr_debug_drain, abr_debug_selfcheck.  No existing signature changed.
 * 3: abr_env_has_impl (which implementations THIS build of the library carries: the product answers 0 for the rejected
 * pipelines 4, 6 and 7, which abr_env_set_impl refuses with ABR_E_UNSUPPORTED); under impl 3 (auto) a launch of ONE decision
 * resolves to 0 at every size (abr_env_get_effective_impl(fused = 0)); ABR_DONE_INTERNAL is reserved for the diagnostic
 * pipelines' watchdogs.  A version-2 host keeps working: nothing it could call changed its signature.
 * 2: abr_env_step_script, abr_env_get_effective_impl, abr_env_notify_restore, impl 5 (three waves per 64
 * lanes); struct abr_mpc_options GREW (mask_is_done + reserved_ appended: a version-1 host passes a
 * shorter struct and must be rebuilt); since 1 also: workspace layout grew, abr_env_set_lane_speeds /
 * _speed_schedule / _bitrate_table are latched until the next full reset, every re-reset advances the
 * policy's episode counter, default impl is 3 (auto).  A host built against version 1 must be rebuilt. */
#define ABR_ABI_VERSION 4
#define ABR_MAX_RATES 16
#define ABR_MAX_HORIZON 8

/* error codes */
#define ABR_OK 0
#define ABR_E_INVALID (-1)      /* bad argument / config */
#define ABR_E_WORKSPACE (-2)    /* workspace too small or misaligned */
#define ABR_E_HIP (-3)          /* a HIP runtime call failed */
#define ABR_E_UNSUPPORTED (-4)  /* valid in the reference, not built here (yet) */

/* per-lane bits of done_out */
#define ABR_DONE_EPISODE 0x1    /* chunk_id >= video_length  (Simulator.py:207-208) */
#define ABR_DONE_TIMEOUT 0x2    /* hit config.max_ticks before finishing */
#define ABR_DONE_BADACT 0x4     /* action outside [0, n_rates): lane frozen (the reference raises IndexError) */
#define ABR_DONE_BADARG 0x8     /* abr_env_reset got a trace id outside [0, n_traces) or a negative start
                                   offset for this lane: lane frozen, nothing read out of bounds */

#define ABR_DONE_INTERNAL 0x10  /* RESERVED: never set by the product library (the diagnostic asynchronous
                                   pipeline uses it for its watchdog) */

/* float32 observation rows written by reset/step: the four arguments of
 * get_next_bitrate (Simulator.py:155) first, then run() locals at that instant */
enum {
    ABR_OBS_CHUNK_ID = 0,       /* chunk_id                                   */
    ABR_OBS_LAST_BITRATE = 1,   /* previous_bitrates[-1] (index) or -1        */
    ABR_OBS_LAST_BANDWIDTH = 2, /* previous_bandwidths[-1] or 0 (:164)        */
    ABR_OBS_BUFFER_LEVEL = 3,   /* buffer_level [s]                           */
    ABR_OBS_GLOBAL_TIME = 4,    /* global_time [s]                            */
    ABR_OBS_PLAY_TIME = 5,      /* play_time [s]                              */
    ABR_OBS_REBUFFER_TIME = 6,  /* rebuffer_time, cumulative [s]              */
    ABR_OBS_STARTUP_TIME = 7,   /* start_up_time, cumulative [s]              */
    ABR_OBS_DIM = 8
};

/* float64 rows of abr_env_observe_f64: everything the oracle records */
enum {
    ABR_F64_GLOBAL_TIME = 0, ABR_F64_REBUFFER_TIME, ABR_F64_STARTUP_TIME, ABR_F64_PLAY_TIME,
    ABR_F64_AVERAGE_LATENCY, ABR_F64_BUFFER_LEVEL, ABR_F64_PLAY_LENGTH, ABR_F64_LAST_BANDWIDTH,
    ABR_F64_CHUNK_ID, ABR_F64_PLAY_ID, ABR_F64_LAST_BITRATE, ABR_F64_FLAGS /* start_up | buffer_empty<<1 | buffer_full<<2 */,
    ABR_F64_HIST_N, ABR_F64_HIST_SUM_INV, ABR_F64_TICK, ABR_F64_DOWNLOAD_TIME,
    ABR_F64_DIM
};

/* Replaces: MPD (Simulator.py:11-17), QOEMetric (:19-24), NetworkInfo.interval
 * (:39-42), the single-ladder Chunk that run() indexes (:82,156), and the
 * constant a speed controller would return (:177; none ships, D8). */
typedef struct abr_env_config {
    int32_t n_rates;            /* len(mpd.chunks.bitrates), 1..ABR_MAX_RATES */
    int32_t video_length;       /* mpd.video_length [chunks]                  */
    double  chunk_length;       /* mpd.chunk_length [s]                       */
    double  max_buffer;         /* mpd.max_buffer (compared in seconds, :190) */
    double  start_up_length;    /* mpd.start_up_length [s]                    */
    double  interval;           /* network_info.interval [s]                  */
    double  rebuffer_weight;    /* qoe_metric.*                               */
    double  variance_weight;
    double  startup_weight;
    double  latency_weight;
    double  speed;              /* play_speed, constant                       */
    double  ladder[ABR_MAX_RATES];
    int32_t max_ticks;          /* per-episode bound on 0.01 s ticks; <=0: 32 * V * ceil(L/dt) */
    int32_t auto_reset;         /* !=0: a lane that finishes is re-armed inside the step (same trace, same
                                   offset; with an episode sampler installed, the sampler's pair for the new
                                   episode); the obs returned is the new episode's first */
} abr_env_config;

typedef struct abr_env abr_env;   /* opaque host-side handle */

int  abr_abi_version(void);
const char *abr_last_error(void);

/* Bytes of device workspace (256-B aligned) abr_env_create needs for n_lanes. */
int abr_env_workspace_bytes(const abr_env_config *cfg, int64_t n_lanes, size_t *bytes_out);

/*
 * Replaces Simulator.__init__/set_qoe_metric/set_network_info/set_mpd
 * (Simulator.py:46-77).  traces_dev: all bandwidth traces back to back
 * (float64, same unit as the ladder); trace t is traces_dev[trace_off_dev[t] ..
 * + trace_len_dev[t]).  The three trace arrays must outlive the handle.
 * Builds the universal tick tables on the host in float64 (the reference's
 * global_time is lane-independent) and uploads them into the workspace.
 *
 * What a trace may contain: every sample finite and >= 0 (0.0, -0.0 and subnormal values included), every
 * trace at least one sample long (trace_len_dev[t] >= 1, n_traces >= 1).  A lane that plays past the end of
 * its trace wraps to the trace's start (build-defined: the reference raises); a trace of one sample wraps
 * at every interval.  A zero sample is an outage: the download makes no progress in that interval.  A lane
 * on a trace without a positive sample never completes a chunk and ends with ABR_DONE_TIMEOUT at
 * config.max_ticks, one addition per tick -- a bounded crawl, not a hang; lanes of the same wave on live
 * traces are not affected.  The library never reads the traces on the host, so it cannot refuse a NaN, an
 * infinite or a negative sample: those are outside the contract, and a binding checks for them itself, as
 * abrsimulator_amd.env.pack_traces does.  Covered by tests/test_trace_edges_{cpu,gpu}.py.
 */
int abr_env_create(const abr_env_config *cfg, const double *traces_dev,
                   const int64_t *trace_off_dev, const int32_t *trace_len_dev, int32_t n_traces,
                   int64_t n_lanes, void *workspace_dev, size_t workspace_bytes, void *stream,
                   abr_env **env_out);
int abr_env_destroy(abr_env *env);

/* When the lanes of this handle are a shard of a larger job: global id of lane 0,
 * used only as the counter of the built-in random policy so that a sharded run
 * reproduces the unsharded one.  Default 0. */
int abr_env_set_lane_id_base(abr_env *env, int64_t lane_id_base);

/* One constant play speed per lane instead of config.speed (what a per-lane speed
 * controller that always answers the same value would do, Simulator.py:176-177).
 * speeds_dev: float64 [n_lanes], > 0, must stay valid from this call until the handle is
 * destroyed or another call replaces it.  The pointer is LATCHED: running episodes keep the
 * speeds they started with; the next abr_env_reset picks the new ones up, and that reset must
 * cover all lanes (lane_mask_dev == NULL, else ABR_E_INVALID).  On a handle that has seen neither
 * abr_env_reset nor abr_env_notify_restore there is no episode to protect and the call takes
 * effect at once.  NULL restores the single speed.  Event-driven kernels only: ABR_E_UNSUPPORTED on
 * impl 1, and abr_env_set_impl(1) refuses while per-lane speeds are in force or pending. */
int abr_env_set_lane_speeds(abr_env *env, const double *speeds_dev);   /* latched: see above */

/* What a speed controller answers, call by call (Simulator.py:176-177: get_next_speed() is
 * asked at the first playing tick of every played chunk, i.e. whenever play_length == 0).
 * speeds_dev: float64 [n_rows][n_lanes]; the p-th played chunk of lane i plays at
 * speeds_dev[min(p, n_rows - 1) * n_lanes + i] (the last row repeats).  p counts the played chunks
 * of the lane's current episode: every reset of the lane (masked or not) and every auto_reset
 * re-arm starts it again at row 0.  n_rows == 1 is abr_env_set_lane_speeds.  Same lifetime and
 * latching rules.  Event-driven kernels only. */
int abr_env_set_speed_schedule(abr_env *env, const double *speeds_dev, int32_t n_rows);

/* A closed-loop speed controller (ABI 4, additive; BUILD-DEFINED: the reference ships no speed
 * controller, D8).  A stateless, piecewise-constant table, comparisons only, evaluated on the device
 * exactly where the reference calls get_next_speed() (Simulator.py:176-177: the first playing tick of
 * every played chunk, play_length == 0).  At that tick of played chunk p:
 *   lat = global_time - play_time   float64 G[k] - pt, pt before this tick's += speed*dt: the
 *                                   reference's instant_latency (:179)
 *   buf = buffer_level              after this tick's += chunk_length when a download completes on it
 *                                   (:170), before its -= speed*dt (:184)
 *   i   = number of q < n_lat with lat >= lat_thr[q]
 *   j   = number of r < n_buf with buf >= buf_thr[r]
 * and the chunk plays at speed[i][j].  Everything after that -- the chunk's length in ticks,
 * play_time, the drains, average_latency -- is the speed schedule's path (abr_env_set_speed_schedule).
 * Fields: n_lat, n_buf in 0..4; lat_thr[0..n_lat) and buf_thr[0..n_buf) finite and strictly ascending
 * [s]; speed[0..n_lat][0..n_buf] finite and > 0.  Entries past those counts are ignored. */
#define ABR_SPEED_RULE_MAX_THR 4
typedef struct abr_speed_rule {
    int32_t n_lat, n_buf;
    double  lat_thr[ABR_SPEED_RULE_MAX_THR];                               /* [s] */
    double  buf_thr[ABR_SPEED_RULE_MAX_THR];                               /* [s] */
    double  speed[ABR_SPEED_RULE_MAX_THR + 1][ABR_SPEED_RULE_MAX_THR + 1]; /* [i][j] */
} abr_speed_rule;                                                          /* 272 bytes */

/* Install a speed rule.  It and abr_env_set_lane_speeds / _speed_schedule are mutually exclusive: the
 * last call wins; rule == NULL restores config.speed.  Latched like abr_env_set_speed_schedule (the next
 * reset of ALL lanes adopts it; at once on a handle with no episode in flight).  The rule is copied by
 * value: the caller's struct may go right after the call.  speed_log_dev: NULL, or caller-owned float64
 * [log_rows][n_lanes] (same lifetime rules as speeds_dev above): row p receives the speed answered for
 * played chunk p of the lane's current episode, for p < log_rows; rows never reached keep what they
 * held.  A reset of the lane (masked or not) and an auto_reset re-arm start its log over at row 0, so
 * the rows past the current episode's last answer hold what earlier episodes wrote there.  A bad field (or log_rows < 0, or log_rows > 0 without a log) is ABR_E_INVALID before anything is
 * stored, and the struct is checked before the handle.  Impl 0, 2, 3 and 5 only: ABR_E_UNSUPPORTED on 1 (tick) and
 * on the diagnostic pipelines 4, 6 and 7, and abr_env_set_impl refuses those while a rule is set or pending. */
int abr_env_set_speed_rule(abr_env *env, const abr_speed_rule *rule, double *speed_log_dev, int32_t log_rows);

/* Per-chunk bitrate ladders: br_table_dev float64 [video_length][n_rates], caller-owned, valid
 * from this call until the handle is destroyed or another call replaces it; NULL restores
 * config.ladder.  This is the evident intent of set_mpd's one-ladder-per-line file
 * (Simulator.py:71-76), which run() itself cannot consume (it indexes a single Chunk,
 * Simulator.py:82,156, and raises AttributeError on the list) -- so it is BUILD-DEFINED:
 * target_size = br[chunk_id][action] * chunk_length, and the variance term of calculate_qoe
 * (and of the per-step reward) is |br[i][a_i] - br[i+1][a_(i+1)]|, each bitrate from its own
 * chunk's ladder.  Latched like abr_env_set_lane_speeds: picked up by the next reset of ALL lanes. */
int abr_env_set_bitrate_table(abr_env *env, const double *br_table_dev);

/* Per-chunk SIZES (ABI 4, additive; BUILD-DEFINED: run() knows bitrate x chunk_length only): variable-bitrate video, where
 * a rung is a nominal quality and its chunks weigh more or less with the scene.  sz_table_dev: float64
 * [video_length][n_rates], caller-owned device memory, valid from this call until the handle is destroyed or another call
 * replaces it; unit: the ladder's unit x seconds, what abr_mpc_select's sz_table_dev holds.  NULL restores bitrate x
 * chunk_length.  The size table decides WHAT IS DOWNLOADED; the bitrate table (or config.ladder) keeps deciding WHAT IS
 * SCORED.  Below, br(c, a) is the abr_env_set_bitrate_table row, else config.ladder, and sz(c, a) this table.
 *   The one change: at a call site with chunk c and action a, target_size = sz(c, a) in place of br(c, a) *
 *     chunk_length (Simulator.py:156).  The bandwidth appended to previous_bandwidths is, as ever, the downloaded size over
 *     the download time (:164).
 *   Nothing that reads a bitrate changes: the variance term of the reward and of abr_env_episode_qoe, the episode
 *     ledger's record, the quality model's u, observation row 1 and abr_mpc_* keep reading br.
 *   Coverage: every launch kind on implementations 0, 1, 2, 3 and 5.  The diagnostic pipelines 4, 6 and 7 refuse a launch
 *     with a size table (ABR_E_UNSUPPORTED), as they do a sampler.
 *   Tree walks: abr_env_lookahead_select, abr_env_plan_select and abr_env_step_plan walk with sz(chunk, a) as each step's
 *     target; their variance keeps br.
 *   Rules: ABR_RULE_RATE and ABR_RULE_BOLA compare and divide by what a chunk costs to fetch: while a size table is in
 *     force their br[m] is e[m] = sz(c, m) / chunk_length, one float64 division, nothing else.  ABR_RULE_BUFFER is
 *     untouched (its map lives on the nominal ladder), and so is FastMPC's lookup (its table was built from the caller's sz).
 *   Learned policy (all four engines, both populations): while a size table is in force features 4 + W + m are sz(c, m) in
 *     place of br(c, m) -- the sizes of the next chunk.  F, feature 1 (br(c - 1, a)), norm_dev and everything downstream
 *     are unchanged.
 *   abr_env_fork needs nothing: there is no per-lane state.
 * Latched exactly like abr_env_set_bitrate_table: the next abr_env_reset of all lanes adopts it, a masked reset while one is
 * pending is ABR_E_INVALID, on a handle with no episode in flight it takes effect at once, and abr_env_notify_restore expects
 * the same table to be set.  A handle with a size table runs the kernels' general instances (abr_env_get_effective_impl).
 * Values must be finite, > 0 and below 2^960.  The library never reads the table on the host, so it cannot refuse a value
 * outside that range: this is the caller's promise, as for the traces and the bitrate table, and a binding checks it
 * itself, as abrsimulator_amd.env.BatchedABREnv does.  NULL handle: ABR_E_INVALID. */
int abr_env_set_size_table(abr_env *env, const double *sz_table_dev);

/* Resume: the whole simulator state is the workspace, so a checkpoint is a copy of it.  After copying
 * a checkpointed workspace into the workspace of a handle built with the same config, lane count
 * and (already set) speeds / bitrate table / size table, call this: it marks the handle as carrying episodes in
 * flight, so that later setter calls are latched again.  It first reads the workspace's layout tag back
 * (ABI 4; one device synchronisation) and returns ABR_E_WORKSPACE -- the handle then stays as it was, the
 * workspace holds the foreign bytes and must be re-initialised by abr_env_reset of all lanes or restored
 * again -- if the bytes were laid out by another ABI version, lane count or configuration. */
int abr_env_notify_restore(abr_env *env);

/* Which kernels serve reset/step: 2 = event-driven (exact closed-form stepping of the
 * float64 tick sequences) with each lane's download side and player side on two waves of one
 * workgroup; 0 = event-driven, one thread per lane; 1 = one loop trip per 0.01 s tick;
 * 5 = as 2 with a third wave per 64 lanes for the service tail of a decision (bandwidth = size /
 * time, history, reward, observation, episode end);
 * 3 (default) = whichever is fastest at this size: 5 up to 65 536 lanes, 2 up to 131 072 lanes,
 * 0 above -- and 0 at every size for launches of ONE decision (abr_env_step, the per-decision
 * launches of abr_env_step_mpc, a fused call with n_steps == 1).
 * 0, 2 and 5 produce identical state and outputs in every case (the workspace is interchangeable between them, also
 * mid-episode).  1 is an independent cross-check: it agrees with them on every lane that ends its episode, but it visits
 * ticks in blocks, so a lane that runs into max_ticks (ABR_DONE_TIMEOUT -- build-defined: the reference has no time-out)
 * is frozen at its block boundary: same done bits, different frozen counters in that lane's last observation.
 * 4 (the asynchronous pipeline of round 3), 6 (the ring-coupled role pipeline of round 5) and 7 (round 5: download and player
 * wave in lock-step through LDS counters, the service wave behind a ring) were measured slower than -- or, 7, within 1 % of --
 * what 3 selects and are not in the product library: ABR_E_UNSUPPORTED, see abr_env_has_impl. */
int abr_env_set_impl(abr_env *env, int32_t impl);

/* 1 if this build of the library can run implementation `impl` (0..7), else 0.  The product library: 0, 1, 2, 3, 5. */
int abr_env_has_impl(int32_t impl);

/* The implementation (0, 1, 2 or 5; never 3) the handle resolves to right now: fused != 0 for
 * abr_env_step_random / abr_env_step_script with more than one decision per call, 0 for launches of
 * one decision (abr_env_step, abr_env_step_mpc, n_steps == 1).  `fused` is 0 or 1; with 2 added to it, 0x100 is added to
 * the answer when the handle's step launches run the kernels' general instances (the form with the per-lane play-speed code
 * and the per-segment chain guards) and not the slimmer no-speeds ones: while a speed feature is latched, a sampler or a
 * quality model is installed, a size table (abr_env_set_size_table) is in force or pending, or the configuration fails the host's proof for the unguarded chains (a trace interval
 * shorter than one 0.01 s tick, max_ticks above 2^20, a non-finite or absurd ladder x chunk_length, speed or max_buffer). */
int abr_env_get_effective_impl(abr_env *env, int32_t fused, int32_t *impl_out);

/*
 * run() state init (Simulator.py:95-133) plus the idle ticks up to the first
 * get_next_bitrate call site.  Lane i uses trace trace_id_dev[i]; its
 * bandwidths[idx] is trace[(start_offset_dev[i] + idx) % len] (D7: wrap is
 * build-defined).  lane_mask_dev (nullable): only lanes with a non-zero byte
 * are reset.  obs_out_dev: float32 [ABR_OBS_DIM][n_lanes] (nullable).
 * A lane whose trace id is outside [0, n_traces) or whose start offset is negative is
 * frozen with ABR_DONE_BADARG (the reference would raise IndexError at Simulator.py:159).
 * Every reset of a lane after its first starts the next episode number of the built-in
 * counter-based policy (abr_env_step_random), so repeated episodes draw fresh actions.
 * trace_id_dev == NULL (with start_offset_dev == NULL) is accepted only while an episode sampler is
 * installed: each reset lane then runs the sampler's pair for its new episode number.
 */
int abr_env_reset(abr_env *env, const int32_t *trace_id_dev, const int32_t *start_offset_dev,
                  const uint8_t *lane_mask_dev, float *obs_out_dev, void *stream);

/*
 * One chunk decision per lane: actions_dev[i] is what get_next_bitrate would
 * have returned (Simulator.py:155); the lane then runs ticks T4..T9 and on,
 * to its next call site or to simulation_end.  reward_out_dev[i] =
 *   wr * d(rebuffer_time) + ws * d(start_up_time) + wv * |br[a] - br[a_prev]|
 * (the per-step split of calculate_qoe, Simulator.py:79-86; the first step's
 * deltas start from 0, so sum(reward) + wl * average_latency == run()'s return).
 * Lanes already done are left untouched and report their done bits again.
 */
int abr_env_step(abr_env *env, const int32_t *actions_dev, float *obs_out_dev,
                 float *reward_out_dev, uint8_t *done_out_dev, void *stream);

/*
 * Episode sampler (ABI 4, additive; BUILD-DEFINED: the reference runs one trace from one offset per run()).  Under
 * auto_reset a lane that ends with ABR_DONE_EPISODE is re-armed inside the launch on a (trace, start offset) pair drawn on
 * the device instead of its previous one.  The assignment of episode e of global lane g = lane_id_base + i is a pure
 * function (abr_lane_jump.h: episode_assign):
 *   w[0..3] = philox4x32-10(key = seed, ctr = (g lo, g hi, 0xFFFFFFFF, (uint32)e))
 *   u       = ((uint64)w0 * n) >> 32            n = n_pool with a pool, else n_traces
 *   t       = pool ? pool[u] : u
 *   span    = offset_span > 0 ? min(offset_span, trace_len[t]) : trace_len[t]
 *   offset  = ((uint64)w1 * span) >> 32
 * The counter step 0xFFFFFFFF is never a chunk id: no draw of abr_env_step_random or of the policy's exploration shares it.
 * e is the lane's episode number (abr_env_get_episode): 0 after the first reset of a fresh lane, +1 at every later reset and
 * at every re-arm.  The draw is keyed by the global lane id, so shards (abr_env_set_lane_id_base) see the unsharded lanes'
 * sequences.  Lanes that end with ABR_DONE_TIMEOUT are not re-armed, with or without a sampler.
 *
 * abr_env_set_episode_sampler copies the struct (s == NULL: sampling off).  Refused with ABR_E_INVALID before anything is
 * stored: a pool with n_pool < 1, offset_span < 0, then (after the handle is checked) a pool id outside [0, n_traces) -- the
 * pool is read back once to be checked (one device synchronisation).  pool is caller-owned device memory that must stay
 * valid and unchanged while the sampler is installed.  The sampler takes effect at the next re-arm or sampled reset; nothing
 * is latched.  abr_env_reset with trace_id_dev == NULL and start_offset_dev == NULL while a sampler is installed draws each
 * reset lane's pair for its new episode number (lane_mask_dev still applies).  Every launch kind and implementation
 * honours it (0, 1, 2, 3, 5); the diagnostic pipelines 4, 6 and 7 refuse a launch with a sampler (ABR_E_UNSUPPORTED).
 */
typedef struct abr_episode_sampler {
    uint64_t seed;
    const int32_t *pool;        /* nullable: device int32 [n_pool] trace ids; NULL = every trace */
    int32_t n_pool;
    int32_t offset_span;        /* >= 0; 0 = the whole trace */
} abr_episode_sampler;          /* 24 bytes */
int abr_env_set_episode_sampler(abr_env *env, const abr_episode_sampler *s);

/* Each lane's current episode: trace id, start offset (as given to abr_env_reset, or drawn) and episode number, int32
 * [n_lanes] device memory each, all nullable; copies enqueued on the stream. */
int abr_env_get_episode(abr_env *env, int32_t *trace_id_out_dev, int32_t *offset_out_dev, int32_t *episode_out_dev,
                        void *stream);

/*
 * n_steps fused decisions per lane with the built-in random policy
 * action = philox4x32-10(key=seed, ctr=(lane, episode_step, episode_no, 0)) % n_rates.
 * Outputs (all nullable) are [n_steps][...] slabs: obs [n_steps][ABR_OBS_DIM][n_lanes],
 * reward/done/actions [n_steps][n_lanes].  Lane state is read and written once per call.  Under the one-thread-per-lane
 * kernels (impl 0) lanes progress independently; the role-split kernels (impl 2 / 5) meet at ONE workgroup barrier per
 * decision (64 lanes, two or three waves), which is what `auto` prefers up to 131 072 lanes.
 */
int abr_env_step_random(abr_env *env, int32_t n_steps, uint64_t seed, float *obs_out_dev,
                        float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                        void *stream);

/*
 * n_steps fused decisions per lane whose actions are given up front: actions_dev int32
 * [n_steps][n_lanes], actions_dev[s][i] = what get_next_bitrate returns at the s-th call site
 * lane i reaches in this call (Simulator.py:155 with a scripted abr_controller).  Outputs as
 * abr_env_step_random.  A lane whose scripted action is outside [0, n_rates) is frozen with
 * ABR_DONE_BADACT at that step, as in abr_env_step.
 */
int abr_env_step_script(abr_env *env, int32_t n_steps, const int32_t *actions_dev, float *obs_out_dev,
                        float *reward_out_dev, uint8_t *done_out_dev, void *stream);

/* calculate_qoe (Simulator.py:79-86) in the reference's operation order from the
 * lane's action history; meaningful for lanes whose episode is complete (with
 * auto_reset: the last completed episode).  qoe_out_dev: float64 [n_lanes].
 * An episode cut by a masked reset is never complete: with auto_reset the answer stays the last
 * completed episode's; without it the variance term reads the action history, which the new
 * episode overwrites as it goes, so the answer is meaningful again once that episode has ended. */
int abr_env_episode_qoe(abr_env *env, double *qoe_out_dev, void *stream);

/*
 * Episode ledger (ABI 4, additive; BUILD-DEFINED).  abr_env_episode_qoe answers for a lane's LAST finished episode only,
 * and the per-step reward leaves the latency term out: a fused launch that finishes several episodes per lane keeps one.
 * While a ledger is installed, every env kernel appends one record per finished episode to a caller-owned blob.
 *
 * THE RULE: a record is appended exactly when the kernels write the episode's QoE terms (what abr_env_episode_qoe reads):
 * at the step at which a lane's episode ends with ABR_DONE_EPISODE or ABR_DONE_TIMEOUT, in every launch kind
 * (abr_env_step, _step_random, _step_script, _step_rule, _step_fastmpc, _step_mpc, _step_mpc_robust, _step_policy,
 * _step_policy_sampled, _step_policy_ac) on every implementation that accepts it (0, 1, 2, 3, 5).  Hence: a lane frozen by
 * ABR_DONE_BADACT / ABR_DONE_BADARG appends nothing; an episode abandoned by a (masked) abr_env_reset appends nothing; a
 * timed-out lane appends one record, once (later launches leave a done lane untouched); and a lane that runs out of ticks
 * BEFORE its new episode's first call site (a reset or a re-arm that ends in ABR_DONE_TIMEOUT without a single decision)
 * appends nothing for that episode either, because no QoE terms are written for it.
 *
 * The blob, abr_env_ledger_bytes(n_lanes, rows) bytes at a 256-byte aligned address: struct-of-arrays with row stride
 * n_lanes; every region starts at the next multiple of 256 bytes after the previous one, in this order:
 *   count   int32   [n_lanes]            episodes recorded for the lane since the blob was zeroed (< 2^31)
 *   total   float64 [5][n_lanes]         running sums over ALL recorded episodes of the lane, added in episode order
 *   rec_f64 float64 [rows][5][n_lanes]   the five float fields of the record in each ring slot
 *   rec_i32 int32   [rows][5][n_lanes]   the five int fields of the record in each ring slot
 * float fields: 0 rebuffer_time, 1 start_up_time, 2 average_latency, 3 variance (sum of |bitrate steps|), 4 qoe, where
 *   qoe = wr * rebuffer_time + wv * variance + ws * start_up_time + wl * average_latency
 * in that order (abr_env_episode_qoe's), so a lane's newest record's qoe equals abr_env_episode_qoe bit for bit.
 * int fields: 0 the lane's episode number while the episode ran (abr_env_get_episode), 1 its trace id, 2 its start offset
 * (the FINISHED episode's pair, not the re-armed one's), 3 chunks downloaded (chunk_id at the end: video_length unless
 * timed out), 4 the done byte (ABR_DONE_EPISODE or ABR_DONE_TIMEOUT).
 * A record goes to slot count % rows, then count is incremented: the ring keeps the lane's last min(count, rows) episodes,
 * the totals keep all of them.  An all-zero blob is an empty ledger; the caller clears it by zeroing it, on the stream
 * the launches run on.  abr_env_reset does not touch it.  It is not part of the workspace (layout and checkpoints unchanged).
 *
 * abr_env_ledger_bytes is pure arithmetic: it needs no handle and no device.  ABR_E_INVALID: n_lanes < 1, rows < 1, NULL
 * bytes_out.  abr_env_set_episode_ledger copies the struct (l == NULL: off; the next launch appends nothing).  Refused
 * with ABR_E_INVALID before anything is stored: rows < 1, base_dev NULL or not 256-byte aligned.  base_dev must stay valid
 * while installed, and must have been sized for this handle's n_lanes.  The diagnostic pipelines 4, 6 and 7 refuse a
 * launch with a ledger (ABR_E_UNSUPPORTED), as they do a sampler.
 */
typedef struct abr_episode_ledger {
    void   *base_dev;           /* caller-owned, 256-B aligned, >= abr_env_ledger_bytes(); all-zero bytes = empty ledger */
    int32_t rows;               /* ring slots per lane, >= 1 */
    int32_t reserved_;          /* 0 */
} abr_episode_ledger;           /* 16 bytes */
int abr_env_ledger_bytes(int32_t n_lanes, int32_t rows, size_t *bytes_out);
int abr_env_set_episode_ledger(abr_env *env, const abr_episode_ledger *l);

/*
 * Quality model (ABI 4, additive; BUILD-DEFINED: the reference's calculate_qoe has no such term, its MPC's objective has --
 * mpc.py:146).  The reward and the episode QoE above are pure costs, which "lowest bitrate, always" minimises.  While a
 * quality model is installed the env kernels also score what was watched: a weight wq, a caller-owned device table u,
 * float64 [video_length][n_rates], computed by the caller (no device log, as abr_rule_config.utility_dev), and a
 * caller-owned blob.
 *
 * PER STEP.  At a step whose download completed -- the step that appends to previous_bandwidths / previous_bitrates --
 * with c the downloaded chunk and a the action:  q = u[c][a];  q_run[i] = q_run[i] + q;  and the step's reward is
 * (float)(rew - wq * q), where rew is the float64 reward expression without a model, in its order: then one multiply, one
 * subtract, one rounding to float32, never fused.  The reward stays a cost: quality lowers it.  A step without a completed
 * download (ABR_DONE_BADACT; a time-out in mid-download) adds nothing and reports the reward it reports without a model.
 *
 * PER EPISODE.  The blob follows the episode ledger's RULE: it is written exactly when the kernels write the episode's QoE
 * terms (ABR_DONE_EPISODE or ABR_DONE_TIMEOUT, every launch kind, implementations 0, 1, 2, 3, 5).  With Q = q_run[i]:
 *   q_last[i] = Q;  rec_q[count[i] % rows][i] = Q;  total_q[i] = total_q[i] + Q;  count[i] = count[i] + 1;
 * and, if the lane is re-armed at that step (auto_reset, ABR_DONE_EPISODE), q_run[i] = 0.0.  abr_env_reset sets q_run of
 * the lanes it resets (all, or the masked ones) to 0.0 and touches nothing else of the blob.
 *
 * The blob, abr_env_quality_bytes(n_lanes, rows) bytes at a 256-byte aligned address: struct-of-arrays with row stride
 * n_lanes; every region starts at the next multiple of 256 bytes after the previous one, in this order:
 *   count   int32   [n_lanes]         episodes recorded for the lane since the blob was zeroed
 *   q_run   float64 [n_lanes]         the running sum of the episode in flight (mid-episode state)
 *   q_last  float64 [n_lanes]         the sum of the lane's last finished episode
 *   total_q float64 [n_lanes]         running sum over ALL recorded episodes of the lane, added in episode order
 *   rec_q   float64 [rows][n_lanes]   the sum of the record in each ring slot
 * An all-zero blob is empty.  It keeps its own count, so it needs no ledger; cleared together with a ledger of the same
 * rows, the slots of the two coincide.  The ledger's layout, its qoe field and abr_env_episode_qoe are what they are without
 * a model, bit for bit: the combined figure is qoe - wq * Q, formed by whoever reads both.
 *
 * abr_env_quality_bytes is pure arithmetic (ABR_E_INVALID: n_lanes < 1, rows < 1, NULL bytes_out).
 * abr_env_set_episode_quality copies the struct (q == NULL: off).  Refused with ABR_E_INVALID before anything is stored: wq
 * not finite, u_dev NULL or not 8-byte aligned, base_dev NULL or not 256-byte aligned, rows < 1.  The table's values are
 * the caller's: a NaN in u propagates.  u_dev and base_dev must stay valid while installed.  abr_env_episode_quality copies
 * q_last to q_out_dev, float64 [n_lanes], on the stream (ABR_E_INVALID without a model).  The diagnostic pipelines 4, 6
 * and 7 refuse a launch with a quality model (ABR_E_UNSUPPORTED), as they do a ledger.
 */
typedef struct abr_episode_quality {
    double        wq;           /* finite */
    const double *u_dev;        /* caller-owned device float64 [video_length][n_rates] */
    void         *base_dev;     /* caller-owned, 256-B aligned, >= abr_env_quality_bytes(); all-zero bytes = empty */
    int32_t       rows;         /* ring slots per lane, >= 1 */
    int32_t       reserved_;    /* 0 */
} abr_episode_quality;          /* 32 bytes */
int abr_env_quality_bytes(int32_t n_lanes, int32_t rows, size_t *bytes_out);
int abr_env_set_episode_quality(abr_env *env, const abr_episode_quality *q);
int abr_env_episode_quality(abr_env *env, double *q_out_dev, void *stream);

/* Full float64 observation, [ABR_F64_DIM][n_lanes]. */
int abr_env_observe_f64(abr_env *env, double *out_dev, void *stream);

/* Device pointers into the workspace for consumers that need exact float64
 * state (the MPC adapter) or want to checkpoint it. */
typedef struct abr_env_state_view {
    int64_t n_lanes;
    const int32_t *chunk_id;      /* [n_lanes] */
    const int32_t *last_bitrate;  /* [n_lanes], -1 before the first chunk */
    const double  *buffer_level;  /* [n_lanes] */
    double        *hist_n;        /* [n_lanes] len(previous_bandwidths), as float64 */
    double        *hist_sum_inv;  /* [n_lanes] sum(1/x for x in previous_bandwidths), list order */
    const uint8_t *done;          /* [n_lanes] ABR_DONE_* bits */
    const uint8_t *action_hist;   /* [video_length][n_lanes] previous_bitrates */
    const double  *bw_hist;       /* [video_length][n_lanes] previous_bandwidths */
} abr_env_state_view;
int abr_env_get_state(abr_env *env, abr_env_state_view *view_out);

/*
 * Lane fork (ABI 4, additive; BUILD-DEFINED: the reference runs one player).  All lane state between launches is the
 * workspace, shared bit for bit by every implementation, so "lane d continues as lane s would have" is a copy of lane s's
 * column of every per-lane region.  For every i < count with 0 <= src[i] < n_lanes and 0 <= dst[i] < n_lanes, lane dst[i]
 * becomes a byte-for-byte copy of lane src[i] AS IT WAS BEFORE THE CALL; every other pair is skipped (src[i] = -1 is the
 * documented "leave dst[i] alone").  src may repeat a lane; src and dst may overlap in any way, a permutation cycle
 * included: the call is two kernels on `stream`, a gather of every source column into the caller's scratch ([row][i]) and a
 * scatter from it.  dst values must be distinct: a duplicate makes one of its writers win, row by row, and never faults.
 * dst_dev == NULL means dst[i] = i.  src_dev / dst_dev: device int32 [count].  Nothing synchronises.
 *
 * Copied: the 8 float64, 1 int64, 15 int32 and 2 uint8 state rows (the per-lane state of a speed rule among them),
 * action_hist, bw_hist, the QoE terms of the last finished episode, the lane's slot of abr_env_step_mpc's action scratch;
 * the installed quality model's q_run column (mid-episode state); and the same columns of obs_dev, float32
 * [ABR_OBS_DIM][n_lanes], when it is not NULL.  NOT copied: the tick tables and the predictor scratch; the episode ledger's
 * and the quality blob's count, totals, q_last and rings (the slot's history of finished episodes); a speed rule's log.
 * The episode number IS copied, and so are the trace id and start offset: the copy runs the source's episode.  Under an
 * episode sampler a re-arm is keyed by the GLOBAL LANE the copy lives in and by that copied episode number, so source and
 * copy are identical up to their next re-arm and draw different pairs there.  Controller-side state the caller owns (a
 * RobustMPC state, a GRU's hidden rows) is the caller's to move, with the same src / dst.  A size table
 * (abr_env_set_size_table) needs nothing: it is the handle's, with no per-lane state.
 *
 * abr_env_fork_scratch_bytes is pure arithmetic (video_length and count): for each region in the order above, then q_run,
 * then obs -- reserved whether present or not -- rows * count * element bytes, rounded up to a multiple of 256.
 * ABR_E_INVALID, the arguments before the handle: NULL src_dev, count < 0 or > 2^31 - 1, count > 0 with scratch_dev NULL or
 * not 256-byte aligned, a NULL handle, scratch_bytes too small.  ABR_E_UNSUPPORTED: per-lane speeds or a speed schedule in
 * force or pending (abr_env_set_lane_speeds / _speed_schedule: their columns are caller-owned and belong to the slot; a
 * constant speed and a speed rule are fine), and the diagnostic pipelines 4, 6 and 7.
 */
int abr_env_fork_scratch_bytes(abr_env *env, int64_t count, size_t *bytes_out);
int abr_env_fork(abr_env *env, const int32_t *src_dev, const int32_t *dst_dev, int64_t count, void *scratch_dev,
                 size_t scratch_bytes, float *obs_dev, void *stream);

/*
 * Beam selection (ABI 4, additive): per-group top-`beam` of beam * n_rates candidates, for a search that keeps `beam`
 * survivors per group and tries every rate on each (abr_env_fork moves the survivors).  Lanes are grouped as slots = beam *
 * n_rates consecutive lanes per group, slots <= 1024; slot s = r * n_rates + m means "survivor r takes action m".  Group g
 * owns lanes [g * slots, (g + 1) * slots); lanes beyond n_groups * slots are neither read nor written.  Per candidate slot
 * s of a group, in float64, never fused:
 *   R_new = R_in[s] + (double)reward[s]          the running sum of the float32 step rewards, in step order
 *   key   = key_override ? key_override[s] : R_new + wl * lat[s]
 *   valid = valid_in[s] != 0 && !(done[s] & ~ABR_DONE_EPISODE) && key == key     (NaN, timed-out and frozen lanes drop out)
 *   rank  = #{ valid t : key[t] < key[s]  or  (key[t] == key[s] and t < s) }
 * and for every slot s = r * n_rates + m:  src_out[s] = the LANE of the valid candidate with rank r, or -1 when fewer than
 * r + 1 candidates are valid;  R_out[s] = that candidate's R_new (0.0 with none);  valid_out[s] = src_out[s] >= 0.
 * The key adds the latency term the step reward leaves out: lat is abr_env_observe_f64's ABR_F64_AVERAGE_LATENCY row.
 * Smaller keys win (the reward is a cost); -0.0 and +0.0 tie and the smaller slot wins.  One workgroup per group, ranks by
 * counting in LDS: slots^2 compares, deterministic.  All arrays are device memory of at least n_groups * slots elements:
 * R_in, lat, key_override (nullable), R_out float64; reward float32; done, valid_in, valid_out uint8; src_out int32.
 * Outputs must not alias inputs.  ABR_E_INVALID: n_groups < 0, beam < 1, n_rates outside 1..ABR_MAX_RATES, a NULL array
 * (lat_dev may be NULL with a key_override); ABR_E_UNSUPPORTED: beam * n_rates > 1024.  n_groups == 0 launches nothing.
 */
int abr_beam_select(int32_t n_groups, int32_t beam, int32_t n_rates, double wl, const double *R_in_dev,
                    const float *reward_dev, const double *lat_dev, const uint8_t *done_dev, const uint8_t *valid_in_dev,
                    const double *key_override_dev, int32_t *src_out_dev, double *R_out_dev, uint8_t *valid_out_dev,
                    void *stream);

/*
 * Lookahead expert (ABI 4, additive; BUILD-DEFINED: the reference has no teacher): for the state each lane is in NOW, the
 * best next bitrate given the trace's real future, by exhaustive enumeration of the next decisions.  One call, read-only.
 *
 * The tree.  For every lane i whose done byte is 0 (a lane that was never reset carries ABR_DONE_EPISODE, as for
 * abr_env_rule_select), with c = chunk_id[i] and h = min(horizon, video_length - c): every sequence a_0 .. a_{h-1} of rates
 * is walked from the lane's state as it stands, by the step the environment kernels run.  A sequence ends at the step that
 * ends the episode, whatever auto_reset says: the lookahead never re-arms and never looks into the next episode.
 *
 * The key.  All float64, never fused.  rew_j is step j's reward as the environment kernels form it,
 *   rew = wr * (G[n_rb] - G[n_rb_obs]) + ws * (G[n_su] - G[n_su_obs]) + wv * var
 *   var = |br(chunk, a) - br(chunk - 1, prev)| when the download completed and prev >= 0, else 0.0
 *   rew = rew - wq * u[chunk][a]                 only while a quality model is installed (abr_env_set_episode_quality)
 * R_0 = 0.0, R_{j+1} = R_j + (double)(float)rew_j -- the float32 rounding reward_out applies, so R is the sum abr_beam_select
 * forms from reported rewards -- and key = R_h + wl * average_latency, the latency being that of the state after the last
 * step: the value abr_env_observe_f64 would report there.  A sequence is dropped when any of its steps sets
 * ABR_DONE_TIMEOUT or when its key is NaN.
 *
 * Outputs (device).  q_out[m][i] (float64 [n_rates][n_lanes], nullable) = the least key over the valid sequences with
 * a_0 = m, NaN when there is none.  key_out[i] (float64 [n_lanes], nullable) = the least q_out[m][i]; action_out[i] (int32
 * [n_lanes]) its m.  -0.0 and +0.0 tie; ties go to the smaller m, and inside a subtree to the lexicographically smaller
 * sequence.  A lane whose done bits are set, or that has no valid sequence, gets action -1, key NaN and a NaN q column.
 * The call reads the workspace, the traces, the tick tables and the quality table and writes only its three outputs: the
 * workspace, q_run, the ledger, bw_hist and action_hist are untouched.  It is enqueued on `stream`; nothing synchronises.
 *
 * Launch splitting.  A lane's tree has n_rates + n_rates^2 + ... + n_rates^horizon nodes.  The call loops over ranges of
 * lanes, each a multiple of 64 and at least 64, such that no launch walks more than max_nodes_per_launch nodes (0: the
 * library's default, 2^31).
 *
 * Refusals, in this order, the arguments before the handle.  ABR_E_INVALID: NULL cfg; NULL action_out_dev; horizon outside
 * 1..ABR_MAX_HORIZON; reserved_ != 0; max_nodes_per_launch < 0; a NULL handle.  ABR_E_UNSUPPORTED: n_rates^horizon > 65 536
 * leaves (one launch walks one decision's tree; larger trees are the beam search's job); per-lane speeds, a speed schedule
 * or a speed rule in force or pending (a constant play speed is fine); the diagnostic pipelines 4, 6 and 7.
 */
typedef struct abr_lookahead_config {
    int32_t horizon;               /* 1..ABR_MAX_HORIZON */
    int32_t reserved_;             /* 0 */
    int64_t max_nodes_per_launch;  /* 0: the library's default */
} abr_lookahead_config;

int abr_env_lookahead_select(abr_env *env, const abr_lookahead_config *cfg, int32_t *action_out_dev, double *key_out_dev,
                             double *q_out_dev, void *stream);

/*
 * Forecast MPC (ABI 4, additive; BUILD-DEFINED: the reference has no such controller): the lookahead's exhaustive walk on a
 * PREDICTED bandwidth instead of the trace's real future -- the MPC of the literature, with this environment's own step
 * (live-edge gating, start-up, buffer cap, max_ticks) and the QoE the ledger reports, quality term included.  Deployable:
 * it reads nothing a player could not know.
 *
 * The forecast P[i], float64, one per lane.
 *  Without forecast_dev: for every lane whose done byte is 0, steps 1-5 of abr_mpc_robust's contract on the environment's
 *  own chunk_id and previous_bandwidths rows (c = chunk_id, h = the lane's bw_hist rows, W = window).  robust == 1 reads and
 *  updates state_dev exactly as abr_env_step_mpc_robust does (same layout, same bytes).  robust == 0 is the same arithmetic
 *  with no error ever stored, P = hm; it needs no state and touches none.  "No decision" (chunk 0, a harmonic mean that is
 *  not finite or not > 0) is P = 0.0.
 *  With forecast_dev: P[i] = forecast_dev[i]; window, robust's state and state_dev are not looked at beyond the refusals
 *  below, and no state is read or written.
 *  Where P[i] is not finite or not > 0 the lane has no decision.  forecast_out_dev (float64 [n_lanes], nullable) receives
 *  the P the walk used, 0.0 for a lane without a decision and for a lane whose done bits are set.
 *
 * The walk is abr_env_lookahead_select's with one change at the root: the lane's trace cursor points at its forecast --
 * trace = &P[i], tlen = 1, tpos = 0 -- so every interval the walk downloads in has bandwidth P[i]; every other field of the
 * lane is the workspace's.  The tree, the key, the dropped sequences (a time-out, a NaN key), the tie rules, the horizon's
 * shrink at the episode's end, the shapes of action_out / key_out / q_out and the launch splitting are word for word the
 * lookahead's.  A lane whose done bits are set, that has no decision or that has no valid sequence gets action -1, key NaN
 * and a NaN q column.
 *
 * abr_env_plan_select writes its outputs and, with robust == 1 and no forecast_dev, the state: the workspace, q_run, the
 * ledger, bw_hist and action_hist are untouched, and selecting twice on one state gives the same answer and the same state.
 * P needs n_lanes float64 of device memory while the call runs: with the built-in forecast that is forecast_out_dev; only
 * a caller that passes neither forecast_dev nor forecast_out_dev has P written to the workspace's MPC scratch (the region
 * abr_env_step_mpc's predictor overwrites at every decision; it carries nothing between calls).
 *
 * abr_env_step_plan follows abr_env_step_mpc: per decision the forecast, the plan, then the download, enqueued back to back
 * on `stream`; outputs (all nullable) as abr_env_step_mpc's.  Finished lanes take no decision and keep their state; action
 * -1 downloads bitrate 0 and actions_out reports 0 for it.  A forecast_dev given here is used unchanged at every decision
 * (a fixed belief).  The built-in forecast goes through the workspace's MPC scratch.  Kernel choice as abr_env_step_mpc.
 *
 * Refusals, in this order, the arguments before the handle.  ABR_E_INVALID: NULL cfg; NULL action_out_dev (select); horizon
 * outside 1..ABR_MAX_HORIZON; reserved_ != 0; max_nodes_per_launch < 0; robust not 0 or 1; without forecast_dev, window
 * outside 1..ABR_ROBUST_MAX_WINDOW; n_steps < 1 (step); a NULL handle; then, with robust == 1 and no forecast_dev, a NULL
 * state_dev, one that is not 8-byte aligned, or state_bytes below abr_mpc_robust_state_bytes(window, n_lanes).
 * ABR_E_UNSUPPORTED: the lookahead's three (the leaf cap; speed features in force or pending; impl 4 / 6 / 7), then, for
 * abr_env_step_plan, impl 1 as abr_env_step_mpc.
 */
typedef struct abr_plan_config {
    int32_t horizon;               /* 1..ABR_MAX_HORIZON */
    int32_t window;                /* 1..ABR_ROBUST_MAX_WINDOW; ignored when forecast_dev is given */
    int32_t robust;                /* 0: P = harmonic mean; 1: RobustMPC's discount P = hm / (1 + max error) */
    int32_t reserved_;             /* 0 */
    int64_t max_nodes_per_launch;  /* as abr_lookahead_config */
    const double *forecast_dev;    /* nullable: float64 [n_lanes], the caller's forecast; skips the built-in one */
    void *state_dev;               /* robust == 1 and no forecast_dev: abr_mpc_robust's state, same layout,
                                      abr_mpc_robust_state_bytes(window, n_lanes), all-zero = empty; else ignored */
    size_t state_bytes;
} abr_plan_config;

int abr_env_plan_select(abr_env *env, const abr_plan_config *cfg, int32_t *action_out_dev, double *key_out_dev,
                        double *q_out_dev, double *forecast_out_dev, void *stream);
int abr_env_step_plan(abr_env *env, const abr_plan_config *cfg, int32_t n_steps, float *obs_out_dev,
                      float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream);

/* ---------------------------------------------------------------------- */
/* MPC lookahead                                                            */
/* ---------------------------------------------------------------------- */

/* Replaces what MPCBitrateController reads through the player protocol
 * (mpc.py:56-57: get_mpd, get_qoe_metric) and its horizon (mpc.py:59). */
typedef struct abr_mpc_config {
    int32_t n_rates;            /* len(mpd.chunks[0].bitrates)  mpc.py:173 */
    int32_t horizon;            /* 2..ABR_MAX_HORIZON (the reference crashes at 1, mpc.py:186) */
    int32_t video_length;       /* len(mpd.chunks) */
    int32_t clip_horizon;       /* !=0: H_eff = min(H, V - chunk) (D12; the reference raises IndexError) */
    double  chunk_length;       /* mpd.chunk_length  mpc.py:108,117,151 */
    double  max_buffer;         /* mpd.max_buffer    mpc.py:108 */
    double  variance_weight;    /* qoe.*             mpc.py:158-160 */
    double  rebuffer_weight;
    double  startup_weight;     /* multiplies the hard-zero startup_delay (mpc.py:141) */
} abr_mpc_config;

/*
 * MPCBitrateController.next_bitrate() (mpc.py:181-186) for n_lanes independent
 * players: harmonic-mean prediction fed back H times (mpc.py:81-93), exhaustive
 * evaluation of objective() (mpc.py:120-162) over all n_rates^horizon combos in
 * scipy.optimize.brute's C order with first-minimum tie-break (mpc.py:178), and
 * int(result[0]).
 *  chunk_dev/prev_bitrate_dev/buffer_dev: chunk_info.chunk_number /
 *      .previous_bitrate / .buffer_level (mpc.py:124,132,136)
 *  hist_n_dev/hist_sum_inv_dev: IN-OUT summary of chunk_info.previous_bandwidths
 *      (length and sum of reciprocals in list order); grown by H predictions
 *      exactly as the reference mutates the caller's list (mpc.py:92, D9)
 *  br_table_dev/sz_table_dev: [video_length][n_rates] mpd.chunks[i].bitrates/.sizes
 *  action_out_dev int32 [n_lanes]; best_flat_out_dev (nullable) int32 [n_lanes]
 *  flat arg-min index; best_J_out_dev (nullable) float64 [n_lanes];
 *  lane_mask_dev (nullable): lanes with a zero byte are skipped entirely
 *  (no history mutation, outputs untouched).
 *  previous_bitrate indexes the ladder as Python does (mpc.py:132,148): -n_rates..-1 wrap to
 *  the top (the env's "no previous chunk" value -1 means the highest rate).
 *  Lanes the reference would raise on report action -1 (flat -1, J NaN) and keep their
 *  history: an empty or zero history (ZeroDivisionError, mpc.py:88,90, D13), a predicted
 *  throughput of 0.0 (the sum of reciprocals overflowed: ZeroDivisionError at mpc.py:88 on
 *  the next pass or at mpc.py:151), a previous_bitrate outside [-n_rates, n_rates)
 *  (IndexError) and, without clip_horizon, chunk + horizon > video_length (IndexError,
 *  mpc.py:126, D12).
 *  Non-finite objectives follow np.argmin over the grid, as scipy's brute does: the first
 *  combination whose J is NaN wins (flat >= 0, J NaN); with no NaN the first minimum wins,
 *  so a grid where every J is +inf gives combination 0 (J = +inf).
 */
int abr_mpc_select(const abr_mpc_config *cfg, const int32_t *chunk_dev,
                   const int32_t *prev_bitrate_dev, const double *buffer_dev, double *hist_n_dev,
                   double *hist_sum_inv_dev, const double *br_table_dev, const double *sz_table_dev,
                   const uint8_t *lane_mask_dev, int32_t *action_out_dev,
                   int32_t *best_flat_out_dev, double *best_J_out_dev, int64_t n_lanes,
                   void *stream);

/*
 * The reference's alternative predictor and utility.  PARITY UNPINNED:
 * the predictor needs statsmodels (mpc.py:4,74), which is not installable here, and no test
 * of the reference touches either; what is implemented is the documented rule below, checked
 * for self-consistency only.
 *  ABR_PREDICT_EXPSMOOTHING  predict_throughput(..., method="expsmoothing") (mpc.py:72-79):
 *      SimpleExpSmoothing(history).fit(0.5) and its `horizon` out-of-sample forecasts, i.e.
 *      the last smoothed level repeated: level(t) = 0.5*y(t) + 0.5*level(t-1), with the
 *      initial level chosen to minimise the sum of squared one-step-ahead errors (closed
 *      form; statsmodels' default `estimated` initialisation finds it numerically).  Needs
 *      the throughput history itself: entry t of lane i at hist_dev[t * hist_stride + i],
 *      hist_len_dev[i] entries (for an environment: abr_env_state_view.bw_hist with stride
 *      n_lanes and chunk_id as the length).  Unlike the harmonic branch it does not grow the
 *      history (no D9) and ignores hist_n / hist_sum_inv.
 *  ABR_UTILITY_LOG  log_bitrate_utility (mpc.py:99-102) with the arity its call sites need:
 *      u = log(bitrate / highest bitrate of that chunk) in place of the identity utility in
 *      video_quality and quality_variance (mpc.py:146-149).
 */
#define ABR_PREDICT_HARMONIC 0
#define ABR_PREDICT_EXPSMOOTHING 1
#define ABR_UTILITY_IDENTITY 0
#define ABR_UTILITY_LOG 1
typedef struct abr_mpc_options {
    int32_t predictor;            /* ABR_PREDICT_* */
    int32_t utility;              /* ABR_UTILITY_* */
    const double *hist_dev;       /* ABR_PREDICT_EXPSMOOTHING only */
    int64_t hist_stride;
    const int32_t *hist_len_dev;
    void *scratch_dev;            /* optional, any predictor: abr_mpc_scratch_bytes() of caller-owned, 8-byte
                                     aligned device memory.  With it the predictor (ten dependent IEEE
                                     divisions per lane at horizon 5) runs as a kernel of its own, one thread
                                     per lane, instead of on 1 of the lane's n_rates^2 search threads: same
                                     results, ~10 % less time.  NULL: everything in one kernel. */
    size_t scratch_bytes;
    int32_t mask_is_done;         /* != 0: lane_mask_dev holds ABR_DONE_* bits (an environment's `done` array, as
                                     is): a lane is skipped iff its byte is NON-zero, and reports action -1.
                                     0: lane_mask_dev is a plain mask, lanes with a zero byte are skipped */
    int32_t reserved_;
} abr_mpc_options;

/* Bytes of scratch abr_mpc_options.scratch_dev needs for n_lanes at cfg->horizon. */
int abr_mpc_scratch_bytes(const abr_mpc_config *cfg, int64_t n_lanes, size_t *bytes_out);

/* abr_mpc_select with options; opt == NULL is abr_mpc_select. */
int abr_mpc_select_opt(const abr_mpc_config *cfg, const abr_mpc_options *opt,
                       const int32_t *chunk_dev, const int32_t *prev_bitrate_dev,
                       const double *buffer_dev, double *hist_n_dev, double *hist_sum_inv_dev,
                       const double *br_table_dev, const double *sz_table_dev,
                       const uint8_t *lane_mask_dev, int32_t *action_out_dev,
                       int32_t *best_flat_out_dev, double *best_J_out_dev, int64_t n_lanes,
                       void *stream);

/*
 * MPC-driven rollout, fused on the device: for n_steps decisions, each lane's action is
 * MPCBitrateController.next_bitrate() (mpc.py:181-186) evaluated on the lane's OWN
 * environment state -- chunk_number = chunk_id, previous_bitrate = previous_bitrates[-1],
 * buffer_level, and previous_bandwidths as the environment's (len, sum of reciprocals)
 * summary, which the predictor grows by `horizon` entries per call exactly as the reference
 * mutates the shared list (mpc.py:92, D9) -- followed by the download of that chunk
 * (Simulator.py:155-170; abr_env_step).  This is the wiring the reference leaves open
 * (get_next_bitrate(...) at Simulator.py:155 vs next_bitrate() at mpc.py:181, D5/D6); no host
 * round trip or host-side tensor work happens between decisions.
 *  br_table_dev/sz_table_dev: [video_length][n_rates] as for abr_mpc_select; cfg->n_rates and
 *  cfg->video_length must equal the environment's.
 *  Lanes whose done bits are set take no decision (action -1) and stay frozen.  A lane the
 *  reference would raise on (empty history at chunk 0: ZeroDivisionError, D13; horizon past
 *  the video end without clip_horizon, D12) downloads bitrate 0 and keeps its history.
 *  Outputs (all nullable): obs [n_steps][ABR_OBS_DIM][n_lanes], reward/done/actions
 *  [n_steps][n_lanes], as abr_env_step_random.  Event-driven kernels only: ABR_E_UNSUPPORTED on impl 1.
 */
int abr_env_step_mpc(abr_env *env, const abr_mpc_config *cfg, const double *br_table_dev,
                     const double *sz_table_dev, int32_t n_steps, float *obs_out_dev,
                     float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                     void *stream);

/*
 * RobustMPC (Yin et al., SIGCOMM 2015): the same search as abr_mpc_select (objective, D10, D11, D12 clip, Python's negative
 * previous_bitrate, first-minimum tie-break, the non-finite rules above) fed by an error-discounted throughput estimate
 * instead of the reference's harmonic predictor.  For one active lane at a decision: c = chunk_number (also the history
 * length), h[0..c) = previous_bandwidths oldest first, W = window.  The lane's state holds the last estimate p*, the chunk
 * c* it was made at (or none) and up to W past relative errors, oldest first.  All float64, in this order:
 *  1. c* == c - 1: push e = |p* - h[c-1]| / h[c-1], keeping the last W errors; c* == c: errors unchanged (selecting
 *     twice on the same state gives the same answer); otherwise (none, a gap, a new episode, a rewind) clear them.
 *  2. n = min(W, c); n == 0: no decision, state := empty.
 *  3. S = sum over j = c-n .. c-1 (in that order) of 1.0 / h[j]; hm = n / S (ABR_RULE_RATE's arithmetic).
 *  4. E = the stored errors' maximum, scanned oldest first: E = e[0], then E = e[k] if e[k] > E; 0.0 with no errors.
 *     P = hm / (1.0 + E).
 *  5. hm not finite or not > 0: no decision, state := empty.  P not > 0: no decision, but p* = hm, c* = c are recorded.
 *  6. Otherwise p* = hm, c* = c, and the search runs with C_hat[i] = P for every i < H_eff.
 * The state is updated whenever step 3 produced an estimate, even if the search then reports no decision (D12, a bad
 * previous_bitrate).  The history summary hist_n / hist_sum_inv is NOT mutated (no D9).  Masked or finished lanes are
 * skipped: state, flat and J untouched, and the action too except under mask_is_done, which reports -1.  "No decision" reports action -1, flat -1, J NaN as abr_mpc_select.
 *
 * State layout (caller-owned device memory, 8-byte aligned, abr_mpc_robust_state_bytes(window, n_lanes); ALL-ZERO BYTES
 * ARE THE EMPTY STATE): int32 [2][n_lanes] -- row 0 c* + 1 (0 = none), row 1 the error count (0..W; any other value reads
 * as 0) -- followed by float64 [1 + window][n_lanes] -- row 0 p*, rows 1 .. 1 + count the errors oldest first (rows at or
 * past the count hold no meaning).  Lane i's field f is at row f, column i, as everywhere in this ABI.  The layout depends
 * on the window: a state is only meaningful for the window it was written with.
 */
#define ABR_ROBUST_MAX_WINDOW 16
typedef struct abr_mpc_robust {
    int32_t window;               /* W, 1..ABR_ROBUST_MAX_WINDOW (RobustMPC's default: 5) */
    int32_t utility;              /* ABR_UTILITY_* as for abr_mpc_select_opt */
    void *state_dev;              /* IN-OUT per-lane state, layout above */
    size_t state_bytes;           /* >= abr_mpc_robust_state_bytes(window, n_lanes) */
    const double *hist_dev;       /* abr_mpc_select_robust: previous_bandwidths, entry j of lane i at
                                     hist_dev[j * hist_stride + i], at least chunk_number rows per lane.  Ignored by
                                     abr_env_step_mpc_robust, which reads the environment's own history */
    int64_t hist_stride;
    void *scratch_dev;            /* abr_mpc_scratch_bytes(cfg, n_lanes) of 8-byte aligned device memory for the
                                     estimates handed to the search.  Required by abr_mpc_select_robust; optional for
                                     abr_env_step_mpc_robust (NULL: the environment's workspace) */
    size_t scratch_bytes;
    int32_t mask_is_done;         /* abr_mpc_select_robust: as abr_mpc_options.mask_is_done */
    int32_t reserved_[5];         /* set to 0 */
} abr_mpc_robust;

/* Bytes of the RobustMPC state of n_lanes lanes at `window`. */
int abr_mpc_robust_state_bytes(int32_t window, int64_t n_lanes, size_t *bytes_out);

/* RobustMPC's next_bitrate for n_lanes independent players; arguments and outputs as abr_mpc_select_opt, without the
 * history summary.  Validation (ABR_E_INVALID, nothing launched): the config as abr_mpc_select, window in 1..16, the
 * utility, a non-NULL 8-byte aligned state of at least the size query's bytes, hist_dev != NULL and hist_stride >= 1,
 * a scratch of at least abr_mpc_scratch_bytes, n_lanes >= 1, then the device pointers. */
int abr_mpc_select_robust(const abr_mpc_config *cfg, const abr_mpc_robust *robust, const int32_t *chunk_dev,
                          const int32_t *prev_bitrate_dev, const double *buffer_dev, const double *br_table_dev,
                          const double *sz_table_dev, const uint8_t *lane_mask_dev, int32_t *action_out_dev,
                          int32_t *best_flat_out_dev, double *best_J_out_dev, int64_t n_lanes, void *stream);

/* abr_env_step_mpc with RobustMPC's estimate: per decision the robust predictor on each lane's own state (chunk_id,
 * previous_bitrates[-1], buffer_level, and the environment's previous_bandwidths rows), the search, then the download.
 * Kernel choice as abr_env_step_mpc (impl 1, tick, answers ABR_E_UNSUPPORTED); finished lanes take no decision and keep
 * their state; "no decision" downloads bitrate 0.  robust->hist_dev, hist_stride and mask_is_done are ignored.
 * Validation (ABR_E_INVALID, nothing launched): the config and robust options as above and n_steps >= 1 before the handle
 * is looked at; then the tables against the environment, the state size and the scratch size (if given) for its lanes. */
int abr_env_step_mpc_robust(abr_env *env, const abr_mpc_config *cfg, const abr_mpc_robust *robust,
                            const double *br_table_dev, const double *sz_table_dev, int32_t n_steps, float *obs_out_dev,
                            float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream);

/*
 * The standard ABR baselines as get_next_bitrate (Simulator.py:155), evaluated on the device at each lane's call site on
 * exact float64 state: c = chunk_id, B = buffer_level, h[0..c) = previous_bandwidths oldest first, br[m] = chunk c's
 * bitrate m (the abr_env_set_bitrate_table row, else config.ladder), M = n_rates.
 * hi(X) = the last m in 1..M-1 with br[m] <= X, else 0 (on an ascending ladder: the highest rate not above X).
 *  ABR_RULE_BUFFER  BBA-0 rate map (Huang et al. 2014), no hysteresis: B <= reservoir -> 0; B >= reservoir + cushion -> M-1;
 *                   else hi(br[0] + ((B - reservoir) / cushion) * (br[M-1] - br[0])).
 *  ABR_RULE_RATE    n = min(window, c); n == 0 -> 0; else S = sum over j = c-n .. c-1 (in that order) of 1.0 / h[j],
 *                   hi(safety * (n / S)).
 *  ABR_RULE_BOLA    BOLA-BASIC (Spiteri et al. 2016): the FIRST m maximising (bola_v * (u[c][m] + bola_gp) - B) / br[m],
 *                   u = utility_dev [video_length][n_rates] float64 (caller-computed, e.g. ln(br[c][m] / br[c][0])).
 * Every operation is float64 in the order written (the library is built with -ffp-contract=off).  Validation (before the
 * handle is looked at; ABR_E_INVALID, nothing launched): kind, finite parameters, reservoir >= 0, cushion > 0, window >= 1,
 * safety > 0, bola_v > 0, utility_dev != NULL for BOLA, n_steps >= 1.
 */
enum { ABR_RULE_BUFFER = 1, ABR_RULE_RATE = 2, ABR_RULE_BOLA = 3 };
typedef struct abr_rule_config {
    int32_t kind, window;
    double reservoir, cushion, safety, bola_v, bola_gp;
    const double *utility_dev;      /* BOLA: [video_length][n_rates] float64 */
} abr_rule_config;

/* n_steps fused decisions per lane taken by the rule, with no host work between decisions.  Outputs (all nullable) as
 * abr_env_step_random; lanes whose done bits are set take no decision (action -1) and stay frozen.  Kernels: `auto` (3) and
 * 0 run the one-thread-per-lane kernel at every size, 1 the tick kernel; 2 and 5 answer ABR_E_UNSUPPORTED (their download
 * wave runs ahead of the player and does not know the call-site buffer level). */
int abr_env_step_rule(abr_env *env, const abr_rule_config *rule, int32_t n_steps, float *obs_out_dev,
                      float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev, void *stream);
/* The rule's answer for each lane on the environment's current state, no step: action_out_dev int32 [n_lanes], -1 for a
 * lane whose done bits are set. */
int abr_env_rule_select(abr_env *env, const abr_rule_config *rule, int32_t *action_out_dev, void *stream);

/*
 * FastMPC (Yin et al., SIGCOMM 2015; ABI 4, additive; BUILD-DEFINED: the reference has no FastMPC).  The MPC search is run
 * once, on the device, over a quantised state space; a decision is then one table lookup, evaluated inside the environment
 * kernels like the bitrate rules above.
 *
 * Inputs: an abr_mpc_config and br / sz tables [V][M] exactly as for abr_mpc_select, the utility, a window W in 1..16, a
 * buffer grid of Nb points bp[] with Nb - 1 edges be[], and a throughput grid of Nq points tp[] with Nq - 1 edges te[]
 * (host arrays of float64, Nb and Nq in 1..ABR_FASTMPC_MAX_POINTS, edges NULL allowed when there are none).  Points and
 * edges are finite and strictly ascending, buffer points >= 0, throughput points > 0, and every point lies in its own cell:
 * e[k-1] <= p[k] < e[k] (so that a state exactly on a grid point reads that point's entry).
 * Layout: n_rows == V: one row per chunk (row = c); otherwise n_rows == H < V: the UNIFORM layout, valid only when every
 * row of br / sz is the same (the caller's promise: the library does not read the tables on the host), row of chunk c =
 * min(V - c, H) - 1, and row r is built at chunk V - 1 - r.
 *
 * Table: uint8 entries [n_rows][M][Nb][Nq] (q fastest).  Entry (row, p, bi, qi) = int(result[0]) of the first-minimum
 * arg-min of objective() at chunk c_row, previous_bitrate p, buffer_level bp[bi] and C_hat[i] = tp[qi] for every
 * i < H_eff -- D10, D11, the D12 clip, the non-finite rules and the utility as abr_mpc_select -- with "no decision" (without
 * clip_horizon: c_row + H > V) stored as 0, which is what abr_env_step_mpc downloads for it.
 *
 * Lookup, for a lane at a call site with chunk c, previous bitrate prev (-M..-1 wrap as in Python), buffer B and history
 * h[0..c):  n = min(W, c); n == 0 -> action 0 (as RATE).  P = ABR_RULE_RATE's harmonic mean of h[c-n .. c-1] (same
 * float64 operations, same order).  bi = number of buffer edges <= B, qi = number of throughput edges <= P (NaN: 0, +inf:
 * the last cell).  action = table[row(c)][prev][bi][qi].  Comparisons only after P: a numpy twin reproduces every answer.
 *
 * Blob (caller-owned device memory, 8-byte aligned, abr_fastmpc_table_bytes): the entries, padded to a multiple of 8 bytes,
 * then be[0 .. Nb-1), then te[0 .. Nq-1), float64.  abr_fastmpc_build writes all of it on the stream (the grids travel as
 * kernel arguments: the host arrays may go as soon as the call returns).  A blob is only meaningful for the config, tables,
 * utility, layout and grid it was built with, and the window of the lookups is the caller's to keep with it (as the
 * RobustMPC state and its window).
 */
#define ABR_FASTMPC_MAX_POINTS 256
typedef struct abr_fastmpc {
    int32_t window;               /* W, 1..ABR_ROBUST_MAX_WINDOW */
    int32_t utility;              /* ABR_UTILITY_* */
    int32_t n_rows;               /* video_length (per chunk) or horizon (uniform, horizon < video_length) */
    int32_t n_buffer;             /* Nb, 1..ABR_FASTMPC_MAX_POINTS */
    int32_t n_tput;               /* Nq, 1..ABR_FASTMPC_MAX_POINTS */
    const double *buffer_points;  /* host [Nb], [s] */
    const double *buffer_edges;   /* host [Nb - 1] */
    const double *tput_points;    /* host [Nq], the ladder's unit */
    const double *tput_edges;     /* host [Nq - 1] */
    int32_t reserved_[2];         /* set to 0 */
} abr_fastmpc;

/* Bytes of the blob, and of the build's device scratch (8-byte aligned; the build runs the grid in slices, so this is
 * bounded whatever the table's size).  Both check the config and every field of fm as the build does. */
int abr_fastmpc_table_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm, size_t *bytes_out);
int abr_fastmpc_build_scratch_bytes(const abr_mpc_config *cfg, const abr_fastmpc *fm, size_t *bytes_out);

/* Build the table into the blob: the existing MPC search on every grid point, slice after slice, all enqueued on `stream`.
 * br_table_dev / sz_table_dev: [video_length][n_rates] as abr_mpc_select.  Validation (ABR_E_INVALID, nothing launched):
 * the config, fm, the blob and the scratch (non-NULL, 8-byte aligned, at least the size queries' bytes), the tables. */
int abr_fastmpc_build(const abr_mpc_config *cfg, const abr_fastmpc *fm, const double *br_table_dev,
                      const double *sz_table_dev, void *table_dev, size_t table_bytes, void *scratch_dev,
                      size_t scratch_bytes, void *stream);

/* The lookup for n_lanes independent players: chunk_dev / prev_bitrate_dev / buffer_dev as abr_mpc_select, the history
 * entry j of lane i at hist_dev[j * hist_stride + i] (at least min(W, chunk) rows before the chunk).  action_out_dev int32
 * [n_lanes]; a lane whose chunk is outside [0, V) or whose previous bitrate is outside [-M, M) reports -1.
 * lane_mask_dev (nullable) as abr_mpc_options with mask_is_done: skipped lanes keep their action, except under
 * mask_is_done, which reports -1.  table_bytes is checked against the size query. */
int abr_fastmpc_select(const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev, size_t table_bytes,
                       const int32_t *chunk_dev, const int32_t *prev_bitrate_dev, const double *buffer_dev,
                       const double *hist_dev, int64_t hist_stride, const uint8_t *lane_mask_dev, int32_t mask_is_done,
                       int32_t *action_out_dev, int64_t n_lanes, void *stream);

/* n_steps fused decisions per lane taken by the lookup on each lane's own call-site state (chunk_id, previous_bitrates[-1],
 * buffer_level, the environment's previous_bandwidths rows), as abr_env_step_rule: outputs (nullable) as
 * abr_env_step_random, done lanes take no decision (action -1); kernels as abr_env_step_rule (ABR_E_UNSUPPORTED on 2 and 5).
 * Validation (ABR_E_INVALID, nothing launched): the config, fm (its grid only by count: the lookup reads the edges from the
 * blob) and n_steps before the handle; then M and V against the environment, and the uniform layout is refused while a
 * per-chunk bitrate table (abr_env_set_bitrate_table) is in force or pending. */
int abr_env_step_fastmpc(abr_env *env, const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev,
                         int32_t n_steps, float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                         int32_t *actions_out_dev, void *stream);
/* The lookup's answer for each lane on the environment's current state, no step: action_out_dev int32 [n_lanes], -1 for a
 * lane whose done bits are set.  Checks as abr_env_step_fastmpc. */
int abr_env_fastmpc_select(abr_env *env, const abr_mpc_config *cfg, const abr_fastmpc *fm, const void *table_dev,
                           int32_t *action_out_dev, void *stream);

/*
 * Learned policy (ABI 4, additive; BUILD-DEFINED: the reference has no learned controller).  A small MLP evaluated on the
 * device on each lane's exact call-site state, one decision per lane, with no host round trip; the caller trains it (in
 * PyTorch, say) and refreshes the weights in place between rollouts.
 *
 * Inputs of a lane that takes a decision: c = chunk_id, B = buffer_level, a = previous_bitrates[-1] (-1 if none),
 * h[0..c) = the lane's previous_bandwidths (abr_env_state_view.bw_hist rows of the current episode), G and P =
 * global_time and play_time exactly as abr_env_observe_f64 reports them, br(r, m) = chunk r's bitrate m (the
 * abr_env_set_bitrate_table row, else config.ladder), V = video_length, M = n_rates, W = window (0..16).
 *
 * Features, F = 4 + W + M, raw values float64:
 *   0         B
 *   1         (a >= 0 and c >= 1) ? br(c - 1, a) : 0.0
 *   2         (double)(V - c)
 *   3         G - P
 *   4 + k     h[c - W + k], or 0.0 where c - W + k < 0 (k < W, oldest first)
 *   4 + W + m br(c, m) (m < M)
 * x_i = (float)((raw_i - shift_i) * scale_i): both operations in float64, then one round-to-nearest conversion.  norm_dev:
 * float64 [2][F], row 0 shift, row 1 scale (caller-owned device memory); NULL = shift 0, scale 1.
 *
 * Network: n_hidden (0..2) hidden layers of widths width[0..n_hidden) (1..64 each), then an output layer of width M.
 * Weights: one float32 blob, per layer Wt [out][in] row-major (torch.nn.Linear.weight's layout) then b [out], layers in
 * order, no padding (abr_policy_weights_bytes).  Output j of a layer: acc = b[j], then acc = fmaf(Wt[j][k], x[k], acc) for
 * k = 0, 1, .., in - 1 in that order (one rounding per term: an f32 MFMA, a VALU and a host std::fmaf chain give the same
 * bits).  A hidden output becomes acc > 0.0f ? acc : 0.0f (NaN and -0 become +0).  The output layer gives score[0..M).
 * f32 subnormals are kept (the library is not built with flush-to-zero).
 *
 * Decision: g = the first argmax (g = 0, then g = m if score[m] > score[g]; NaN never wins, a NaN score[0] answers 0).
 * Exploration, an exact integer contract: one philox4x32-10 block with the random policy's key and counter (key = seed,
 * ctr = (global lane id lo, hi, c, episode number), as abr_env_step_random).  Output word 1 < explore_threshold (a uint64 in
 * [0, 2^32]): the action is the random policy's action from the same block (what abr_env_step_random would draw at this
 * call site); otherwise g.  0 never explores, 2^32 always does.
 *
 * A lane whose done bits are set takes no decision: action -1, its feature and score columns 0.0f.
 */
#define ABR_POLICY_MAX_WINDOW 16
#define ABR_POLICY_MAX_HIDDEN 2
#define ABR_POLICY_MAX_WIDTH 64
typedef struct abr_policy {
    int32_t window;                       /* W, 0..ABR_POLICY_MAX_WINDOW */
    int32_t n_hidden;                     /* 0..ABR_POLICY_MAX_HIDDEN */
    int32_t width[ABR_POLICY_MAX_HIDDEN]; /* hidden widths, 1..ABR_POLICY_MAX_WIDTH; entries past n_hidden set to 0 */
    const float *weights_dev;             /* the blob (device, 4-byte aligned) */
    size_t weights_bytes;                 /* == abr_policy_weights_bytes(this, n_rates) */
    const double *norm_dev;               /* float64 [2][F] (device, 8-byte aligned) or NULL */
    uint64_t seed;                        /* philox key of the exploration draw */
    uint64_t explore_threshold;           /* 0 .. 2^32 */
    int32_t reserved_[4];                 /* set to 0 */
} abr_policy;

/* F = 4 + window + n_rates (window 0..16, n_rates 1..ABR_MAX_RATES). */
int abr_policy_feature_dim(int32_t window, int32_t n_rates, int32_t *dim_out);
/* Bytes of the weight blob for pol's shape (window, n_hidden, width; the pointers are not looked at) and n_rates. */
int abr_policy_weights_bytes(const abr_policy *pol, int32_t n_rates, size_t *bytes_out);

/* The policy's decision for each lane on the environment's current state, no step: action_out_dev int32 [n_lanes];
 * features_out_dev float32 [F][n_lanes] and scores_out_dev float32 [n_rates][n_lanes], both nullable.  Validation
 * (ABR_E_INVALID, nothing launched): the struct (shape, window, reserved_ zero, weights non-NULL and aligned, norm aligned,
 * threshold <= 2^32) before the handle; then weights_bytes against the environment's n_rates. */
int abr_env_policy_select(abr_env *env, const abr_policy *pol, int32_t *action_out_dev, float *features_out_dev,
                          float *scores_out_dev, void *stream);

/* n_steps fused decisions: per decision the policy kernel on each lane's own state, then the download of that chunk
 * (abr_env_step).  Outputs (all nullable): obs [n_steps][ABR_OBS_DIM][n_lanes], reward / done / actions [n_steps][n_lanes]
 * as abr_env_step_random, features [n_steps][F][n_lanes], scores [n_steps][n_rates][n_lanes] as abr_env_policy_select.
 * Kernels as abr_env_step_mpc (ABR_E_UNSUPPORTED on impl 1, tick).  Validation as abr_env_policy_select, with
 * n_steps >= 1 before the handle. */
int abr_env_step_policy(abr_env *env, const abr_policy *pol, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                        uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                        void *stream);

/*
 * Sampled decisions of the learned policy (ABI 4, additive; BUILD-DEFINED).  A stochastic policy (an actor trained with
 * A2C or PPO) takes its action from softmax(score / T) and its trainer needs the probability of that action; inside a
 * fused rollout only the device can draw it.  Exact, so that a host build of the same header and a numpy twin reproduce
 * every bit (the library is built with -ffp-contract=off -fno-fast-math; every operation below is float32,
 * round-to-nearest-even, one rounding each).
 *
 * Inputs: the scores s[0..M) and the first argmax g of abr_policy (unchanged), iT = inv_temperature (finite, > 0).
 *   Fallback: if s[g] is not finite (+inf; NaN at index 0 with nothing greater; all scores -inf) the decision is g and
 *     the distribution is one-hot at g.
 *   Scaled logits, for m = 0 .. M-1 in order: d_m = s_m - s[g], x_m = d_m * iT, e_m = exp_c(x_m).  x_m <= 0 (a NaN s_m
 *     gives a NaN x_m, and e_m = 0), so e[g] = exp_c(0) = 1 and 1 <= S <= M.
 *   exp_c(x): +0 when !(x >= -80) (-inf and NaN included).  Otherwise
 *     k = rintf(x * 0x1.715476p+0f)                      (one rounded product, then round half to even; -116 <= k <= 0)
 *     r = fmaf(-k, 0x1.63p-1f, x);  r = fmaf(-k, -0x1.bd0106p-13f, r)              (Cephes' split of ln 2)
 *     p = 0x1.6b69e0p-10f;  then p = fmaf(p, r, c) for c = 0x1.1234fcp-7f, 0x1.555694p-5f, 0x1.55549cp-3f, 0.5f, 1.0f,
 *       1.0f in that order                                (a minimax fit of exp on [-ln2/2, ln2/2] with c0 = c1 = 1, c2 = 1/2)
 *     exp_c = ldexpf(p, k), exact (k >= -116 keeps p * 2^k normal).
 *     exp_c(+-0) = 1 exactly; on [-80, 0] its relative error against exp is below 2^-23 (7.7e-8 on a dense grid).
 *   Sum: S = e_0 + e_1 + ... + e_(M-1), added in that order from 0.0f; cum_m is the same running sum after term m.
 *   Draw: w2 = output word 2 of the policy's philox block (key seed, counter (global lane id lo, hi, c, episode number),
 *     the block whose words 0 and 1 the exploration reads); q = (float)(w2 >> 8) * 0x1p-24f (exact, q < 1),
 *     t = q * S (rounded).  The sample is the first m with cum_m > t.  The comparison is strict, so an action with
 *     e_m = 0 is never drawn; t < S = cum_(M-1) always, so one m qualifies (were none to, the answer would be g).
 *   Exploration is unchanged: word 1 < explore_threshold takes the random policy's action from word 0; otherwise the
 *     action is the sample (ABR_POLICY_SOFTMAX) or g (ABR_POLICY_ARGMAX, exactly abr_env_policy_select's action).
 *   probs[m] = e_m / S, the correctly rounded float32 division: the policy's distribution pi before exploration
 *     (ABR_POLICY_ARGMAX: one-hot at g).  With explore_threshold thr, eps = thr / 2^32, the behaviour distribution is
 *     (1 - eps) * pi[m] + eps * rho[m], rho[m] = (ceil((m + 1) * 2^32 / M) - ceil(m * 2^32 / M)) / 2^32, the exact share
 *     of words w0 with ((uint64)w0 * M) >> 32 == m.
 * A lane whose done bits are set takes no decision: action -1, its feature, score and probs columns 0.0f.
 */
#define ABR_POLICY_ARGMAX 0
#define ABR_POLICY_SOFTMAX 1
typedef struct abr_policy_sampling {
    int32_t mode;                         /* ABR_POLICY_ARGMAX or ABR_POLICY_SOFTMAX */
    float inv_temperature;                /* 1 / T: finite, > 0 (unused by ABR_POLICY_ARGMAX but checked) */
    int32_t reserved_[6];                 /* set to 0 */
} abr_policy_sampling;

/* abr_env_policy_select with the decision of `smp` (above) and probs_out_dev float32 [n_rates][n_lanes] (nullable).
 * Validation (ABR_E_INVALID, nothing launched): abr_env_policy_select's checks of pol, then smp (non-NULL, mode,
 * inv_temperature, reserved_ zero), all before the handle; then as abr_env_policy_select. */
int abr_env_policy_select_sampled(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                                  int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                  float *probs_out_dev, void *stream);

/* abr_env_step_policy with the decisions of `smp`; probs_out_dev float32 [n_steps][n_rates][n_lanes] (nullable).
 * Validation as abr_env_policy_select_sampled, with n_steps >= 1 before the handle; ABR_E_UNSUPPORTED on tick. */
int abr_env_step_policy_sampled(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp, int32_t n_steps,
                                float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                                int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                                float *probs_out_dev, void *stream);

/*
 * Actor-critic rollouts (ABI 4, additive; BUILD-DEFINED): the critic's estimate V(s_t) of the state each decision was
 * taken in, for a critic that shares the actor's trunk -- a Linear(in, 1) head next to the Linear(in, M) output layer.
 * Everything but one dot product is already computed by the policy's forward pass.  (A critic that is a separate network
 * is left to the trainer: it is one batched GEMM over the features slab.)
 *
 * head_dev: float32 [in + 1], Wv[0..in) then bv; in = width[n_hidden - 1], or F when n_hidden == 0.
 * Value: v = bv, then v = fmaf(Wv[k], y[k], v) for k = 0, 1, .., in - 1 in that order, y = the last hidden layer's
 * post-ReLU output (x when n_hidden == 0): the chain rule of every other output of abr_policy.  The value takes no part
 * in the argmax, the softmax or the exploration, and the scores are bit for bit what they are without it.
 * A lane whose done bits are set reports value 0.0f.
 */
typedef struct abr_policy_value {
    const float *head_dev;                /* device, 4-byte aligned, non-NULL */
    size_t head_bytes;                    /* == (in + 1) * 4 */
    int32_t reserved_[4];                 /* set to 0 */
} abr_policy_value;

/* abr_env_policy_select_sampled with value_out_dev float32 [n_lanes] (nullable).  smp with ABR_POLICY_ARGMAX gives
 * abr_env_policy_select's actions and a one-hot probs.  Validation (ABR_E_INVALID, nothing launched): pol, smp, then val
 * (non-NULL, head non-NULL and aligned, reserved_ zero), all before the handle; then weights_bytes and head_bytes against
 * the shape. */
int abr_env_policy_select_ac(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                             const abr_policy_value *val, int32_t *action_out_dev, float *features_out_dev,
                             float *scores_out_dev, float *probs_out_dev, float *value_out_dev, void *stream);

/* abr_env_step_policy_sampled with values_out_dev float32 [n_steps][n_lanes] (nullable), the value of the state each
 * decision was taken in, and last_value_out_dev float32 [n_lanes] (nullable), the value of each lane's state after the
 * last step: one more evaluation of the forward pass at the end of the call that stores no decision.  It is 0.0f
 * for a lane whose done bits are set; under auto_reset a lane that finished on the last step reports the re-armed episode's
 * first state (abr_gae never reads it there: done[n_steps - 1] ends the recurrence).  Every other output and the
 * workspace are byte for byte what abr_env_step_policy_sampled leaves.  Validation as abr_env_policy_select_ac, with
 * n_steps >= 1 before the handle; ABR_E_UNSUPPORTED on tick. */
int abr_env_step_policy_ac(abr_env *env, const abr_policy *pol, const abr_policy_sampling *smp,
                           const abr_policy_value *val, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                           uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev,
                           float *scores_out_dev, float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                           void *stream);

/*
 * The matrix engine of the learned policy (ABI 4, additive; BUILD-DEFINED): the same network evaluated as f32 MFMA
 * products (units as rows, env lanes as columns), which lifts the shape limits to 0..3 hidden layers of 1..128 units.
 * Everything above that abr_policy, abr_policy_sampling and abr_policy_value say holds word for word: the features and
 * their normalisation, the blob (per layer Wt [out][in] then b [out], unpadded), the chain of every output (acc = b[j],
 * then acc = fmaf(Wt[j][k], x[k], acc) for k ascending -- on gfx950 v_mfma_f32_32x32x2_f32 is bit for bit that chain,
 * subnormals kept), the ReLU, the first argmax, the exploration draw, exp_c, the softmax draw, probs, the value head over
 * the last hidden output, and a done lane's -1, zero columns and value 0.  Only the shape limits differ: for a shape inside
 * both limits a blob and a head are interchangeable and every output is bit-identical between the two engines.
 * One entry pair covers every mode: smp == NULL is the first argmax (abr_env_policy_select's decision) and requires
 * probs_out_dev == NULL; val == NULL requires the value outputs to be NULL.
 */
#define ABR_POLICY_MX_MAX_HIDDEN 3
#define ABR_POLICY_MX_MAX_WIDTH 128
typedef struct abr_policy_mx {
    int32_t window;                       /* W, 0..ABR_POLICY_MAX_WINDOW */
    int32_t n_hidden;                     /* 0..ABR_POLICY_MX_MAX_HIDDEN */
    int32_t width[ABR_POLICY_MX_MAX_HIDDEN + 1]; /* 1..ABR_POLICY_MX_MAX_WIDTH below n_hidden, 0 from n_hidden on */
    const float *weights_dev;             /* the blob (device, 4-byte aligned) */
    size_t weights_bytes;                 /* == abr_policy_mx_weights_bytes(this, n_rates) */
    const double *norm_dev;               /* float64 [2][F] (device, 8-byte aligned) or NULL */
    uint64_t seed;                        /* philox key of the exploration draw */
    uint64_t explore_threshold;           /* 0 .. 2^32 */
    int32_t reserved_[4];                 /* set to 0 */
} abr_policy_mx;

/* Bytes of the weight blob for pol's shape and n_rates (the pointers are not looked at); == abr_policy_weights_bytes on
 * a shape both structs can hold.  The largest (3 x 128, window 16, 16 rates) is 159 296. */
int abr_policy_mx_weights_bytes(const abr_policy_mx *pol, int32_t n_rates, size_t *bytes_out);

/* abr_env_policy_select_ac on the matrix engine; smp and val nullable as above.  Validation (ABR_E_INVALID, nothing
 * launched): pol (shape, window, reserved_ zero, weights non-NULL and aligned, norm aligned, threshold <= 2^32), smp and
 * val where given, probs_out_dev without smp, value_out_dev without val, all before the handle; then weights_bytes and
 * head_bytes against the environment's n_rates. */
int abr_env_policy_select_mx(abr_env *env, const abr_policy_mx *pol, const abr_policy_sampling *smp,
                             const abr_policy_value *val, int32_t *action_out_dev, float *features_out_dev,
                             float *scores_out_dev, float *probs_out_dev, float *value_out_dev, void *stream);

/* abr_env_step_policy_ac on the matrix engine: per decision the matrix kernel, then the download of that chunk;
 * last_value_out_dev is one more forward-only launch, and the workspace after the call is byte for byte what the lane
 * engine's rollout leaves.  Validation as abr_env_policy_select_mx (values_out_dev and last_value_out_dev need val), with
 * n_steps >= 1 before the handle; ABR_E_UNSUPPORTED on tick. */
int abr_env_step_policy_mx(abr_env *env, const abr_policy_mx *pol, const abr_policy_sampling *smp,
                           const abr_policy_value *val, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                           uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev,
                           float *scores_out_dev, float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                           void *stream);

/*
 * Policy populations (ABI 4, additive; BUILD-DEFINED): P networks of ONE shape in a single launch, one weight set per
 * group of lanes (evolution strategies, population-based training, checkpoint leagues, A/B runs of two actors).
 * A population shares everything but the weights: window, hidden widths, n_rates, normalisation, seed, exploration
 * threshold and the sampling struct are those of the one abr_policy / abr_policy_mx handed in.
 * Membership: LOCAL lane i of the environment (0 <= i < n_lanes) belongs to member i / group.  group is a multiple of
 * 256 (the workgroup of both policy kernels, so a workgroup serves one member), n_members == ceil(n_lanes / group), and
 * the last member may own fewer than `group` lanes.  Membership never looks at lane_id_base: the philox counters keep
 * using lane_id_base + i exactly as in the single-network entries.
 * Weights: dense float32 [n_members][weights_bytes / 4], 4-byte aligned; pol->weights_dev points at member 0 and
 * pol->weights_bytes is ONE member's size, abr_policy_weights_bytes (abr_policy_mx_weights_bytes) of the shape.  Member
 * m's blob is byte for byte what a single abr_policy of that shape takes.  Value heads: float32 [n_members][in + 1];
 * val->head_dev points at member 0's head and val->head_bytes is one head's size.
 * Numerics: for every lane of member m, every output (action, features, scores, probs, value, last_value, and obs,
 * reward, done and the workspace, which the environment writes) is bit for bit what the single-network entry of the same
 * engine gives on that lane with member m's blob and head.  That sentence is the whole numerical contract.
 */
typedef struct abr_policy_pop {
    int32_t n_members;      /* P >= 1 */
    int32_t group;          /* lanes per member, a multiple of 256 */
    int32_t reserved_[6];   /* 0 */
} abr_policy_pop;

/* abr_env_policy_select_ac for a population (lane engine).  smp == NULL is the first argmax (abr_env_policy_select's
 * decision) and requires probs_out_dev == NULL; val == NULL requires value_out_dev == NULL.  Validation (ABR_E_INVALID,
 * nothing launched): pol as abr_env_policy_select, smp and val where given, probs_out_dev without smp, value_out_dev
 * without val, then pop (non-NULL, n_members >= 1, group >= 256 and a multiple of 256, reserved_ zero,
 * n_members * (int64)group representable), all before the handle; then ONE member's weights_bytes and head_bytes against
 * the shape, then n_members == ceil(n_lanes / group). */
int abr_env_policy_select_pop(abr_env *env, const abr_policy *pol, const abr_policy_pop *pop,
                              const abr_policy_sampling *smp, const abr_policy_value *val, int32_t *action_out_dev,
                              float *features_out_dev, float *scores_out_dev, float *probs_out_dev, float *value_out_dev,
                              void *stream);

/* abr_env_step_policy_ac for a population (lane engine): outputs as there, smp and val nullable as above
 * (values_out_dev and last_value_out_dev need val).  The last_value launch uses the same member mapping.  Validation as
 * abr_env_policy_select_pop, with n_steps >= 1 after pop and before the handle; ABR_E_UNSUPPORTED on tick. */
int abr_env_step_policy_pop(abr_env *env, const abr_policy *pol, const abr_policy_pop *pop,
                            const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                            float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                            float *features_out_dev, float *scores_out_dev, float *probs_out_dev, float *values_out_dev,
                            float *last_value_out_dev, void *stream);

/* The same two entries on the matrix engine (abr_policy_mx): validation as abr_env_policy_select_mx /
 * abr_env_step_policy_mx with pop checked after val (and before n_steps), then as above after the handle. */
int abr_env_policy_select_mx_pop(abr_env *env, const abr_policy_mx *pol, const abr_policy_pop *pop,
                                 const abr_policy_sampling *smp, const abr_policy_value *val, int32_t *action_out_dev,
                                 float *features_out_dev, float *scores_out_dev, float *probs_out_dev,
                                 float *value_out_dev, void *stream);
int abr_env_step_policy_mx_pop(abr_env *env, const abr_policy_mx *pol, const abr_policy_pop *pop,
                               const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                               float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev,
                               int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                               float *probs_out_dev, float *values_out_dev, float *last_value_out_dev, void *stream);

/*
 * Recurrent learned policy (ABI 4, additive; BUILD-DEFINED): one GRU cell per lane, evaluated on the device, whose hidden
 * state persists across decisions and across launches and restarts with the lane's episode.  An actor that has to infer a
 * hidden network condition (a bandwidth regime) from what it has seen carries that belief in the state.
 *
 * Network: the features x[0..F) exactly as abr_policy defines them (the same norm_dev); one GRU cell of H units,
 * 1 <= H <= ABR_POLICY_GRU_MAX_HIDDEN; the output layer Linear(H, M) over the NEW hidden state h'; optionally an
 * abr_policy_value head over h' (in = H, head_bytes == (H + 1) * 4).
 * Blob: one float32 blob in torch.nn.GRUCell's own layout and gate order (r, z, n), so that a trained module copies over
 * with no permutation: W_ih [3H][F], W_hh [3H][H], b_ih [3H], b_hh [3H], then W_out [M][H], b_out [M]; unpadded
 * (abr_policy_gru_weights_bytes).
 * State: state_dev float32 [H][n_lanes], caller-owned device memory, 4-byte aligned, state_bytes == H * n_lanes * 4.  The
 * library keeps nothing else; the workspace is untouched (so a checkpoint of the workspace does not hold the state: the
 * caller saves the slab next to it).
 * h_in, the hidden state entering a decision, for a lane that takes one: +0.0f in every unit when c == 0 (c = chunk_id),
 * otherwise the lane's column of state_dev.  That is the whole episode-boundary rule: every path that starts an episode
 * (abr_env_reset, a masked reset, an auto_reset re-arm, the episode sampler) restarts the recurrence, and no environment
 * kernel knows of it.
 * Cell: every operation float32, round-to-nearest-even, one rounding each, in this order.  For unit j and gate g in
 * (r, z, n), six k-ordered chains, each from its bias:
 *   gi_g = b_ih[gH + j], then gi_g = fmaf(W_ih[gH + j][k], x[k], gi_g), k = 0 .. F-1
 *   gh_g = b_hh[gH + j], then gh_g = fmaf(W_hh[gH + j][k], h_in[k], gh_g), k = 0 .. H-1
 *   r = sig_c(gi_r + gh_r);  z = sig_c(gi_z + gh_z);  n = tanh_c(fmaf(r, gh_n, gi_n))
 *   d = h_in[j] - n;  h'[j] = fmaf(z, d, n)                      (GRUCell's n + z * (h - n))
 * Activations, on exp_c (abr_policy_sampling; its text is unchanged and its argument here is never positive):
 *   sig_c(v): a NaN v returns v.  Otherwise e = exp_c(-fabsf(v)), q = 1.0f + e, result (v >= 0 ? 1.0f : e) / q, the
 *     correctly rounded division.
 *   tanh_c(v): a NaN v returns v.  Otherwise e = exp_c(-2.0f * fabsf(v)) (the product is exact),
 *     t = (1.0f - e) / (1.0f + e), result copysignf(t, v).  tanh_c(+-0) = +-0; +-1 for |v| > 40.
 *   Both are accurate in ABSOLUTE terms only (sig_c(-90) = 0, not 8e-40; near 0 tanh_c's error does not shrink with v).
 *   Derivation, with u = 2^-24 (one rounding), exp_c = E (1 + d1), |d1| < 2u (its stated bound), E = exp(-|v|) or
 *   exp(-2|v|) in (0, 1], first order in u:
 *     sig_c, v >= 0: 1 / (1 + E): d1 enters through the denominator with weight E / (1 + E), then the sum and the
 *       quotient round: relative (2E / (1 + E) + 2) u, absolute ((4E + 2) / (1 + E)^2) u, which falls in E: <= 2u.
 *     sig_c, v < 0: E / (1 + E): d1's weight is 1 / (1 + E): absolute (E (4 + 2E) / (1 + E)^2) u, which rises in E: <= 1.5u.
 *       Below -80, exp_c is 0 and the true value is under 2e-35.
 *     tanh_c: T = (1 - E) / (1 + E), dT/dE = -2 / (1 + E)^2: d1 gives (4E / (1 + E)^2) u, the three roundings 3 T u:
 *       ((3 + 4E - 3E^2) / (1 + E)^2) u, which falls in E: <= 3u.
 *   |sig_c - sigmoid| <= 2^-23 and |tanh_c - tanh| <= 3 * 2^-24 (both times 1 + 2^-20 for the second-order terms).
 *   Measured against float64 on 1 310 203 points of [-90, 90]: 8.915e-8 (0.748 * 2^-23) and 8.895e-8 (0.497 * 3 * 2^-24).
 * Outputs: score[m] = b_out[m], then fmaf(W_out[m][k], h'[k], .), k ascending; the value head is the same chain over h'.
 * Then abr_policy's first argmax, exploration and abr_policy_sampling's decision, unchanged: the same philox block, the
 * same words, the same probs.
 * Commit: with commit != 0 a lane that takes a decision has h' written over its column of state_dev.  A lane whose done
 * bits are set takes no decision: action -1, its feature, score, probs and hidden-out columns 0.0f, value 0.0f, and its
 * column of state_dev is NOT touched.
 * Populations: abr_env_gru_select_pop / abr_env_gru_step_pop, below (one blob per lane group, one slab).
 * Not covered: sharded environments, LSTM cells and stacked cells.  (H above 64: abr_policy_gru_mx, below.)
 */
#define ABR_POLICY_GRU_MAX_HIDDEN 64
typedef struct abr_policy_gru {           /* 80 bytes, no padding */
    int32_t window;                       /* W, 0..ABR_POLICY_MAX_WINDOW */
    int32_t hidden;                       /* H, 1..ABR_POLICY_GRU_MAX_HIDDEN */
    const float *weights_dev;             /* the blob (device, 4-byte aligned) */
    size_t weights_bytes;                 /* == abr_policy_gru_weights_bytes(this, n_rates) */
    const double *norm_dev;               /* float64 [2][F] (device, 8-byte aligned) or NULL */
    float *state_dev;                     /* float32 [H][n_lanes] (device, 4-byte aligned, non-NULL) */
    size_t state_bytes;                   /* == H * n_lanes * 4 */
    uint64_t seed;                        /* philox key of the exploration draw */
    uint64_t explore_threshold;           /* 0 .. 2^32 */
    int32_t reserved_[4];                 /* set to 0 */
} abr_policy_gru;

/* Bytes of the weight blob for pol's shape (window, hidden; the pointers are not looked at) and n_rates:
 * 4 * (3H (F + H + 2) + M (H + 1)). */
int abr_policy_gru_weights_bytes(const abr_policy_gru *pol, int32_t n_rates, size_t *bytes_out);

/* The recurrent policy's decision for each lane on the environment's current state, no step.  One form for every mode, as
 * the matrix engine's: smp == NULL is the first argmax and requires probs_out_dev == NULL; val == NULL requires
 * value_out_dev == NULL.  Outputs as abr_env_policy_select_ac, and hidden_out_dev float32 [H][n_lanes] (nullable): h_in,
 * the state the decision was taken from AFTER the c == 0 rule -- what a trainer needs to recompute the step.  commit != 0
 * writes h' to state_dev (above); commit == 0 leaves state_dev byte for byte.
 * Validation (ABR_E_INVALID, nothing launched): the struct (window, hidden, reserved_ zero, weights and state non-NULL and
 * 4-byte aligned, norm 8-byte aligned, threshold <= 2^32), smp and val where given, probs_out_dev without smp,
 * value_out_dev without val, all before the handle; then weights_bytes, state_bytes and head_bytes against the
 * environment. */
int abr_env_policy_select_gru(abr_env *env, const abr_policy_gru *pol, const abr_policy_sampling *smp,
                              const abr_policy_value *val, int32_t commit, int32_t *action_out_dev,
                              float *features_out_dev, float *scores_out_dev, float *probs_out_dev, float *value_out_dev,
                              float *hidden_out_dev, void *stream);

/* n_steps fused decisions: outputs as abr_env_step_policy_ac, and hidden_out_dev float32 [n_steps][H][n_lanes] (nullable),
 * the h_in of every decision.  Every decision commits.  last_value_out_dev is one more forward-only launch with
 * commit = 0: it leaves state_dev byte for byte as the last decision left it.  Apart from the state slab the call is byte
 * for byte a loop of abr_env_policy_select_gru(commit = 1) then abr_env_step.  Validation as abr_env_policy_select_gru
 * (values_out_dev and last_value_out_dev need val), with n_steps >= 1 before the handle; ABR_E_UNSUPPORTED on tick. */
int abr_env_step_policy_gru(abr_env *env, const abr_policy_gru *pol, const abr_policy_sampling *smp,
                            const abr_policy_value *val, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                            uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev,
                            float *scores_out_dev, float *probs_out_dev, float *values_out_dev, float *last_value_out_dev,
                            float *hidden_out_dev, void *stream);

/*
 * The recurrent policy's matrix engine (ABI 4, additive; BUILD-DEFINED): a second engine with the arithmetic contract of
 * abr_policy_gru, word for word -- the same features, the same blob (GRUCell's own layout and gate order, then the
 * head, unpadded), the same state slab [H][n_lanes] and c == 0 rule, the same six k-ordered chains per unit (gi_g and
 * gh_g separate accumulators, each from its own bias, added after the chains), the same sig_c / tanh_c /
 * d = h_in[j] - n / h' = fmaf(z, d, n), the same output chains over h' and value head, the same argmax, exploration
 * and softmax draw, the same rules for commit, done lanes and hidden_out.  Only the width limit is lifted:
 * 1 <= H <= ABR_POLICY_GRU_MX_MAX_HIDDEN.  The chains are issued as v_mfma_f32_32x32x2_f32 (as abr_policy_mx's), whose
 * accumulation is the fmaf chain in k order: on a shape inside both limits (H <= 64) a blob, a head and a state slab are
 * interchangeable between the engines, and every output and the committed state are bit-identical.
 * abr_policy_gru_mx is a distinct type with abr_policy_gru's layout, as abr_policy_mx is next to abr_policy.
 * Populations: abr_env_gru_mx_select_pop / abr_env_gru_mx_step_pop, below (one blob per lane group, one slab).
 * Not covered: sharded environments, LSTM cells and stacked cells.
 */
#define ABR_POLICY_GRU_MX_MAX_HIDDEN 128
typedef struct abr_policy_gru_mx {        /* 80 bytes, no padding: field for field abr_policy_gru */
    int32_t window;                       /* W, 0..ABR_POLICY_MAX_WINDOW */
    int32_t hidden;                       /* H, 1..ABR_POLICY_GRU_MX_MAX_HIDDEN */
    const float *weights_dev;             /* the blob (device, 4-byte aligned) */
    size_t weights_bytes;                 /* == abr_policy_gru_mx_weights_bytes(this, n_rates) */
    const double *norm_dev;               /* float64 [2][F] (device, 8-byte aligned) or NULL */
    float *state_dev;                     /* float32 [H][n_lanes] (device, 4-byte aligned, non-NULL) */
    size_t state_bytes;                   /* == H * n_lanes * 4 */
    uint64_t seed;                        /* philox key of the exploration draw */
    uint64_t explore_threshold;           /* 0 .. 2^32 */
    int32_t reserved_[4];                 /* set to 0 */
} abr_policy_gru_mx;

/* As abr_policy_gru_weights_bytes, the same formula: 4 * (3H (F + H + 2) + M (H + 1)). */
int abr_policy_gru_mx_weights_bytes(const abr_policy_gru_mx *pol, int32_t n_rates, size_t *bytes_out);

/* abr_env_policy_select_gru on the matrix engine: the same parameters, outputs, commit rule, validation order and
 * messages. */
int abr_env_gru_mx_select(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_sampling *smp,
                          const abr_policy_value *val, int32_t commit, int32_t *action_out_dev, float *features_out_dev,
                          float *scores_out_dev, float *probs_out_dev, float *value_out_dev, float *hidden_out_dev,
                          void *stream);

/* abr_env_step_policy_gru on the matrix engine: every decision commits, last_value_out_dev is a forward-only launch that
 * commits nothing, byte for byte a loop of abr_env_gru_mx_select(commit = 1) then abr_env_step; ABR_E_UNSUPPORTED on
 * tick. */
int abr_env_gru_mx_step(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_sampling *smp,
                        const abr_policy_value *val, int32_t n_steps, float *obs_out_dev, float *reward_out_dev,
                        uint8_t *done_out_dev, int32_t *actions_out_dev, float *features_out_dev, float *scores_out_dev,
                        float *probs_out_dev, float *values_out_dev, float *last_value_out_dev, float *hidden_out_dev,
                        void *stream);

/*
 * Recurrent policy populations (ABI 4, additive; BUILD-DEFINED): abr_policy_pop, unchanged, over abr_policy_gru and
 * abr_policy_gru_mx -- P GRU cells of ONE shape in a single launch, one weight set per group of lanes, for the trainers
 * that need no backpropagation through time (evolution strategies, population-based training) and for leagues.
 * Membership: exactly abr_policy_pop's.  LOCAL lane i belongs to member i / group, group is a multiple of 256 (the
 * workgroup of both recurrent kernels), n_members == ceil(n_lanes / group), the last member may own fewer lanes, and
 * lane_id_base takes no part.
 * Weights: dense float32 [n_members][weights_bytes / 4]; pol->weights_dev points at member 0 and pol->weights_bytes is
 * ONE member's size, abr_policy_gru_weights_bytes of the shape.  Member m's row is byte for byte the blob a single
 * abr_policy_gru of that shape takes (GRUCell's layout, then the head, unpadded).  Value heads: float32
 * [n_members][H + 1]; val->head_dev points at member 0's head and val->head_bytes is one head's size.
 * State: still ONE slab, float32 [H][n_lanes], state_bytes == H * n_lanes * 4: members own disjoint columns.  The c == 0
 * rule, commit, the done-lane rule and hidden_out are abr_policy_gru's, word for word.
 * Numerics: on every lane of member m, every output (action, features, scores, probs, value, last_value, hidden_out),
 * the committed column of the state slab, and the workspace are bit for bit what the single-network entry of the same
 * engine gives on that lane with member m's blob and head.  That sentence is the whole numerical contract.
 * Not covered: sharded environments, LSTM cells and stacked cells; per-member window, norm, seed, exploration or sampling.
 */

/* abr_env_policy_select_gru for a population.  Validation (ABR_E_INVALID, nothing launched): everything
 * abr_env_policy_select_gru checks before the handle, then pop (non-NULL, n_members >= 1, group >= 256 and a multiple of
 * 256, reserved_ zero, n_members * (int64)group representable), then the handle; then ONE member's weights_bytes, the
 * slab's state_bytes and one head's head_bytes against the environment, then n_members == ceil(n_lanes / group). */
int abr_env_gru_select_pop(abr_env *env, const abr_policy_gru *pol, const abr_policy_pop *pop,
                                  const abr_policy_sampling *smp, const abr_policy_value *val, int32_t commit,
                                  int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                                  float *probs_out_dev, float *value_out_dev, float *hidden_out_dev, void *stream);

/* abr_env_step_policy_gru for a population: every decision commits, and the last_value launch (commit = 0) uses the same
 * member mapping.  Validation as abr_env_gru_select_pop, with n_steps >= 1 after pop and before the handle;
 * ABR_E_UNSUPPORTED on tick. */
int abr_env_gru_step_pop(abr_env *env, const abr_policy_gru *pol, const abr_policy_pop *pop,
                                const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                                float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                                float *features_out_dev, float *scores_out_dev, float *probs_out_dev, float *values_out_dev,
                                float *last_value_out_dev, float *hidden_out_dev, void *stream);

/* The same two entries on the matrix engine (abr_policy_gru_mx, H up to ABR_POLICY_GRU_MX_MAX_HIDDEN): the same
 * parameters, validation order and messages; on H <= 64 bit for bit the lane engine's population. */
int abr_env_gru_mx_select_pop(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_pop *pop,
                              const abr_policy_sampling *smp, const abr_policy_value *val, int32_t commit,
                              int32_t *action_out_dev, float *features_out_dev, float *scores_out_dev,
                              float *probs_out_dev, float *value_out_dev, float *hidden_out_dev, void *stream);
int abr_env_gru_mx_step_pop(abr_env *env, const abr_policy_gru_mx *pol, const abr_policy_pop *pop,
                            const abr_policy_sampling *smp, const abr_policy_value *val, int32_t n_steps,
                            float *obs_out_dev, float *reward_out_dev, uint8_t *done_out_dev, int32_t *actions_out_dev,
                            float *features_out_dev, float *scores_out_dev, float *probs_out_dev, float *values_out_dev,
                            float *last_value_out_dev, float *hidden_out_dev, void *stream);

/*
 * Generalised advantage estimation over the slabs of a fused rollout (no handle).  Device pointers, row stride n_lanes:
 * reward, values float32 [n_steps][n_lanes]; last_value float32 [n_lanes]; done uint8 [n_steps][n_lanes]; actions int32
 * [n_steps][n_lanes] or NULL (every step is live); outputs adv, ret float32 [n_steps][n_lanes], which may not overlap
 * the inputs.  gamma and lam are finite and in [0, 1].
 *
 * Exact: float32, round-to-nearest-even, one rounding per operation.  gl = gamma * lam.  Per lane i: A = 0,
 * nv = last_value[i]; then for t = n_steps - 1 down to 0, with r = reward[t][i], v = values[t][i]:
 *   a dead step (actions != NULL and actions[t][i] < 0: the lane took no decision) writes adv = ret = +0.0f and sets
 *     A = 0, nv = 0;
 *   otherwise, term = (done[t][i] != 0):
 *     q = term ? 0 : gamma * nv;  delta = (r + q) - v;  w = term ? 0 : gl * A;  A = delta + w;
 *     adv[t][i] = A;  ret[t][i] = A + v;  nv = v.
 * q and w are selects, not products with a mask: a non-finite value behind an episode end makes no NaN in front of it.
 * done[t] is set at the step that ends an episode and row t + 1 (under auto_reset) belongs to the next one, so the
 * recurrence restarts at every set byte.  EVERY done bit ends it: ABR_DONE_EPISODE, _TIMEOUT, _BADACT, _BADARG.  A lane
 * that timed out is never re-armed and has no next call site whose value could stand in for the truncated tail, so a
 * time-out is treated as a terminal state, not bootstrapped.
 * Refused (ABR_E_INVALID, nothing launched): n_steps < 1, n_lanes < 1, a NULL pointer other than actions, a float32 or
 * int32 pointer that is not 4-byte aligned, gamma or lam outside [0, 1] (NaN included).
 */
int abr_gae(const float *reward_dev, const float *values_dev, const float *last_value_dev, const uint8_t *done_dev,
            const int32_t *actions_dev, int32_t n_steps, int64_t n_lanes, float gamma, float lam, float *adv_out_dev,
            float *ret_out_dev, void *stream);

/*
 * Synthesise a bandwidth corpus on the device (no handle): a Markov chain over K bandwidth regimes with uniform noise
 * around each regime's level and per-regime outages, written over caller-owned trace arrays of abr_env_create's layout.
 * Build-defined: the reference has no generator.  Only entries [0, K) of each array are read; of a cumulative row only
 * [0, K - 1): the last cumulative value is implicitly 2^32.
 *
 * Exact: integers and float64 only, round-to-nearest-even, one rounding per operation, in this order.  For trace t
 * (global id g = trace_id_base + t) and sample i in [0, trace_len_dev[t]), with philox4 the philox4x32-10 block of
 * csrc/abr_lane_jump.h (key, lane, step, episode) and key = seed ^ 0x5452414345535953:
 *   s_-1 = #{ j < K - 1 : v0 >= init_cum[j] },          (v0, ..) = philox4(key, g, 0xFFFFFFFF, generation)
 *   s_i  = #{ j < K - 1 : w0 >= cum[s_(i-1)][j] },      (w0, w1, w2, w3) = philox4(key, g, i, generation)
 *   u = (double)(w1 >> 8) * 2^-24;  r = 2.0 * u - 1.0   (exact, in [-1, 1))
 *   x = level[s_i] * (1.0 + spread[s_i] * r);  x = +0.0 when w2 < outage_thr[s_i]
 *   traces_dev[trace_off_dev[t] + i] = x
 * With level >= 0 and spread <= 1 every sample is finite and >= 0: what abr_env_create requires of a trace.  generation
 * selects a fresh corpus from the same seed; a sub-range generated with trace_id_base = a equals rows [a, a + n_traces)
 * of the whole corpus.  A trace whose length on the device is < 1 is skipped; nothing outside the rows is written, and the
 * rows need no alignment beyond 8 bytes and need not be adjacent.  Runs on `stream` without synchronising.
 *
 * Regenerating the corpus a handle uses is legal at any point in stream order and takes effect for lanes that are reset
 * (or re-armed) afterwards: the library keeps nothing derived from the samples.  A lane that is mid-episode when its
 * corpus is regenerated is outside the contract: it stays bounded, because every sample is valid, but matches no replay.
 *
 * Refused (ABR_E_INVALID, nothing launched), the struct before the pointers: a NULL model; n_states outside 1..8;
 * reserved_ != 0; a level that is not finite or is negative; no state with level > 0 and outage_thr < 2^32 (no sample could
 * ever be positive); a spread that is NaN or outside [0, 1]; an outage_thr, init_cum or cum entry above 2^32; a cumulative
 * row that decreases (of the entries that are read); traces_dev, trace_off_dev or trace_len_dev NULL or not aligned to its element (8, 8 and 4 bytes);
 * n_traces < 1; trace_id_base < 0.
 */
#define ABR_TRACE_MAX_STATES 8
typedef struct abr_trace_model {
    int32_t  n_states;                                             /* K, 1..8 */
    int32_t  reserved_;                                            /* 0 */
    double   level[ABR_TRACE_MAX_STATES];                          /* regime bandwidth, finite, >= 0, same unit as the ladder */
    double   spread[ABR_TRACE_MAX_STATES];                         /* 0..1: relative half-width of the uniform noise */
    uint64_t outage_thr[ABR_TRACE_MAX_STATES];                     /* 0..2^32: a sample in regime s is 0.0 when word2 < outage_thr[s] */
    uint64_t init_cum[ABR_TRACE_MAX_STATES];                       /* 0..2^32, non-decreasing: cumulative initial distribution */
    uint64_t cum[ABR_TRACE_MAX_STATES][ABR_TRACE_MAX_STATES];      /* cum[s][j], 0..2^32, non-decreasing in j: cumulative row s of the transition matrix */
} abr_trace_model;              /* 776 bytes */
int abr_trace_synth(const abr_trace_model *model, uint64_t seed, uint32_t generation, int64_t trace_id_base,
                    double *traces_dev, const int64_t *trace_off_dev, const int32_t *trace_len_dev, int32_t n_traces,
                    void *stream);

/* Diagnostic: the full objective grid of ONE lane, J_out_dev float64
 * [n_rates^horizon], given explicit predictions pred_dev[horizon]. */
int abr_mpc_objective_grid(const abr_mpc_config *cfg, int32_t chunk, int32_t prev_bitrate,
                           double buffer_level, const double *pred_dev, const double *br_table_dev,
                           const double *sz_table_dev, double *J_out_dev, void *stream);

/* Diagnostic: count independent chains "x <- fl(x + c), up to n times, stop right after the
 * first result that is >= thr (stop_kind 0, c > 0), <= thr (1, c < 0) or < thr (2, c < 0)" --
 * the float64 sequences of Simulator.py:160-163 and :184,:190-194 -- advanced by the kernels'
 * exact closed form (csrc/abr_exact_jump.h) on the device.  estimate_bias 0 is the product
 * path; +4 / -4 spoil the jump-length estimate so that the exact fallback search runs.
 * Outputs per case: final x, additions performed, 1 if it stopped on the predicate.
 * stop_kind + 0x100 runs the form of the chains that the no-speeds kernel instances use, which tests no guard per segment
 * (abr_exact_jump.h: GUARDS_PROVEN); every n must then be in 1..2^20 and every x0, c, thr finite (not checked). */
int abr_debug_chain(int32_t stop_kind, int32_t estimate_bias, const double *x0_dev,
                    const double *c_dev, const double *thr_dev, const int32_t *n_dev, int64_t count,
                    double *x_out_dev, int32_t *a_out_dev, uint8_t *hit_out_dev, void *stream);

/* Diagnostic: count independent drains "x <- fl(x - sd), up to n times, stop right after the first result that is <= 0" --
 * buffer_level -= play_speed * dt, Simulator.py:184, :194 -- at ONE subtrahend sd for all cases, advanced on the device the way
 * the environment kernels do when every lane plays at the same speed: by the per-binade cascade built for levels below
 * max_level (csrc/abr_exact_jump.h: drain_cascade; abr_env_create builds it for max_buffer + chunk_length), or by the general
 * chain for a wave that holds a value at or above the cascade's top.  Outputs per case as abr_debug_chain; *stages_out
 * (nullable, host) = binades the cascade covers.  ABR_E_UNSUPPORTED when no cascade exists for (sd, max_level). */
int abr_debug_drain(double sd, double max_level, const double *x0_dev, const int32_t *n_dev, int64_t count,
                    double *x_out_dev, int32_t *a_out_dev, uint8_t *hit_out_dev, int32_t *stages_out, void *stream);

/* Diagnostic: a self-check of the PRODUCT build's role-split kernels (impl 2 and 5).  Their service code re-reads the launch's
 * parameter block from the kernel-argument segment every iteration instead of holding it in registers, which is only right
 * while that block is the kernels' first argument; a checking instance of each of the two kernel templates (the product
 * instances' signature) is launched once (one workgroup, no lane state touched) with a sentinel in the block and reports
 * whether the re-read saw it.  result_dev: uint32 [2] device memory (three-wave kernel, two-wave kernel): 1 = seen,
 * 2 = not seen, 0 = that launch never ran. */
int abr_debug_selfcheck(abr_env *env, uint32_t *result_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ABR_ENV_H */
