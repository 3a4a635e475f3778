"""BatchedABREnv: the reference's Simulator.run() tick loop (Simulator.py:93-210)
turned inside out into reset()/step(actions) over many independent lanes.

Host Python only holds PyTorch-ROCm tensors and calls the C ABI
(include/abr_env.h); all simulation runs in the HIP kernels of csrc/abr_env.hip.
"""
import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import _lib
from .episodes import EpisodeSampler
from .ledger import EpisodeLedger
from .quality import EpisodeQuality, utility_table
from .speed import LatencySpeedController
from .tracesynth import TraceModel
from ._lib import F64_DIM, F64_ROWS, OBS_DIM, OBS_ROWS
from .datamodel import MPD, NetworkInfo, QOEMetric


def pack_traces(traces: Sequence, device):
    """Ragged list of bandwidth traces -> (flat f64, offsets i64, lengths i32) on `device`."""
    ts = [torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in traces]
    if not ts or any(t.numel() == 0 for t in ts):
        raise ValueError("every trace needs at least one bandwidth sample")
    lens = torch.tensor([t.numel() for t in ts], dtype=torch.int32)
    off = torch.zeros(len(ts), dtype=torch.int64)
    off[1:] = torch.cumsum(lens[:-1].to(torch.int64), 0)
    flat = torch.cat(ts)
    # a NaN/inf/negative bandwidth can never complete a download: the lane would crawl to
    # max_ticks one real addition at a time (bounded, but pointlessly slow)
    if not bool(torch.isfinite(flat).all()) or bool((flat < 0).any()):
        raise ValueError("bandwidth traces must be finite and non-negative")
    return flat.to(device), off.to(device), lens.to(device)


class BoundOut(dict):
    """An output dict of step_random / step_script whose device pointers have been looked up once
    (BatchedABREnv.bind_out): a launch per call is then a ctypes call and nothing else.  The tensors
    must not be replaced afterwards."""
    ptrs = None


class BatchedABREnv:
    """n_lanes independent players, one per GPU thread.

    mpd / qoe_metric / network_info carry the reference's field names
    (datamodel.py).  reset() returns the observation at each lane's first
    get_next_bitrate call site (Simulator.py:155); step(actions) supplies that
    call's return value and returns (obs, reward, done) at the next one.
    Observations are float32 [OBS_DIM, n_lanes] (rows: _lib.OBS_ROWS); the exact
    float64 state is available through observe_f64() and state_view().
    """

    def __init__(self, mpd: MPD, qoe_metric: QOEMetric, network_info: NetworkInfo, n_lanes: int,
                 device="cuda", speed=1.0, auto_reset: bool = False, max_ticks: int = 0,
                 lane_id_base: int = 0, impl: str = "auto", library: Optional[str] = None, chunk_sizes=None):
        # `library`: a diagnostic build of the same ABI (tools/diag/csrc/Makefile -> tools/diag/lib), by path or file
        # name.  The product library holds only what `auto` can select plus the jump / split / tick cross-checks;
        # impl="async" / "ring3" (pipelines that were measured slower, kept for the parity tests and the records)
        # need such a library and are refused (ABR_E_UNSUPPORTED) by the product.
        self.lib = _lib.lib(library)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("BatchedABREnv runs on a ROCm device only (no CPU path exists)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._dev_index = self.device.index
        self.n_lanes = int(n_lanes)
        self.mpd, self.qoe_metric, self.network_info = mpd, qoe_metric, network_info
        # one ladder for the whole video (what run() indexes, Simulator.py:82,156) or, for an MPD
        # whose chunks differ (set_mpd's one-ladder-per-line file), a per-chunk table
        self.br_table = None
        if mpd.uniform():
            ladder = mpd.ladder()
        else:
            table = mpd.bitrate_table()
            if len(table) != int(mpd.video_length) or any(len(r) != len(table[0]) for r in table):
                raise ValueError("a per-chunk MPD needs video_length ladders of equal length")
            ladder = table[0]
            self.br_table = torch.tensor(table, dtype=torch.float64, device=self.device).contiguous()
            if not bool((self.br_table > 0).all()):
                raise ValueError("bitrates must be > 0")
        cfg = _lib.EnvConfig()
        cfg.n_rates, cfg.video_length = len(ladder), int(mpd.video_length)
        cfg.chunk_length, cfg.max_buffer = float(mpd.chunk_length), float(mpd.max_buffer)
        cfg.start_up_length, cfg.interval = float(mpd.start_up_length), float(network_info.interval)
        cfg.rebuffer_weight = float(qoe_metric.rebuffer_weight)
        cfg.variance_weight = float(qoe_metric.variance_weight)
        cfg.startup_weight = float(qoe_metric.startup_weight)
        cfg.latency_weight = float(getattr(qoe_metric, "latency_weight", 0.0))
        self.lane_speeds = None
        self.speed_controller = None
        self._speed_log = None
        if isinstance(speed, LatencySpeedController):
            # a closed-loop speed rule, evaluated in the kernels at every played chunk's first playing tick
            self.speed_controller = speed
            speed = 1.0
        elif torch.is_tensor(speed) or hasattr(speed, "__len__"):
            # per-lane play speeds: [N] = one constant speed per lane;
            # [rows, N] = a speed controller's answers, one row per played chunk
            # (Simulator.py:176-177; the last row repeats)
            ls = torch.as_tensor(speed, dtype=torch.float64)
            if ls.dim() == 1:
                ls = ls.reshape(1, -1)
            if (ls.dim() != 2 or ls.shape[1] != self.n_lanes or ls.shape[0] < 1
                    or not bool((ls > 0).all()) or not bool(torch.isfinite(ls).all())):
                raise ValueError("per-lane speeds must be [n_lanes] or [rows, n_lanes] finite values > 0")
            self.lane_speeds = ls.to(self.device).contiguous()
            speed = 1.0
        cfg.speed = float(speed)
        if len(ladder) > _lib.MAX_RATES:
            raise ValueError(f"at most {_lib.MAX_RATES} bitrates")
        for i, b in enumerate(ladder):
            cfg.ladder[i] = b
        cfg.max_ticks, cfg.auto_reset = int(max_ticks), int(bool(auto_reset))
        self.cfg = cfg
        self.n_rates, self.video_length = cfg.n_rates, cfg.video_length

        bw = network_info.bandwidths
        if torch.is_tensor(bw):
            bw = [bw] if bw.dim() == 1 else list(bw)
        elif len(bw) > 0 and not hasattr(bw[0], "__len__"):
            bw = [bw]              # one trace given as a flat list of floats
        with torch.cuda.device(self.device):
            self.traces, self.trace_off, self.trace_len = pack_traces(bw, self.device)
            self.n_traces = int(self.trace_len.numel())
            nbytes = C.c_size_t()
            self._check(self.lib.abr_env_workspace_bytes(C.byref(cfg), self.n_lanes, C.byref(nbytes)))
            self.workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            assert self.workspace.data_ptr() % 256 == 0
            h = C.c_void_p()
            self._check(self.lib.abr_env_create(
                C.byref(cfg), _lib.ptr(self.traces), _lib.ptr(self.trace_off),
                _lib.ptr(self.trace_len), self.n_traces, self.n_lanes, _lib.ptr(self.workspace),
                nbytes.value, self._stream(), C.byref(h)))
        self._h = h
        # the layout tag abr_env_create wrote into the workspace's last bytes, kept aside: what a state to be loaded must carry
        self._tag = self.workspace[-self.TAG_BYTES:].clone()
        if lane_id_base:
            self._check(self.lib.abr_env_set_lane_id_base(self._h, int(lane_id_base)))
        impls = {"jump": 0, "tick": 1, "split": 2, "auto": 3, "async": 4, "split3": 5, "ring3": 6, "pair3": 7}
        if impl not in impls:
            raise ValueError("impl must be 'auto' (default: the fastest at this size, see effective_impl()), "
                             "'split' / 'split3' (role-split event-driven kernels, two / three waves per 64 lanes), "
                             "'jump' (event-driven, one thread per lane) or 'tick' ('async' / 'ring3' only with "
                             "library=<a diagnostic build that carries them>)")
        self.impl = impl
        self._check(self.lib.abr_env_set_impl(self._h, impls[impl]))
        if self.lane_speeds is not None:
            self._check(self.lib.abr_env_set_speed_schedule(self._h, _lib.ptr(self.lane_speeds),
                                                           int(self.lane_speeds.shape[0])))
        if self.speed_controller is not None:
            self.set_speed_controller(self.speed_controller)
        if self.br_table is not None:
            self._check(self.lib.abr_env_set_bitrate_table(self._h, _lib.ptr(self.br_table)))
        # variable-bitrate video: what each chunk weighs (set_chunk_sizes).  None: bitrate * chunk_length, and Chunk.sizes
        # stays ignored -- MPDs with sizes are handed to the MPC controllers by callers that expect CBR downloads
        self.sz_table = None
        self._sz_keep = []
        if chunk_sizes is not None:
            self.set_chunk_sizes(chunk_sizes)
        self.obs = torch.zeros(OBS_DIM, self.n_lanes, dtype=torch.float32, device=self.device)
        self.reward = torch.zeros(self.n_lanes, dtype=torch.float32, device=self.device)
        self.done = torch.zeros(self.n_lanes, dtype=torch.uint8, device=self.device)
        self.trace_id = None
        self.start_offset = None
        self.episode_sampler = None
        self.episode_ledger = None
        self.quality = None

    def set_quality(self, weight=1.0, utility="identity", rows=None):
        """Add a video-quality term to the QoE (include/abr_env.h: abr_episode_quality).  The reward and episode_qoe() are
        pure costs, which the lowest bitrate minimises; while a quality model is installed, every step that completes a
        download reports reward - weight * u[chunk][action], and every finished episode's sum of u is recorded next to
        the episode ledger's record (quality.py: EpisodeQuality -- last(), totals(), ring(), records(ledger),
        per_trace(), per_member()), so that qoe_q = qoe - weight * quality is the episode's score.  utility: "identity"
        (u = the bitrate: with weight 1 the term BatchedMPCController's objective maximises), "log" (ln(br / lowest),
        BOLA's), "log_top" (ln(br / highest), the MPC's utility="log"), or a [video_length][n_rates] array; the tables are
        built on the host in float64 from the per-chunk bitrate table when the MPD has one.  rows: ring slots per lane,
        default the installed ledger's, else 1.  `weight` may also be an EpisodeQuality built for this env (to continue
        a restored one).  Returns the EpisodeQuality; env.quality holds it and keeps its tensors alive.
        set_quality(None) turns the term off: rewards are then what they were.  reset() zeroes the running sums of the
        lanes it resets and nothing else."""
        if weight is None:
            self._check(self.lib.abr_env_set_episode_quality(self._h, None))
            self.quality = None
            return None
        if isinstance(weight, EpisodeQuality):
            q = weight
            if q.n_lanes != self.n_lanes or q.device != self.device:
                raise ValueError(f"the quality model is for {q.n_lanes} lanes on {q.device}, this env has {self.n_lanes} "
                                 f"on {self.device}")
            if tuple(q.table.shape) != (self.video_length, self.n_rates):
                raise ValueError(f"the utility table must be [{self.video_length}][{self.n_rates}]")
        else:
            if rows is None:
                rows = self.episode_ledger.rows if self.episode_ledger is not None else 1
            br = self.br_table.cpu().numpy() if self.br_table is not None else [self.cfg.ladder[m] for m in range(self.n_rates)]
            table = utility_table(utility, br, self.video_length)
            with torch.cuda.device(self.device):
                q = EpisodeQuality(self.n_lanes, int(rows), weight, table, self.device)
        nbytes = C.c_size_t()
        self._check(self.lib.abr_env_quality_bytes(self.n_lanes, q.rows, C.byref(nbytes)))
        if nbytes.value != q.blob.numel():
            raise RuntimeError(f"quality layout mismatch: the library wants {nbytes.value} bytes, quality.py laid out "
                               f"{q.blob.numel()}")
        st = _lib.EpisodeQuality()
        st.wq, st.u_dev, st.base_dev, st.rows, st.reserved_ = q.weight, q.table.data_ptr(), q.blob.data_ptr(), q.rows, 0
        self._check(self.lib.abr_env_set_episode_quality(self._h, C.byref(st)))
        # the library holds the table's and the blob's addresses: the model must live as long as it is installed
        self.quality = q
        return q

    def set_chunk_sizes(self, table):
        """Variable-bitrate video (include/abr_env.h: abr_env_set_size_table): a size table decides what is DOWNLOADED,
        the bitrates keep deciding what is SCORED.  table: "mpd" (mpd.size_table(): Chunk.sizes where given -- what
        BatchedMPCController and FastMPCController plan on, so this is what makes them and the environment agree), an
        array-like [video_length][n_rates] in the ladder's unit x seconds, or None (back to bitrate * chunk_length).
        Checked on the host: shape, finite, > 0, < 2**960.  Latched like the bitrate table: the next reset of ALL lanes
        adopts it (a masked reset before that raises); at once on an env that has not been reset yet.  env.sz_table
        holds the device tensor the library reads."""
        if table is None:
            self._check(self.lib.abr_env_set_size_table(self._h, None))
            self.sz_table = None
            return None
        if isinstance(table, str):
            if table != "mpd":
                raise ValueError("chunk_sizes must be None, 'mpd' or a [video_length][n_rates] table")
            table = self.mpd.size_table()
            if any(len(r) != self.n_rates for r in table):
                raise ValueError(f"every chunk's sizes must have {self.n_rates} entries")
        t = torch.as_tensor(table, dtype=torch.float64)
        if tuple(t.shape) != (self.video_length, self.n_rates):
            raise ValueError(f"the size table must be [{self.video_length}][{self.n_rates}], got {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()) or not bool((t > 0).all()) or not bool((t < 2.0 ** 960).all()):
            raise ValueError("chunk sizes must be finite, > 0 and below 2**960")
        t = t.to(self.device).contiguous().clone()
        self._check(self.lib.abr_env_set_size_table(self._h, _lib.ptr(t)))
        # the library holds the table's address, and running episodes keep reading the one they started with
        self._sz_keep.append(t)
        self.sz_table = t
        return t

    def set_episode_ledger(self, rows):
        """Record every finished episode on the device (include/abr_env.h: abr_episode_ledger): while a ledger is
        installed, each lane whose episode ends with ABR_DONE_EPISODE or ABR_DONE_TIMEOUT appends one record -- the QoE
        terms episode_qoe() reads, their weighted sum, the episode's number, trace id, start offset, chunk count and done
        byte -- to a ring of `rows` slots per lane, and adds it to per-lane running totals.  Returns the EpisodeLedger
        (ledger.py: count(), totals(), ring(), records(), per_trace(), clear()); env.episode_ledger holds it and keeps
        its blob alive.  `rows` may also be an EpisodeLedger built for this env's lane count and device (to continue a
        restored one).  set_episode_ledger(None) turns recording off.  reset() never touches the ledger."""
        if rows is None:
            self._check(self.lib.abr_env_set_episode_ledger(self._h, None))
            self.episode_ledger = None
            return None
        if isinstance(rows, EpisodeLedger):
            led = rows
            if led.n_lanes != self.n_lanes or led.device != self.device:
                raise ValueError(f"the ledger is for {led.n_lanes} lanes on {led.device}, this env has {self.n_lanes} "
                                 f"on {self.device}")
        else:
            with torch.cuda.device(self.device):
                led = EpisodeLedger(self.n_lanes, int(rows), self.device)
        nbytes = C.c_size_t()
        self._check(self.lib.abr_env_ledger_bytes(self.n_lanes, led.rows, C.byref(nbytes)))
        if nbytes.value != led.blob.numel():
            raise RuntimeError(f"ledger layout mismatch: the library wants {nbytes.value} bytes, ledger.py laid out "
                               f"{led.blob.numel()}")
        st = _lib.EpisodeLedger()
        st.base_dev, st.rows, st.reserved_ = led.blob.data_ptr(), led.rows, 0
        self._check(self.lib.abr_env_set_episode_ledger(self._h, C.byref(st)))
        # the library holds the blob's address: the ledger must live as long as it is installed
        self.episode_ledger = led
        return led

    def set_episode_sampler(self, seed, pool=None, offset_span: int = 0):
        """Draw each episode's (trace, start offset) on the device (include/abr_env.h: abr_episode_sampler): under
        auto_reset a lane that ends its episode is re-armed on the pair drawn for its next episode number, and
        reset(sample=True) draws the pairs of the lanes it resets.  seed: the philox key (uint64); pool: None (every trace)
        or trace ids to draw from; offset_span: 0 (anywhere in the trace) or draw offsets from the first offset_span
        positions.  set_episode_sampler(None) turns sampling off.  The pool is checked on the host here; episodes.py:
        EpisodeSampler.draw computes the same pairs in numpy."""
        if seed is None:
            self._check(self.lib.abr_env_set_episode_sampler(self._h, None))
            self.episode_sampler, self._sampler_pool = None, None
            return
        es = EpisodeSampler(seed, pool, offset_span)
        es.check(self.n_traces)
        pool_t = None
        if es.pool is not None:
            pool_t = torch.from_numpy(es.pool).to(self.device).contiguous()
        st = _lib.EpisodeSampler()
        st.seed, st.pool = es.seed, (pool_t.data_ptr() if pool_t is not None else None)
        st.n_pool, st.offset_span = (int(pool_t.numel()) if pool_t is not None else 0), es.offset_span
        with torch.cuda.device(self.device):
            self._check(self.lib.abr_env_set_episode_sampler(self._h, C.byref(st)))
        # the library holds the pool's address: keep the tensor alive while the sampler is installed
        self.episode_sampler, self._sampler_pool = es, pool_t

    def synth_traces(self, model, seed, generation: int = 0):
        """Regenerate this environment's own corpus in place on the device (tracesynth.py: TraceModel; include/abr_env.h:
        abr_trace_synth): self.traces is overwritten through self.trace_off / self.trace_len, trace ids from 0, on the
        current stream, without synchronising, reading back or resetting.  Lanes reset (or re-armed) afterwards run on the
        new samples; a lane that is mid-episode is outside the contract, so follow with reset().  TraceModel.draw(seed,
        generation, range(n_traces), length) computes the same samples on the host."""
        if not isinstance(model, TraceModel):
            raise TypeError("synth_traces takes a TraceModel")
        st = model.struct()
        self._call(self.lib.abr_trace_synth, C.byref(st), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                   C.c_uint32(int(generation) & 0xFFFFFFFF), 0, _lib.ptr(self.traces), _lib.ptr(self.trace_off),
                   _lib.ptr(self.trace_len), self.n_traces)

    def episodes(self):
        """Each lane's current episode: dict(trace_id, start_offset, episode), int32 [N] each (fresh tensors, copied on the
        current stream)."""
        out = {k: torch.empty(self.n_lanes, dtype=torch.int32, device=self.device)
               for k in ("trace_id", "start_offset", "episode")}
        self._call(self.lib.abr_env_get_episode, self._h, _lib.ptr(out["trace_id"]), _lib.ptr(out["start_offset"]),
                   _lib.ptr(out["episode"]))
        return out

    def set_speed_controller(self, controller, log_rows: int = 0):
        """Install a LatencySpeedController (None: back to the constant config speed).  Latched like the per-lane speeds:
        the next reset of ALL lanes adopts it; at once on a handle that has not been reset yet.  log_rows > 0 keeps a log
        of its answers, float64 [log_rows, n_lanes] (speed_log()): row p holds the speed of played chunk p of the lane's
        current episode.  Replaces per-lane speeds or a schedule given before."""
        if controller is not None and not isinstance(controller, LatencySpeedController):
            raise TypeError("set_speed_controller takes a LatencySpeedController or None")
        log_rows = int(log_rows)
        if log_rows < 0:
            raise ValueError("log_rows must be >= 0")
        log = None
        if controller is not None and log_rows > 0:
            log = torch.zeros(log_rows, self.n_lanes, dtype=torch.float64, device=self.device)
        rule = controller.to_struct() if controller is not None else None
        self._check(self.lib.abr_env_set_speed_rule(self._h, C.byref(rule) if rule is not None else None,
                                                    _lib.ptr(log) if log is not None else None,
                                                    log_rows if log is not None else 0))
        # the library holds the log's address: keep the tensor alive as long as the rule may write it
        self._log_keep = getattr(self, "_log_keep", []) + ([log] if log is not None else [])
        self.speed_controller, self._speed_log = controller, log

    def speed_log(self):
        """The speed rule's log ([log_rows, n_lanes] float64 view; None without one): row p = the speed answered for
        played chunk p of each lane's current episode.  Rows a lane has not reached keep their earlier contents."""
        return self._speed_log

    # -- plumbing ----------------------------------------------------------
    def _check(self, rc):
        _lib.check(rc, self.lib)

    def _stream(self):
        return _lib.current_stream(self.device)

    def _call(self, fn, *args):
        """One C-ABI call with self.device current: the library launches on the stream it is
        handed, and HIP launches go to the CURRENT device."""
        if torch.cuda.current_device() == self._dev_index:     # the common case: no context switch to pay
            self._check(fn(*args, self._stream()))
        else:
            with torch.cuda.device(self.device):
                self._check(fn(*args, self._stream()))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.abr_env_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _i32(self, t, name):
        t = torch.as_tensor(t, device=self.device)
        if t.dtype != torch.int32:
            t = t.to(torch.int32)
        t = t.contiguous()
        if t.shape != (self.n_lanes,):
            raise ValueError(f"{name} must have shape ({self.n_lanes},), got {tuple(t.shape)}")
        return t

    def _rollout_out(self, n, want_obs=True, want_actions=True, actions_key=True):
        """Fresh output tensors of n fused decisions: dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N]); an
        entry that is not wanted is None, and actions_key=False leaves the actions key out (step_script)."""
        N, dev = self.n_lanes, self.device
        out = dict(obs=torch.empty(n, OBS_DIM, N, dtype=torch.float32, device=dev) if want_obs else None,
                   reward=torch.empty(n, N, dtype=torch.float32, device=dev),
                   done=torch.empty(n, N, dtype=torch.uint8, device=dev))
        if actions_key:
            out["actions"] = torch.empty(n, N, dtype=torch.int32, device=dev) if want_actions else None
        return out

    def _rollout(self, fn, head, n, out, want_obs, want_actions):
        """A rollout entry fn(handle, *head, n, obs, reward, done, actions) into `out` (None: a fresh _rollout_out)."""
        if out is None:
            out = self._rollout_out(n, want_obs, want_actions)
        self._call(fn, self._h, *head, n, *(_lib.ptr(out.get(k)) for k in ("obs", "reward", "done", "actions")))
        return out

    # -- the step surface --------------------------------------------------
    def reset(self, trace_id=None, start_offset=None, mask=None, check=False, sample=False):
        """Simulator.py:95-133 + idle ticks to the first ABR call.  Default assignment: lane i -> trace
        i % n_traces, offset 0.  `mask`: only lanes with a non-zero byte are reset (a masked reset inside an RL loop).

        No device-to-host synchronisation happens here: a lane whose trace id is outside [0, n_traces) or whose start
        offset is negative is frozen ON THE DEVICE with ABR_DONE_BADARG in its done byte (the reference would raise
        IndexError at Simulator.py:159); the observation returned for it looks like a fresh lane's.  `done_after_reset()`
        reads the lanes' done bytes as they stand (a zero-copy view, no step needed) so that a caller can see such lanes
        without a step.  check=True validates on the host first and raises ValueError instead -- before this object or
        the device state changes -- at the price of two synchronisations.

        sample=True (with an episode sampler installed, set_episode_sampler): every reset lane runs the sampler's pair for
        its new episode number; trace_id / start_offset must then be None.  self.trace_id / self.start_offset then hold
        each lane's pair as episodes() reports it after the reset."""
        if sample:
            if trace_id is not None or start_offset is not None:
                raise ValueError("reset(sample=True) draws the trace ids and start offsets: pass neither")
            if self.episode_sampler is None:
                raise ValueError("reset(sample=True) needs an episode sampler (set_episode_sampler)")
            m = None
            if mask is not None:
                m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            self._call(self.lib.abr_env_reset, self._h, None, None, _lib.ptr(m), _lib.ptr(self.obs))
            ep = self.episodes()
            self.trace_id, self.start_offset = ep["trace_id"], ep["start_offset"]
            return self.obs
        if trace_id is None:
            trace_id = torch.arange(self.n_lanes, device=self.device, dtype=torch.int32) % self.n_traces
        tid = self._i32(trace_id, "trace_id")
        if start_offset is None:
            start_offset = torch.zeros(self.n_lanes, dtype=torch.int32, device=self.device)
        off = self._i32(start_offset, "start_offset")
        if check:                                  # before anything of this object changes
            if int(tid.min()) < 0 or int(tid.max()) >= self.n_traces:
                raise ValueError("trace_id out of range")
            if int(off.min()) < 0:
                raise ValueError("start_offset must be >= 0")
        self.trace_id, self.start_offset = tid, off
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._call(self.lib.abr_env_reset, self._h, _lib.ptr(self.trace_id),
                   _lib.ptr(self.start_offset), _lib.ptr(m), _lib.ptr(self.obs))
        return self.obs

    def done_after_reset(self):
        """The lanes' done bytes as they stand in the workspace (uint8 [N], zero-copy): ABR_DONE_BADARG for a lane the last
        reset() froze because of its trace id / start offset, 0 for a lane that is running."""
        return self.mpc_inputs()[5]

    def step(self, actions):
        """One chunk per lane.  Returns (obs f32[OBS_DIM,N], reward f32[N], done u8[N]);
        the tensors are reused across calls."""
        a = self._i32(actions, "actions")
        self._call(self.lib.abr_env_step, self._h, _lib.ptr(a), _lib.ptr(self.obs),
                   _lib.ptr(self.reward), _lib.ptr(self.done))
        return self.obs, self.reward, self.done

    # the Pensieve-style name BASELINE.json uses for the same call
    get_video_chunk = step

    def step_random(self, n_steps: int, seed: int, out=None, want_actions=True):
        """n_steps fused decisions per lane under the built-in counter-based
        random policy.  Returns dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N])."""
        n = int(n_steps)
        if out is None:
            out = self._rollout_out(n, want_actions=want_actions)
        ptrs = getattr(out, "ptrs", None)
        if ptrs is None:
            ptrs = (_lib.ptr(out.get("obs")), _lib.ptr(out.get("reward")), _lib.ptr(out.get("done")),
                    _lib.ptr(out.get("actions")))
        self._call(self.lib.abr_env_step_random, self._h, n, C.c_uint64(int(seed) & (2 ** 64 - 1)), *ptrs)
        return out

    def bind_out(self, out):
        """Look the device pointers of an output dict (obs / reward / done / actions, any of them None) up
        once; pass the result as `out=` to step_random."""
        b = BoundOut(out)
        b.ptrs = (_lib.ptr(out.get("obs")), _lib.ptr(out.get("reward")), _lib.ptr(out.get("done")),
                  _lib.ptr(out.get("actions")))
        return b

    def step_script(self, actions, out=None):
        """len(actions) fused decisions per lane with the ABR controller's answers given up front:
        actions int32 [n_steps, N] (what run() does with a scripted abr_controller,
        Simulator.py:155).  Returns dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N])."""
        a = torch.as_tensor(actions, device=self.device)
        if a.dtype != torch.int32:
            a = a.to(torch.int32)
        a = a.contiguous()
        if a.dim() != 2 or a.shape[1] != self.n_lanes or a.shape[0] < 1:
            raise ValueError(f"actions must have shape (n_steps, {self.n_lanes}), got {tuple(a.shape)}")
        n = int(a.shape[0])
        if out is None:
            out = self._rollout_out(n, actions_key=False)
        self._call(self.lib.abr_env_step_script, self._h, n, _lib.ptr(a), _lib.ptr(out.get("obs")),
                   _lib.ptr(out.get("reward")), _lib.ptr(out.get("done")))
        return out

    def effective_impl(self, fused: bool = False):
        """Name of the kernels the handle resolves to right now ('auto' is a policy, not a kernel): fused=True for a
        step_random / step_script call of MORE than one decision, False for launches of one decision (step, step_mpc,
        and a fused call with n_steps == 1) -- under 'auto' those resolve to 'jump' at every size (include/abr_env.h)."""
        v = C.c_int32()
        self._check(self.lib.abr_env_get_effective_impl(self._h, int(bool(fused)), C.byref(v)))
        return {0: "jump", 1: "tick", 2: "split", 4: "async", 5: "split3", 6: "ring3", 7: "pair3"}[v.value]

    def general_instance(self, fused: bool = False) -> bool:
        """True while the handle's step launches run the kernels' general instances (the per-lane play-speed code, chains
        that test their guards in every segment) and not the slimmer no-speeds ones: a latched speed feature, an episode
        sampler, a quality model, a size table in force or pending (set_chunk_sizes), or a configuration that fails the host's proof for the unguarded chains -- a trace
        interval shorter than one 0.01 s tick, max_ticks above 2^20 (include/abr_env.h: abr_env_get_effective_impl)."""
        v = C.c_int32()
        self._check(self.lib.abr_env_get_effective_impl(self._h, int(bool(fused)) | 2, C.byref(v)))
        return bool(v.value & 0x100)

    def step_mpc(self, controller, n_steps: int, out=None, want_obs=True, want_actions=True):
        """n_steps decisions per lane taken by `controller` (a BatchedMPCController whose
        tables match this environment) on the device: next_bitrate() on each lane's own
        state, then the download, with no host work between decisions (a method="robust" controller runs
        abr_env_step_mpc_robust with its own per-lane state).  Returns
        dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N])."""
        n = int(n_steps)
        method, utility = getattr(controller, "method", "harmonic"), getattr(controller, "utility", "identity")
        if method != "robust" and (method != "harmonic" or utility != "identity"):
            # abr_env_step_mpc runs the harmonic predictor and the identity utility: anything else would be ignored
            raise ValueError(f"step_mpc runs method='harmonic' with utility='identity', or method='robust'; this "
                             f"controller has method={method!r}, utility={utility!r}")
        br, sz = controller._tables()
        cfg = controller.config()
        if method == "robust":
            # RobustMPC: the controller's per-lane state rides along; the estimates go through the workspace's scratch
            rob = controller.robust_options(self.n_lanes)
            return self._rollout(self.lib.abr_env_step_mpc_robust, (C.byref(cfg), C.byref(rob), _lib.ptr(br), _lib.ptr(sz)),
                                 n, out, want_obs, want_actions)
        return self._rollout(self.lib.abr_env_step_mpc, (C.byref(cfg), _lib.ptr(br), _lib.ptr(sz)), n, out, want_obs,
                             want_actions)

    def step_rule(self, controller, n_steps: int, out=None, want_obs=True, want_actions=True):
        """n_steps decisions per lane taken by a bitrate rule (rules.py: BufferBasedController, RateBasedController,
        BolaController; fastmpc.py: FastMPCController, which runs abr_env_step_fastmpc on its table) on the device, on each
        lane's own call-site state, with no host work between decisions.  Runs the one-thread-per-lane kernel under 'auto'
        and 'jump', the tick kernel under 'tick'; 'split' / 'split3' are refused (include/abr_env.h).  Returns
        dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N])."""
        n = int(n_steps)
        if getattr(controller, "method", None) == "fastmpc":
            cfg, fm, table = controller.bound()
            return self._rollout(self.lib.abr_env_step_fastmpc, (C.byref(cfg), C.byref(fm), _lib.ptr(table)), n, out,
                                 want_obs, want_actions)
        return self._rollout(self.lib.abr_env_step_rule, (C.byref(controller.config()),), n, out, want_obs, want_actions)

    def step_plan(self, controller, n_steps: int, out=None, want_obs=True, want_actions=True, forecast=None):
        """n_steps decisions per lane taken by forecast MPC (planner.py: ForecastMPCController) on the device: per decision
        the throughput forecast, the exhaustive plan on it and the download, with no host work between decisions
        (abr_env_step_plan).  `forecast` (float64 [N]) replaces the built-in forecast at every decision: a fixed belief.
        Finished lanes take no decision; "no decision" downloads bitrate 0 and is reported as 0.  Every event-driven
        kernel; 'tick' is refused.  Returns dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N])."""
        n = int(n_steps)
        return self._rollout(self.lib.abr_env_step_plan, (C.byref(controller.config(forecast)),), n, out, want_obs,
                             want_actions)

    def step_policy(self, controller, n_steps: int, out=None, want_obs=True, want_actions=True, want_features=False,
                    want_scores=False, want_probs=False, want_values=False, want_hidden=False):
        """n_steps decisions per lane taken by a learned policy (policy.py: PolicyController) on the device, each one the
        policy kernel on every lane's own call-site state followed by the download of that chunk, with no host work
        between decisions.  Every event-driven kernel; 'tick' is refused (include/abr_env.h).  Returns
        dict(obs[n,OBS_DIM,N], reward[n,N], done[n,N], actions[n,N], features[n,F,N], scores[n,M,N], probs[n,M,N]);
        an entry that is not wanted is None.  A controller with sample="softmax" draws each action on the device
        (abr_env_step_policy_sampled); probs is the policy's distribution at each decision, before exploration.
        want_values=True (a controller with a value head; ValueError without one) adds values[n,N], the critic's V of the
        state each decision was taken in, and last_value[N], V of the state the launch leaves behind -- what
        advantage.gae needs next to reward, done and actions (abr_env_step_policy_ac).  A controller built with
        engine="matrix" runs the same rollout on the MFMA kernel (abr_env_step_policy_mx), with the same outputs.
        A policy.PolicyPopulation rolls out P networks at once, member m on its own lane group, with the same dict and
        flags (abr_env_step_policy_pop, abr_env_step_policy_mx_pop).
        A policy.RecurrentPolicyController rolls out its GRU cell (abr_env_step_policy_gru): every decision advances
        controller.hidden, and want_hidden=True adds hidden[n,H,N], the state each decision was taken from (zeros at a
        lane's first chunk) -- with features, what a trainer needs to recompute each step in torch.  Built with
        engine="matrix" it rolls out on the MFMA kernel (abr_env_gru_mx_step), H up to 128, with the same outputs.
        A policy.RecurrentPolicyPopulation rolls out P GRU cells at once, member m on its own lane group and its own
        columns of the one hidden slab (abr_env_gru_step_pop, abr_env_gru_mx_step_pop), with the same dict and flags."""
        n = int(n_steps)
        recurrent = getattr(controller, "method", None) in ("policy_gru", "policy_gru_population")
        if want_hidden and not recurrent:
            raise ValueError("want_hidden needs a RecurrentPolicyController or a RecurrentPolicyPopulation")
        pol = controller.bound(self)
        val = controller.value() if want_values or (out is not None and out.get("values") is not None) else None
        if out is None:
            out = self._rollout_out(n, want_obs, want_actions)
            N, dev = self.n_lanes, self.device
            out["features"] = (torch.empty(n, controller.feature_dim, N, dtype=torch.float32, device=dev)
                               if want_features else None)
            out["scores"] = torch.empty(n, self.n_rates, N, dtype=torch.float32, device=dev) if want_scores else None
            out["probs"] = torch.empty(n, self.n_rates, N, dtype=torch.float32, device=dev) if want_probs else None
            if val is not None:
                out["values"] = torch.empty(n, N, dtype=torch.float32, device=dev)
                out["last_value"] = torch.empty(N, dtype=torch.float32, device=dev)
            if want_hidden:
                out["hidden"] = torch.empty(n, controller.hidden_size, N, dtype=torch.float32, device=dev)
        self._policy_call(controller, pol, val, out, n_steps=n)
        return out

    _SELECT_OUT = ("actions", "features", "scores", "probs", "value", "hidden")
    _STEP_OUT = ("obs", "reward", "done", "actions", "features", "scores", "probs", "values", "last_value", "hidden")

    def _policy_call(self, controller, pol, val, out, n_steps=None, commit=None):
        """The one call behind every learned-policy select (n_steps None) and every step_policy.  controller.entries(val,
        probs wanted) names the (select, step) pair of C entry points it takes, the structs they take after the policy's,
        and how many of the optional output groups -- probs; value(s); hidden -- they have; the rest is the same for all:
        n_steps (or the recurrent select's commit), then the outputs in the header's order, None where not wanted."""
        (select, step), structs, groups = controller.entries(val, out.get("probs") is not None)
        lead = [C.byref(pol)] + [C.byref(s) if s is not None else None for s in structs]
        if n_steps is None:
            name, keys = select, self._SELECT_OUT[:3 + groups]
            lead += [] if commit is None else [int(bool(commit))]
        else:
            name, keys = step, self._STEP_OUT[:6 + (0, 1, 3, 4)[groups]]
            lead.append(n_steps)
        self._call(getattr(self.lib, name), self._h, *lead, *(_lib.ptr(out.get(k)) for k in keys))

    # -- exact state -------------------------------------------------------
    def observe_f64(self):
        """dict of float64 [N] tensors: everything the reference's run() frame holds
        at the call site (rows: _lib.F64_ROWS)."""
        out = torch.empty(F64_DIM, self.n_lanes, dtype=torch.float64, device=self.device)
        self._call(self.lib.abr_env_observe_f64, self._h, _lib.ptr(out))
        return {k: out[i] for i, k in enumerate(F64_ROWS)}

    def episode_qoe(self, quality=False):
        """calculate_qoe (Simulator.py:79-86) of each lane's (last) finished episode, float64 [N].  quality=True (with a
        quality model installed, set_quality): qoe - weight * the episode's quality sum, the joined record's qoe_q."""
        out = torch.empty(self.n_lanes, dtype=torch.float64, device=self.device)
        self._call(self.lib.abr_env_episode_qoe, self._h, _lib.ptr(out))
        if quality:
            if self.quality is None:
                raise ValueError("episode_qoe(quality=True) needs a quality model (set_quality)")
            q = torch.empty(self.n_lanes, dtype=torch.float64, device=self.device)
            self._call(self.lib.abr_env_episode_quality, self._h, _lib.ptr(q))
            return out - self.quality.weight * q
        return out

    def state_view(self):
        v = _lib.StateView()
        self._check(self.lib.abr_env_get_state(self._h, C.byref(v)))
        return v

    def _view(self, addr, dtype, shape):
        """Zero-copy tensor over a region of the workspace."""
        off = addr - self.workspace.data_ptr()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        return self.workspace[off:off + nbytes].view(dtype).view(*shape)

    def history(self):
        """(previous_bitrates u8[V,N], previous_bandwidths f64[V,N]) -- rows >= chunk_id are stale."""
        v = self.state_view()
        return (self._view(v.action_hist, torch.uint8, (self.video_length, self.n_lanes)),
                self._view(v.bw_hist, torch.float64, (self.video_length, self.n_lanes)))

    def mpc_inputs(self):
        """Zero-copy float64/int32 tensors the MPC kernel reads and mutates (D9):
        (chunk_id, last_bitrate, buffer_level, hist_n, hist_sum_inv, done)."""
        v = self.state_view()
        N = self.n_lanes
        return (self._view(v.chunk_id, torch.int32, (N,)), self._view(v.last_bitrate, torch.int32, (N,)),
                self._view(v.buffer_level, torch.float64, (N,)), self._view(v.hist_n, torch.float64, (N,)),
                self._view(v.hist_sum_inv, torch.float64, (N,)), self._view(v.done, torch.uint8, (N,)))

    # -- fork ---------------------------------------------------------------
    def fork(self, src, dst=None, update_pairs=True):
        """Copy lanes on the device (include/abr_env.h: abr_env_fork): lane dst[i] becomes a byte-for-byte copy of lane
        src[i] as it was before the call -- state rows, action and bandwidth history, the quality model's running sum and
        this env's obs columns -- and continues exactly as src[i] would have.  src, dst: int32 tensors of equal length;
        src[i] = -1 (or any index outside the lanes, on either side) skips the pair; dst=None means dst[i] = i.  src may
        repeat a lane and the two may overlap in any way (a permutation included); dst values must be distinct.  The
        ledger's and the quality model's records stay with the slot.  self.trace_id / self.start_offset follow by tensor
        indexing; controller-side state (a RobustMPC state, a GRU's hidden rows) is the caller's: t[:, dst] = t[:, src].
        update_pairs=False leaves the two bookkeeping tensors alone (a caller whose copies stay on their source's pair).
        Enqueued on the current stream; nothing synchronises.  Refused while per-lane speeds or a schedule are set."""
        s = torch.as_tensor(src, device=self.device)
        s = (s if s.dtype == torch.int32 else s.to(torch.int32)).contiguous()
        if s.dim() != 1:
            raise ValueError("src must be a 1-d tensor of lane indices")
        d = None
        if dst is not None:
            d = torch.as_tensor(dst, device=self.device)
            d = (d if d.dtype == torch.int32 else d.to(torch.int32)).contiguous()
            if d.shape != s.shape:
                raise ValueError(f"dst must have src's shape {tuple(s.shape)}, got {tuple(d.shape)}")
        count = int(s.numel())
        if count == 0:
            return
        need = C.c_size_t()
        self._check(self.lib.abr_env_fork_scratch_bytes(self._h, count, C.byref(need)))
        scratch = getattr(self, "_fork_scratch", None)
        if scratch is None or scratch.numel() < need.value:
            with torch.cuda.device(self.device):
                scratch = self._fork_scratch = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        self._call(self.lib.abr_env_fork, self._h, _lib.ptr(s), _lib.ptr(d), count, _lib.ptr(scratch),
                   C.c_size_t(scratch.numel()), _lib.ptr(self.obs))
        if not update_pairs or self.trace_id is None or self.start_offset is None:
            return
        # the same pairs on the two bookkeeping tensors (fresh tensors: the old ones may be the caller's)
        si = s.long()
        ok = (si >= 0) & (si < self.n_lanes)
        si = si.clamp(0, self.n_lanes - 1)
        if d is None and count == self.n_lanes:                 # every lane names its source: one gather per tensor
            self.trace_id = torch.where(ok, self.trace_id[si], self.trace_id)
            self.start_offset = torch.where(ok, self.start_offset[si], self.start_offset)
            return
        di = torch.arange(count, device=self.device) if d is None else d.long()
        ok &= (di >= 0) & (di < self.n_lanes)
        di = torch.where(ok, di, self.n_lanes)                  # skipped pairs land in a spare slot
        for name in ("trace_id", "start_offset"):
            t = getattr(self, name)
            new = torch.cat([t, t[:1]])
            new[di] = t[si]
            setattr(self, name, new[:self.n_lanes].contiguous())

    # -- checkpoint / resume ------------------------------------------------
    TAG_BYTES = 256    # the workspace's last 256 bytes: its layout tag (include/abr_env.h, ABI 4)

    def state_dict(self):
        """All simulator state is the workspace tensor (the reference keeps it in
        run() locals and cannot checkpoint).  The dict is stamped with the ABI version and the
        workspace size it was taken under; the workspace itself ends in the library's layout tag."""
        sd = dict(workspace=self.workspace.clone(), trace_id=self.trace_id, start_offset=self.start_offset,
                  abi_version=_lib.ABI_VERSION, workspace_bytes=int(self.workspace.numel()))
        if self.quality is not None:           # the running sums are mid-episode state; the key exists only with a model
            sd["quality"] = self.quality.state_dict()
        return sd

    def load_state_dict(self, sd):
        """Refuses -- before anything is copied -- a state that was taken under another ABI version (the lane-state layout
        changes between versions; sizes can coincide), with another lane count or another configuration: the stamp of
        state_dict() and the layout tag at the end of the saved workspace are compared with this handle's own."""
        if sd.get("abi_version") != _lib.ABI_VERSION:
            raise ValueError(f"state_dict was taken under ABI version {sd.get('abi_version')}, this library is version "
                             f"{_lib.ABI_VERSION}: the workspace layout differs, the checkpoint cannot be restored")
        w = sd["workspace"]
        if w.numel() != self.workspace.numel() or sd.get("workspace_bytes") != self.workspace.numel():
            raise ValueError("workspace size mismatch: different config or lane count")
        if not torch.equal(w[-self.TAG_BYTES:].cpu(), self._tag.cpu()):
            raise ValueError("workspace layout tag mismatch: the checkpoint belongs to another lane count, configuration "
                             "or library version")
        if sd.get("quality") is not None and self.quality is not None:
            self.quality.load_state_dict(sd["quality"])        # refuses another shape, weight or table before anything is copied
        self.workspace.copy_(w)
        self.trace_id, self.start_offset = sd["trace_id"], sd["start_offset"]
        # the handle now carries episodes in flight (a freshly built one had none): the speeds /
        # bitrate table given to __init__ are in force, later setter calls are latched again
        self._check(self.lib.abr_env_notify_restore(self._h))


def obs_dict(obs):
    """Name the rows of an observation tensor."""
    return {k: obs[..., i, :] for i, k in enumerate(OBS_ROWS)}
