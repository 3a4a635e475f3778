"""FastMPC (Yin et al., SIGCOMM 2015): the MPC search run once, on the device, over a quantised state space -- (chunk row,
previous bitrate, buffer level, throughput estimate) -- and a table lookup per decision.  The table's contract (what each
entry is, how a lane finds its entry, the blob's layout) is include/abr_env.h: abr_fastmpc; the lookup is evaluated inside
the environment kernels like the bitrate rules (csrc/abr_lane_jump.h: fastmpc_lookup).

    ctl = FastMPCController(EnvPlayer(env), horizon=5, window=5)
    out = env.step_rule(ctl, 48)            # builds the table on first use, then 48 fused decisions per lane
    a = ctl.next_bitrate()                  # or one decision per lane on the current state, then env.step(a)
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .mpc import BatchedMPCController

DEFAULT_POINTS = 64


def arithmetic_edges(points):
    """Edges halfway between neighbouring points: (p[k] + p[k+1]) / 2."""
    p = np.asarray(points, np.float64)
    return (p[:-1] + p[1:]) / 2.0


def geometric_edges(points):
    """Edges at the geometric mean of neighbouring points: sqrt(p[k] * p[k+1])."""
    p = np.asarray(points, np.float64)
    return np.sqrt(p[:-1] * p[1:])


class FastMPCController:
    """FastMPC over `player` (the protocol of BatchedMPCController: get_mpd(), get_qoe_metric(), and `player.env` for
    next_bitrate()).  horizon, clip_horizon and utility as BatchedMPCController; window: the harmonic mean of the last
    `window` throughputs is the estimate the table is read at.

    Grids (float64, 1..256 points each): buffer_points default to 64 points evenly spaced over [0, max_buffer +
    chunk_length] with arithmetic-midpoint edges; tput_points to 64 geometric points from min(bitrate) / 4 to
    max(bitrate) * 4 with geometric-midpoint edges.  Points given without edges get those same midpoints.
    layout: "uniform" (rows = horizon; needs identical bitrates and sizes for every chunk and horizon < video_length),
    "per_chunk" (rows = video_length), or None: uniform when the MPD allows it.

    The table is built lazily (build(); again after build(force=True) or when the MPD / QoE weights changed) into a
    device blob the controller owns; entries() views it as uint8 [rows, M, Nb, Nq]."""

    method = "fastmpc"
    UTILITIES = BatchedMPCController.UTILITIES

    def __init__(self, player, horizon=5, window=5, utility="identity", clip_horizon=True, buffer_points=None,
                 tput_points=None, buffer_edges=None, tput_edges=None, layout=None, device=None):
        if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= _lib.ROBUST_MAX_WINDOW:
            raise ValueError(f"window must be an integer in 1..{_lib.ROBUST_MAX_WINDOW}")
        if utility not in self.UTILITIES:
            raise ValueError("utility is 'identity' or 'log'")
        if layout not in (None, "uniform", "per_chunk"):
            raise ValueError("layout is 'uniform', 'per_chunk' or None")
        self.player = player
        env = getattr(player, "env", None)
        if device is None:
            device = env.device if env is not None else "cuda"
        self.device = torch.device(device)
        self.window, self.utility = int(window), utility
        self._mpc = BatchedMPCController(player, horizon=horizon, clip_horizon=clip_horizon, device=self.device,
                                         utility=utility)
        self.lib = self._mpc.lib
        self.horizon, self.clip_horizon = self._mpc.horizon, self._mpc.clip_horizon
        self._layout = layout
        mpd = self._mpc.mpd
        br, sz = self._host_tables()
        if buffer_points is None:
            buffer_points = np.linspace(0.0, float(mpd.max_buffer) + float(mpd.chunk_length), DEFAULT_POINTS)
        if tput_points is None:
            tput_points = np.geomspace(float(br.min()) / 4.0, float(br.max()) * 4.0, DEFAULT_POINTS)
        self.buffer_points = np.ascontiguousarray(buffer_points, np.float64).ravel()
        self.tput_points = np.ascontiguousarray(tput_points, np.float64).ravel()
        self.buffer_edges = np.ascontiguousarray(
            arithmetic_edges(self.buffer_points) if buffer_edges is None else buffer_edges, np.float64).ravel()
        self.tput_edges = np.ascontiguousarray(
            geometric_edges(self.tput_points) if tput_edges is None else tput_edges, np.float64).ravel()
        for name, p, e in (("buffer", self.buffer_points, self.buffer_edges),
                           ("throughput", self.tput_points, self.tput_edges)):
            if not 1 <= p.size <= _lib.FASTMPC_MAX_POINTS or e.size != p.size - 1:
                raise ValueError(f"the {name} grid needs 1..{_lib.FASTMPC_MAX_POINTS} points and one edge fewer")
        self._table = None
        self._key = None
        self._fm = None

    # -- tables and layout ---------------------------------------------------
    def _host_tables(self):
        chunks = self._mpc.mpd.chunk_list()
        L = float(self._mpc.mpd.chunk_length)
        br = np.array([[float(b) for b in c.bitrates] for c in chunks], np.float64)
        sz = np.array([[float(s) for s in (c.sizes if c.sizes is not None else [b * L for b in c.bitrates])]
                       for c in chunks], np.float64)
        return br, sz

    @property
    def uniform(self):
        """True when the table has one row per remaining horizon (the uniform layout), False for one row per chunk."""
        cfg = self._mpc.config()
        if self._layout == "per_chunk":
            return False
        br, sz = self._host_tables()
        same = bool((br == br[:1]).all() and (sz == sz[:1]).all())
        fits = cfg.horizon < cfg.video_length
        if self._layout == "uniform":
            if not (same and fits):
                raise ValueError("the uniform layout needs identical bitrates and sizes for every chunk and "
                                 "horizon < video_length")
            return True
        return same and fits

    @property
    def n_rows(self):
        cfg = self._mpc.config()
        return cfg.horizon if self.uniform else cfg.video_length

    def update_mpd(self):
        """Pick up a new MPD from the player (the next build() rebuilds the table)."""
        self._mpc.update_mpd()

    def update_qoe(self):
        """Pick up new QoE weights from the player (the next build() rebuilds the table)."""
        self._mpc.update_qoe()

    def options(self):
        """The abr_fastmpc struct (its host grids point into this controller's arrays)."""
        fm = _lib.FastMpc()
        fm.window, fm.utility, fm.n_rows = self.window, self.UTILITIES[self.utility], self.n_rows
        fm.n_buffer, fm.n_tput = self.buffer_points.size, self.tput_points.size
        fm.buffer_points, fm.buffer_edges = self.buffer_points.ctypes.data, self.buffer_edges.ctypes.data
        fm.tput_points, fm.tput_edges = self.tput_points.ctypes.data, self.tput_edges.ctypes.data
        return fm

    def config(self):
        return self._mpc.config()

    def _build_key(self):
        # the MPD (by identity), the horizon, the clip and the weights; the layout is decided when the table is built
        return self._mpc._bind_key(1)

    # -- the table -------------------------------------------------------------
    def build(self, force=False):
        """Build the table on the device (enqueued on the current stream; nothing synchronises).  Lazy: a no-op while
        the table in hand was built for the current MPD, weights and grid, unless force."""
        br, sz = self._mpc._tables()
        key = self._build_key()
        if self._table is not None and self._key == key and not force:
            return self._table
        cfg, fm = self.config(), self.options()
        nbytes, sbytes = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.abr_fastmpc_table_bytes(C.byref(cfg), C.byref(fm), C.byref(nbytes)), self.lib)
        _lib.check(self.lib.abr_fastmpc_build_scratch_bytes(C.byref(cfg), C.byref(fm), C.byref(sbytes)), self.lib)
        table = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        scratch = torch.empty(sbytes.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.abr_fastmpc_build(C.byref(cfg), C.byref(fm), _lib.ptr(br), _lib.ptr(sz),
                                                  _lib.ptr(table), table.numel(), _lib.ptr(scratch), scratch.numel(),
                                                  _lib.current_stream(self.device)), self.lib)
        self._table, self._key, self._fm = table, key, (cfg, fm)
        return table

    def bound(self):
        """(config, options, blob) for the C ABI, building the table first if needed."""
        table = self.build()
        cfg, fm = self._fm
        return cfg, fm, table

    def entries(self):
        """The table's entries as a uint8 [rows, M, Nb, Nq] view of the blob."""
        cfg, fm, table = self.bound()
        shape = (fm.n_rows, cfg.n_rates, fm.n_buffer, fm.n_tput)
        return table[:int(np.prod(shape))].view(shape)

    # -- decisions -------------------------------------------------------------
    def next_bitrate(self):
        """One decision per lane on the environment's current state (no step): int32 [N], -1 for a lane whose done bits
        are set."""
        env = self.player.env
        cfg, fm, table = self.bound()
        action = torch.empty(env.n_lanes, dtype=torch.int32, device=env.device)
        env._call(env.lib.abr_env_fastmpc_select, env._h, C.byref(cfg), C.byref(fm), _lib.ptr(table),
                  _lib.ptr(action))
        return action

    def select(self, chunk, previous_bitrate, buffer_level, previous_bandwidths, mask=None, mask_is_done=False):
        """The lookup for N independent players: chunk / previous_bitrate int32 [N], buffer_level float64 [N],
        previous_bandwidths float64 [T, N] (T >= every chunk), mask uint8 [N] or None.  Returns int32 [N]."""
        cfg, fm, table = self.bound()
        N = int(chunk.numel())
        for t, dt in ((chunk, torch.int32), (previous_bitrate, torch.int32), (buffer_level, torch.float64)):
            if t.dtype != dt or t.device.type != "cuda" or t.numel() != N:
                raise TypeError(f"select needs {dt} [N] tensors on the GPU")
        hist = previous_bandwidths
        if hist.dtype != torch.float64 or hist.dim() != 2 or hist.shape[1] != N or hist.stride(1) != 1:
            raise TypeError("previous_bandwidths must be float64 [T, N] with unit lane stride")
        if N and int(chunk.max()) > hist.shape[0]:
            raise TypeError("previous_bandwidths has fewer rows than a lane's chunk")
        action = torch.empty(N, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.abr_fastmpc_select(
                C.byref(cfg), C.byref(fm), _lib.ptr(table), table.numel(), _lib.ptr(chunk), _lib.ptr(previous_bitrate),
                _lib.ptr(buffer_level), C.c_void_p(hist.data_ptr()), hist.stride(0), _lib.ptr(mask),
                int(bool(mask_is_done)), _lib.ptr(action), N, _lib.current_stream(self.device)), self.lib)
        return action
