"""The standard ABR baselines next to the MPC: buffer-based (BBA-0, Huang et al. 2014), rate-based (harmonic mean of the
recent throughput) and BOLA-BASIC (Spiteri et al. 2016), each a get_next_bitrate (Simulator.py:155) evaluated on the
device on every lane's exact float64 state.  The decision rules and their operation order are the contract of
include/abr_env.h (abr_rule_config); the device code is csrc/abr_lane_jump.h: rule_select.

Each controller follows the player protocol BatchedMPCController uses (mpc.py: EnvPlayer): `player.get_mpd()` for the
parameters, `player.env` (a BatchedABREnv) for next_bitrate().  Two ways to drive an environment with one:

    ctl = RateBasedController(EnvPlayer(env), window=5)
    out = env.step_rule(ctl, 48)            # 48 fused decisions per lane, no host work between them
    a = ctl.next_bitrate()                  # or one decision per lane on the current state, then env.step(a)
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


class _RuleController:
    KIND = 0

    def __init__(self, player):
        self.player = player
        self.mpd = player.get_mpd()
        self._cfg = None

    @property
    def env(self):
        return self.player.env

    def _fill(self, cfg):
        pass

    def config(self):
        """The abr_rule_config this controller hands to abr_env_step_rule / abr_env_rule_select (built once)."""
        if self._cfg is None:
            c = _lib.RuleConfig()
            c.kind = self.KIND
            self._fill(c)
            self._cfg = c
        return self._cfg

    def next_bitrate(self):
        """One decision per lane on the environment's current state (no step): int32 [N], -1 for a lane whose done bits
        are set."""
        env = self.env
        action = torch.empty(env.n_lanes, dtype=torch.int32, device=env.device)
        env._call(env.lib.abr_env_rule_select, env._h, C.byref(self.config()), _lib.ptr(action))
        return action


class BufferBasedController(_RuleController):
    """BBA-0 rate map without hysteresis: bitrate 0 up to `reservoir` seconds of buffer, the top bitrate from
    reservoir + `cushion` on, a linear map of the buffer onto [br[0], br[M-1]] in between (rounded down to a ladder rate).
    Defaults: reservoir = 0.25 * max_buffer, cushion = 0.5 * max_buffer."""
    KIND = _lib.RULE_BUFFER

    def __init__(self, player, reservoir=None, cushion=None):
        super().__init__(player)
        mb = float(self.mpd.max_buffer)
        self.reservoir = 0.25 * mb if reservoir is None else float(reservoir)
        self.cushion = 0.5 * mb if cushion is None else float(cushion)
        if not (math.isfinite(self.reservoir) and self.reservoir >= 0.0):
            raise ValueError(f"reservoir must be finite and >= 0, got {self.reservoir}")
        if not (math.isfinite(self.cushion) and self.cushion > 0.0):
            raise ValueError(f"cushion must be finite and > 0, got {self.cushion}")

    def _fill(self, c):
        c.reservoir, c.cushion = self.reservoir, self.cushion


class RateBasedController(_RuleController):
    """The highest ladder rate not above safety * the harmonic mean of the last `window` chunk throughputs (bitrate 0
    before the first chunk)."""
    KIND = _lib.RULE_RATE

    def __init__(self, player, window=5, safety=1.0):
        super().__init__(player)
        if int(window) != window or int(window) < 1:
            raise ValueError(f"window must be an integer >= 1, got {window}")
        self.window, self.safety = int(window), float(safety)
        if not (math.isfinite(self.safety) and self.safety > 0.0):
            raise ValueError(f"safety must be finite and > 0, got {safety}")

    def _fill(self, c):
        c.window, c.safety = self.window, self.safety


class BolaController(_RuleController):
    """BOLA-BASIC: the first bitrate maximising (v * (u[c][m] + gamma_p) - buffer_level) / br[c][m], with the utility
    u[c][m] = ln(br[c][m] / br[c][0]) computed here in float64 from the environment's bitrate table.  Default
    v = (max_buffer - chunk_length) / (ln(ladder[-1] / ladder[0]) + gamma_p), which needs max_buffer > chunk_length."""
    KIND = _lib.RULE_BOLA

    def __init__(self, player, gamma_p=5.0, v=None):
        super().__init__(player)
        self.gamma_p = float(gamma_p)
        table = np.asarray(self.mpd.bitrate_table(), np.float64)
        if table.ndim != 2 or not bool((table > 0).all()):
            raise ValueError("BOLA needs a [video_length][n_rates] table of bitrates > 0")
        if v is None:
            L, mb = float(self.mpd.chunk_length), float(self.mpd.max_buffer)
            if mb <= L:
                raise ValueError(f"the default BOLA v needs max_buffer > chunk_length (got {mb} <= {L}); pass v")
            v = (mb - L) / (math.log(table[0, -1] / table[0, 0]) + self.gamma_p)
        self.v = float(v)
        if not (math.isfinite(self.v) and self.v > 0.0) or not math.isfinite(self.gamma_p):
            raise ValueError(f"v must be finite and > 0 and gamma_p finite, got v={v}, gamma_p={gamma_p}")
        self.utility = np.log(table / table[:, :1])       # float64 [video_length][n_rates], on the host
        self._utility_dev = None

    def _fill(self, c):
        if self._utility_dev is None:
            self._utility_dev = torch.from_numpy(np.ascontiguousarray(self.utility)).to(self.env.device)
        c.bola_v, c.bola_gp = self.v, self.gamma_p
        c.utility_dev = self._utility_dev.data_ptr()
