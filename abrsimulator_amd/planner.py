"""Forecast MPC: the deployable baseline that optimises the QoE the project reports.  Per decision a throughput forecast P
per lane -- the harmonic mean of the last `window` downloads, discounted by RobustMPC's largest recent relative error when
`robust` -- and then the lookahead's exhaustive walk of the next `horizon` decisions in a world of constant bandwidth P,
through the step the environment kernels run (live-edge gating, start-up, buffer cap, max_ticks) and with the key the
ledger reports, a quality model's term among them.  The contract is include/abr_env.h (abr_plan_config); the device code is
csrc/abr_lane_jump.h (plan_forecast, look_subtree) and csrc/abr_env.hip (plan_forecast_kernel, plan_kernel).

It follows the player protocol of rules.py (`player.env`, a BatchedABREnv):

    ctl = ForecastMPCController(EnvPlayer(env), horizon=4)           # RobustMPC's forecast, window 5
    sel = ctl.select(want_q=True, want_forecast=True)                # action int32 [N] (-1: none), key, q [M, N], forecast
    env.step(ctl.next_bitrate())                                     # -1 answered as bitrate 0
    out = env.step_plan(ctl, 48)                                     # the fused rollout: forecast, plan, download

`forecast=` (float64 [N] on the env's device) replaces the built-in forecast by the caller's own; no state is touched then.

The robust forecast keeps per-lane state (`state`, uint8, the layout of abr_mpc_robust: int32 [2][N] then float64
[1 + window][N], all-zero = empty).  Like RobustMPC's, it is controller-side state: after env.fork(src, dst) it follows with
`t[:, dst] = t[:, src]` on both tensors of state_rows().
"""
import ctypes as C

import torch

from . import _lib


class ForecastMPCController:
    def __init__(self, player, horizon, window=5, robust=True, max_nodes_per_launch=0):
        if int(horizon) != horizon or not 1 <= int(horizon) <= _lib.MAX_HORIZON:
            raise ValueError(f"horizon must be an integer in 1..{_lib.MAX_HORIZON}, got {horizon}")
        if int(window) != window or not 1 <= int(window) <= _lib.ROBUST_MAX_WINDOW:
            raise ValueError(f"window must be an integer in 1..{_lib.ROBUST_MAX_WINDOW}, got {window}")
        if int(max_nodes_per_launch) != max_nodes_per_launch or int(max_nodes_per_launch) < 0:
            raise ValueError(f"max_nodes_per_launch must be an integer >= 0 (0: the library's default), got "
                             f"{max_nodes_per_launch}")
        self.player = player
        self.horizon, self.window, self.robust = int(horizon), int(window), bool(robust)
        self.max_nodes_per_launch = int(max_nodes_per_launch)
        self._state = None

    @property
    def env(self):
        return self.player.env

    # -- the robust forecast's per-lane state -------------------------------
    @property
    def state(self):
        """The robust state of the environment's lanes (uint8, abr_mpc_robust's layout), allocated all-zero (empty) on
        first use.  robust=False and a caller's forecast neither read nor write it."""
        env = self.env
        if self._state is None or self._state.device != env.device:
            need = C.c_size_t()
            _lib.check(env.lib.abr_mpc_robust_state_bytes(self.window, env.n_lanes, C.byref(need)), env.lib)
            self._state = torch.zeros(need.value, dtype=torch.uint8, device=env.device)
        return self._state

    def state_rows(self):
        """Zero-copy views of `state` with the lanes as columns: (int32 [2, N]: c* + 1 and the error count, float64
        [1 + window, N]: p* and the errors).  After env.fork(src, dst): t[:, dst] = t[:, src] on both."""
        N = self.env.n_lanes
        st = self.state
        return st[:8 * N].view(torch.int32).view(2, N), st[8 * N:].view(torch.float64).view(1 + self.window, N)

    def reset_state(self):
        """Forget every lane's past estimates and errors."""
        if self._state is not None:
            self._state.zero_()

    def config(self, forecast=None):
        """The abr_plan_config for the environment's lanes; `forecast`: the caller's float64 [N] device tensor or None."""
        env = self.env
        cfg = _lib.PlanConfig(self.horizon, self.window, int(self.robust), 0, self.max_nodes_per_launch, None, None, 0)
        if forecast is not None:
            if not torch.is_tensor(forecast) or forecast.dtype != torch.float64:
                raise ValueError("forecast must be a float64 tensor")
            if tuple(forecast.shape) != (env.n_lanes,):
                raise ValueError(f"forecast must have shape ({env.n_lanes},), got {tuple(forecast.shape)}")
            if forecast.device != env.device or not forecast.is_contiguous():
                raise ValueError(f"forecast must be a contiguous tensor on {env.device}, got one on {forecast.device}")
            cfg.forecast_dev = forecast.data_ptr()
        elif self.robust:
            st = self.state
            cfg.state_dev, cfg.state_bytes = st.data_ptr(), st.numel()
        return cfg

    def select(self, want_key=True, want_q=False, want_forecast=False, forecast=None):
        """One decision per lane on the environment's current state (no step, nothing synchronises): a dict with `action`
        int32 [N] (-1 for a lane that is finished, has no forecast -- chunk 0, or a forecast that is not finite or not > 0
        -- or has no sequence without a time-out), `key` float64 [N] (NaN with action -1), `q` float64 [M, N], the least
        cost per first bitrate, and `forecast` float64 [N], the P the walk used (0.0 where there was none).  Entries that
        are not wanted are None.  Writes nothing but the robust state; selecting twice gives the same answer and state.
        The library's refusals (a tree of more than 65 536 leaves, speed features) raise AbrError."""
        env = self.env
        cfg = self.config(forecast)
        action = torch.empty(env.n_lanes, dtype=torch.int32, device=env.device)
        key = torch.empty(env.n_lanes, dtype=torch.float64, device=env.device) if want_key else None
        q = torch.empty(env.n_rates, env.n_lanes, dtype=torch.float64, device=env.device) if want_q else None
        # the built-in forecast needs its n_lanes doubles somewhere outside the workspace: always ours
        P = torch.empty(env.n_lanes, dtype=torch.float64, device=env.device) if want_forecast or forecast is None else None
        env._call(env.lib.abr_env_plan_select, env._h, C.byref(cfg), _lib.ptr(action), _lib.ptr(key), _lib.ptr(q), _lib.ptr(P))
        return dict(action=action, key=key, q=q, forecast=P if want_forecast else None)

    def next_bitrate(self, forecast=None):
        """The actions alone, int32 [N], with "no decision" (-1) answered as bitrate 0: what env.step takes."""
        return self.select(want_key=False, forecast=forecast)["action"].clamp_(min=0)
