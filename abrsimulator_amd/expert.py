"""The lookahead expert: for the state each lane is in right now, the best next bitrate given the trace's real future --
the teacher an imitation learner (Comyco's expert, DAgger) asks at every state its own policy reaches.  One launch walks
the exact tree of the next `horizon` decisions of every lane in registers and writes nothing back; the tree, the key and
the tie rules are the contract of include/abr_env.h (abr_env_lookahead_select), the device code is csrc/abr_lane_jump.h
(look_subtree) and csrc/abr_env.hip (lookahead_kernel).  The key is the sum of the step rewards the environment reports
(a quality model's term among them) plus the latency term, so the teacher optimises the metric the project reports.

It follows the player protocol of rules.py (`player.env`, a BatchedABREnv):

    exp = LookaheadExpert(EnvPlayer(env), horizon=4)
    lab = exp.labels(want_q=True)       # action int32 [N] (-1: no label), key float64 [N], q float64 [M, N]
    a = exp.next_bitrate()              # the actions alone
"""
import ctypes as C

import torch

from . import _lib


class LookaheadExpert:
    def __init__(self, player, horizon, max_nodes_per_launch=0):
        if int(horizon) != horizon or not 1 <= int(horizon) <= _lib.MAX_HORIZON:
            raise ValueError(f"horizon must be an integer in 1..{_lib.MAX_HORIZON}, got {horizon}")
        if int(max_nodes_per_launch) != max_nodes_per_launch or int(max_nodes_per_launch) < 0:
            raise ValueError(f"max_nodes_per_launch must be an integer >= 0 (0: the library's default), got "
                             f"{max_nodes_per_launch}")
        self.player = player
        self.horizon, self.max_nodes_per_launch = int(horizon), int(max_nodes_per_launch)
        self._cfg = _lib.LookaheadConfig(self.horizon, 0, self.max_nodes_per_launch)

    @property
    def env(self):
        return self.player.env

    def labels(self, want_key=True, want_q=False):
        """One exact decision per lane on the environment's current state (no step, nothing synchronises): a dict with
        `action` int32 [N] (-1 for a lane whose done bits are set or that has no sequence without a time-out), `key`
        float64 [N], the least cost over the lane's tree (NaN with action -1), and `q` float64 [M, N], the least cost per
        first bitrate (NaN where there is none).  Entries that are not wanted are None.  The library's refusals (a tree
        of more than 65 536 leaves, speed features) raise AbrError."""
        env = self.env
        action = torch.empty(env.n_lanes, dtype=torch.int32, device=env.device)
        key = torch.empty(env.n_lanes, dtype=torch.float64, device=env.device) if want_key else None
        q = torch.empty(env.n_rates, env.n_lanes, dtype=torch.float64, device=env.device) if want_q else None
        env._call(env.lib.abr_env_lookahead_select, env._h, C.byref(self._cfg), _lib.ptr(action), _lib.ptr(key), _lib.ptr(q))
        return dict(action=action, key=key, q=q)

    def next_bitrate(self):
        """The actions alone: int32 [N]."""
        return self.labels(want_key=False)["action"]
