"""Hindsight beam search through the real kernels: the best bitrate sequence of a trace whose future is known.

Every ABR evaluation reports such a bound (Pensieve's "offline optimal", Comyco's expert).  The simulator's dynamics are
exact, live-gated and tick-quantised, so the bound is searched through the environment itself: each group of
beam * n_rates lanes carries `beam` survivors of one (trace, start offset), every survivor tries every rate in one step(),
abr_beam_select ranks the candidates on the device and env.fork() moves the winners into place.  The prefix score adds the
latency term the step reward leaves out, wl * average_latency: it dominates the final QoE, and pruning on the reward sum
alone is worse than greedy.  With beam >= n_rates ** (video_length - 1) nothing is pruned and the result is the optimum.
"""
import torch

from . import _lib


def beam_select(lib, n_groups, beam, n_rates, wl, R, reward, lat, done, valid, key_override, src_out, R_out, valid_out,
                stream):
    """abr_beam_select on tensors (include/abr_env.h); every tensor holds at least n_groups * beam * n_rates elements."""
    _lib.check(lib.abr_beam_select(int(n_groups), int(beam), int(n_rates), float(wl), _lib.ptr(R), _lib.ptr(reward),
                                   _lib.ptr(lat), _lib.ptr(done), _lib.ptr(valid), _lib.ptr(key_override),
                                   _lib.ptr(src_out), _lib.ptr(R_out), _lib.ptr(valid_out), stream), lib)


class HindsightSearch:
    """Beam search of width `beam` for the episode of least QoE cost on given (trace, start offset) pairs.

    env: a BatchedABREnv built with auto_reset=False and n_lanes >= groups * beam * n_rates.  Lanes are grouped as
    slots = beam * n_rates consecutive lanes per group (slots <= 1024); slot r * n_rates + m is "survivor r takes rate m".
    run(trace_id, start_offset), one pair per group, returns dict(qoe f64 [groups], actions int32 [V, groups], lane
    int32 [groups], valid uint8 [groups]): the best episode found, its bitrate sequence (the winner's action history:
    fork carries each lane's history, so there are no back-pointers), the lane that holds it and whether the group found
    any finished episode.  qoe is episode_qoe(quality=True) with a quality model installed, else episode_qoe().
    begin() / step() / finish() are run()'s pieces; step() returns that iteration's (src, R, valid).  Nothing
    synchronises before the results are read.  Out of scope: ShardedABREnv, auto_reset=True, merging duplicate states."""

    def __init__(self, env, beam):
        if env.cfg.auto_reset:
            raise ValueError("HindsightSearch needs an env built with auto_reset=False")
        self.env, self.beam = env, int(beam)
        self.n_rates, self.V = env.n_rates, env.video_length
        self.slots = self.beam * self.n_rates
        if self.beam < 1 or self.slots > 1024:
            raise ValueError(f"beam * n_rates must be in 1..1024, got {self.beam} * {self.n_rates}")
        if env.n_lanes < self.slots:
            raise ValueError(f"the env has {env.n_lanes} lanes, one group needs {self.slots}")
        N, dev = env.n_lanes, env.device
        lane = torch.arange(N, device=dev)
        self.actions = (lane % self.slots % self.n_rates).to(torch.int32)       # the rate slot s tries: s % n_rates
        self._valid0 = ((lane % self.slots) < self.n_rates).to(torch.uint8)     # all slots start equal: keep one survivor
        self.wl = float(env.cfg.latency_weight)
        self.groups = 0
        self.t = 0

    def begin(self, trace_id, start_offset):
        env, S = self.env, self.slots
        tid = torch.as_tensor(trace_id, device=env.device).to(torch.int32).reshape(-1)
        off = torch.as_tensor(start_offset, device=env.device).to(torch.int32).reshape(-1)
        G = int(tid.numel())
        if G < 1 or off.numel() != G:
            raise ValueError("trace_id and start_offset hold one pair per group")
        if G * S > env.n_lanes:
            raise ValueError(f"{G} groups of {S} slots need {G * S} lanes, the env has {env.n_lanes}")
        N, dev = env.n_lanes, env.device
        g = (torch.arange(N, device=dev) // S).clamp(max=G - 1)                 # lanes past the last group: its pair, unused
        env.reset(tid[g].contiguous(), off[g].contiguous())
        self.groups, self.t = G, 0
        self.R = torch.zeros(N, dtype=torch.float64, device=dev)
        self.valid = self._valid0.clone()
        self.valid[G * S:] = 0
        # outputs of a select; lanes past the last group keep src -1 (fork leaves them alone)
        self._src = torch.full((N,), -1, dtype=torch.int32, device=dev)
        self._R_out = torch.zeros(N, dtype=torch.float64, device=dev)
        self._valid_out = torch.zeros(N, dtype=torch.uint8, device=dev)

    def _select(self, reward, lat, done, key_override=None):
        env = self.env
        with torch.cuda.device(env.device):
            beam_select(env.lib, self.groups, self.beam, self.n_rates, self.wl, self.R, reward, lat, done, self.valid,
                        key_override, self._src, self._R_out, self._valid_out, env._stream())
        return self._src, self._R_out, self._valid_out

    def step(self, record=True):
        """One iteration: every survivor tries every rate, the candidates are ranked, and -- on all steps but the last --
        the winners are forked into place.  Returns (src int32 [N], R f64 [N], valid u8 [N], reward f32 [N], lat f64 [N],
        done u8 [N]): the select's outputs and the inputs it read (fresh tensors; None with record=False)."""
        if self.t >= self.V:
            raise RuntimeError("the search has taken its video_length steps: finish()")
        env = self.env
        _, reward, done = env.step(self.actions)
        lat = env.observe_f64()["average_latency"]
        src, R, valid = self._select(reward, lat, done)
        out = (src.clone(), R.clone(), valid.clone(), reward.clone(), lat.clone(), done.clone()) if record else None
        self.t += 1
        if self.t < self.V:
            env.fork(src, update_pairs=False)       # a survivor stays in its group, and a group runs one pair
            self.R, self._R_out = self._R_out, self.R
            self.valid, self._valid_out = self._valid_out, self.valid
        else:
            self._last = (reward.clone(), done.clone())     # the candidates stay where they are for the final ranking
        return out

    def finish(self):
        """The final ranking, on the episode's own QoE: rank 0 of every group."""
        if self.t != self.V:
            raise RuntimeError("finish() comes after video_length steps")
        env, S, G = self.env, self.slots, self.groups
        qoe = env.episode_qoe(quality=env.quality is not None)
        reward, done = self._last
        src, _, valid = self._select(reward, None, done, key_override=qoe)
        first = torch.arange(G, device=env.device) * S
        lane, ok = src[first], valid[first].clone()
        at = lane.clamp(min=0).long()
        hist = env.history()[0]
        nan = torch.full((G,), float("nan"), dtype=torch.float64, device=env.device)
        return dict(qoe=torch.where(ok.bool(), qoe[at], nan), actions=hist[:, at].to(torch.int32),
                    lane=lane.clone(), valid=ok)

    def run(self, trace_id, start_offset):
        self.begin(trace_id, start_offset)
        for _ in range(self.V):
            self.step(record=False)
        return self.finish()
