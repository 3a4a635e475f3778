"""Twin of the closed-loop speed rule (include/abr_env.h: abr_speed_rule) -- TEST INFRASTRUCTURE.

Two pieces:
- `rule_np`: the rule itself in numpy (comparisons and a table read), for seeded fuzzing against the host build.
- `RuleTickEnv`: the reference's tick loop (oracle/pyloop.py, pinned to the reference goldens) with the rule evaluated
  where Simulator.py:176-177 calls get_next_speed(): at the first playing tick of every played chunk, from
  lat = global_time - play_time (:179, before this tick's += speed*dt) and the buffer level at that point of the tick
  (after :170, before :184).  It logs every answer, so that the answers can be replayed through the C oracle as a
  speed schedule (oracle.env_batch(speeds=log)).
"""
import numpy as np

from oracle.pyloop import PyTickEnv


def rule_arrays(ctl):
    """(lat_thr, buf_thr, speeds [n_lat+1, n_buf+1]) of a LatencySpeedController."""
    return (np.asarray(ctl.latency_thresholds, np.float64), np.asarray(ctl.buffer_thresholds, np.float64),
            np.asarray(ctl.speeds, np.float64))


def rule_np(lat_thr, buf_thr, speeds, lat, buf):
    """speeds[i, j] with i = #{q: lat >= lat_thr[q]}, j = #{r: buf >= buf_thr[r]}, elementwise over lat / buf."""
    lat = np.asarray(lat, np.float64)
    buf = np.asarray(buf, np.float64)
    i = (lat[..., None] >= np.asarray(lat_thr, np.float64)).sum(-1)
    j = (buf[..., None] >= np.asarray(buf_thr, np.float64)).sum(-1)
    return np.asarray(speeds, np.float64)[i, j]


class RuleTickEnv(PyTickEnv):
    """One lane of the tick loop whose play speed is the rule's answer; `log` lists the answers of this episode."""

    def __init__(self, *args, rule, **kw):
        self.rule = rule                     # (lat_thr, buf_thr, speeds)
        self.log = []
        self._sp = 1.0
        super().__init__(*args, **kw)

    @property
    def speed(self):
        # read once per playing tick (PyTickEnv._tail); play_len == 0 is the reference's `play_length == 0`
        if self.play_len == 0:
            lat = self.t - self.play_time
            self._sp = float(rule_np(*self.rule, lat, self.buf))
            self.log.append(self._sp)
        return self._sp

    @speed.setter
    def speed(self, _):
        pass                                 # the constructor's constant speed: the rule replaces it

    def reset(self):
        self.log = []
        return super().reset()


STEP_KEYS = ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "average_latency",
             "play_id", "last_bandwidth")
FINAL_KEYS = ("global_time", "rebuffer_time", "start_up_time", "play_time", "buffer_level", "average_latency",
              "play_id", "qoe")


def twin_batch(meta, traces, trace_id, offset, actions, rule, log_rows):
    """Episodes of N lanes.  Returns (steps {key: [N, V]} at each call site, final {key: [N]},
    bandwidths [N, V], log [N, log_rows] (NaN past the last answer), n_answers [N])."""
    actions = np.asarray(actions, np.int32)
    N, V = actions.shape
    steps = {k: np.zeros((N, V)) for k in STEP_KEYS}
    final = {k: np.zeros(N) for k in FINAL_KEYS}
    bws = np.zeros((N, V))
    log = np.full((N, log_rows), np.nan)
    n_ans = np.zeros(N, np.int64)
    for i in range(N):
        env = RuleTickEnv(meta["ladder"], meta["chunk_length"], V, meta["max_buffer"], meta["start_up_length"],
                          meta["interval"], meta["weights"], list(traces[trace_id[i]]), int(offset[i]), rule=rule)
        obs = [env.reset()]
        for s in range(V):
            o, done = env.step(int(actions[i, s]))
            if not done:
                obs.append(o)
        for s, o in enumerate(obs):
            for k in STEP_KEYS:
                steps[k][i, s] = o[k]
        fo = env._obs()
        for k in FINAL_KEYS[:-1]:
            final[k][i] = fo[k]
        final["qoe"][i] = env.qoe()
        bws[i] = env.hist_bw
        n = min(len(env.log), log_rows)
        log[i, :n] = env.log[:n]
        n_ans[i] = len(env.log)
    return steps, final, bws, log, n_ans
