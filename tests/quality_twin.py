"""A numpy twin of the quality model's contract (include/abr_env.h: abr_episode_quality), written from the header's text
and independent of abrsimulator_amd/quality.py and of csrc/abr_lane_jump.h: the layout arithmetic, the per-step rule, the
per-episode rule and the reset; and a driver that replays a launch's (actions, done) slabs through them."""
import numpy as np

DONE_EPISODE, DONE_TIMEOUT, DONE_BADACT = 1, 2, 4


def up256(b):
    return -(-int(b) // 256) * 256


def layout(n_lanes, rows):
    """Byte offsets (count, q_run, q_last, total_q, rec_q) and the size of the blob."""
    o_run = up256(4 * n_lanes)
    o_last = o_run + up256(8 * n_lanes)
    o_tot = o_last + up256(8 * n_lanes)
    o_rec = o_tot + up256(8 * n_lanes)
    return 0, o_run, o_last, o_tot, o_rec, o_rec + up256(rows * 8 * n_lanes)


class TwinQuality:
    def __init__(self, n_lanes, rows, wq, u):
        self.n, self.rows = int(n_lanes), int(rows)
        self.wq = np.float64(wq)
        self.u = np.asarray(u, np.float64)
        self.o = layout(self.n, self.rows)
        self.blob = np.zeros(self.o[5], np.uint8)
        n, r = self.n, self.rows
        self.count = self.blob[0:4 * n].view(np.int32)
        self.q_run = self.blob[self.o[1]:self.o[1] + 8 * n].view(np.float64)
        self.q_last = self.blob[self.o[2]:self.o[2] + 8 * n].view(np.float64)
        self.total_q = self.blob[self.o[3]:self.o[3] + 8 * n].view(np.float64)
        self.rec_q = self.blob[self.o[4]:self.o[4] + 8 * n * r].view(np.float64).reshape(r, n)

    def step(self, lane, chunk, action, rew):
        """A step of `lane` that completed the download of `chunk` at rate `action`; rew: the float64 reward without a
        model.  Returns the float64 reward with it (the kernels round that to float32)."""
        q = self.u[chunk, action]
        self.q_run[lane] = self.q_run[lane] + q
        with np.errstate(invalid="ignore", over="ignore"):
            return np.float64(rew) - self.wq * q

    def close(self, lane, rearm):
        """The episode of `lane` has ended (ABR_DONE_EPISODE or ABR_DONE_TIMEOUT); rearm: auto_reset and ABR_DONE_EPISODE."""
        Q = self.q_run[lane]
        self.q_last[lane] = Q
        self.rec_q[int(self.count[lane]) % self.rows, lane] = Q
        self.total_q[lane] = self.total_q[lane] + Q
        self.count[lane] += 1
        if rearm:
            self.q_run[lane] = 0.0

    def reset(self, mask=None):
        if mask is None:
            self.q_run[:] = 0.0
        else:
            self.q_run[np.asarray(mask).astype(bool)] = 0.0

    def launch(self, chunk0, actions, done, auto_reset, rew64=None, frozen=None):
        """Replay one launch.  chunk0 [n]: each lane's chunk id at its first call site of the launch; actions, done
        [n_steps, n] as the launch reported them (done: the ABR_DONE_* byte each step left); frozen [n] bool: lanes that
        were done before the launch.  rew64 [n_steps, n] (optional): the float64 rewards without a model.  A step
        completed its download unless it reports ABR_DONE_BADACT, or ABR_DONE_TIMEOUT alone (the contract: a time-out
        in mid-download).  Returns (the float64 rewards with the model, or None; hit [n_steps, n] bool; the chunk id
        [n_steps, n] each step downloaded; each lane's chunk id after the launch; the lanes frozen after it)."""
        actions, done = np.asarray(actions), np.asarray(done)
        T, n = actions.shape
        V = self.u.shape[0]
        chunk = np.array(chunk0, np.int64)
        live = np.ones(n, bool) if frozen is None else ~np.asarray(frozen, bool)
        out = None if rew64 is None else np.array(rew64, np.float64)
        hit, cs = np.zeros((T, n), bool), np.zeros((T, n), np.int64)
        for t in range(T):
            for i in range(n):
                if not live[i]:
                    continue
                d = int(done[t, i])
                cs[t, i] = chunk[i]
                if d & DONE_BADACT:
                    live[i] = False
                    continue
                h = not (d & DONE_TIMEOUT) or bool(d & DONE_EPISODE)
                if h:
                    hit[t, i] = True
                    r = self.step(i, int(chunk[i]), int(actions[t, i]), 0.0 if out is None else out[t, i])
                    if out is not None:
                        out[t, i] = r
                    chunk[i] += 1
                ended = chunk[i] >= V and h
                if ended or (d & DONE_TIMEOUT):
                    rearm = bool(auto_reset) and ended
                    self.close(i, rearm)
                    if rearm:
                        chunk[i] = 0
                    else:
                        live[i] = False
        return out, hit, cs, chunk, ~live
