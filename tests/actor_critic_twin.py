"""numpy twin of the actor-critic additions (include/abr_env.h: abr_policy_value, abr_gae): the value head as one more
k-ordered fmaf chain over the last hidden layer's output (tests/policy_twin.py's exact fmaf), and the GAE recurrence in
float32 with one rounding per operation, vectorised over lanes.  edge_slabs() builds the slabs both the CPU and the GPU
tests run the recurrence on."""
import numpy as np

import policy_twin as T

f32 = np.float32


def hidden(layers, x):
    """The value head's input y [in, N]: the last hidden layer's post-ReLU output, x itself without a hidden layer."""
    h = np.asarray(x, np.float32)
    for W, b in layers[:-1]:
        h = T.relu(T.layer(W, b, h))
    return h


def value(layers, head, x):
    """v [N] = bv, then fmaf(Wv[k], y[k], v) for k in order.  head = (Wv [in], bv)."""
    Wv, bv = head
    return T.layer(np.asarray(Wv, np.float32).reshape(1, -1), np.asarray(bv, np.float32).reshape(1), hidden(layers, x))[0]


def gae(reward, values, last_value, done, actions=None, gamma=0.99, lam=0.95):
    """(adv, ret) float32 [T, N] by the contract's recurrence, every operation one float32 rounding."""
    r, v = np.asarray(reward, np.float32), np.asarray(values, np.float32)
    T_, N = r.shape
    gamma, lam = f32(gamma), f32(lam)
    gl = f32(gamma * lam)
    A = np.zeros(N, np.float32)
    nv = np.asarray(last_value, np.float32).copy()
    adv, ret = np.empty((T_, N), np.float32), np.empty((T_, N), np.float32)
    zero = np.zeros(N, np.float32)
    with np.errstate(all="ignore"):
        for t in range(T_ - 1, -1, -1):
            term = np.asarray(done[t]) != 0
            dead = np.asarray(actions[t]) < 0 if actions is not None else np.zeros(N, bool)
            q = np.where(term, zero, gamma * nv)
            delta = (r[t] + q) - v[t]
            w = np.where(term, zero, gl * A)
            A = np.where(dead, zero, delta + w)
            adv[t] = A
            ret[t] = np.where(dead, zero, A + v[t])
            nv = np.where(dead, zero, v[t])
    return adv, ret


def edge_slabs(T_, N, seed):
    """Seeded slabs [T_, N] whose lanes cycle through the recurrence's edge cases: an episode end at t = 0, at t = T_ - 1,
    on consecutive steps, on every step; lanes dead throughout; dead tails (with and without a done byte in front, as a
    rollout without auto_reset leaves them); every done bit; infinite and NaN values, rewards and last values BEHIND an
    episode end or a dead step (they may not leak across it); plain random lanes.  Returns dict(reward, values,
    last_value, done, actions, poison) -- poison [T_, N] marks the planted non-finite entries and poison_last [N]."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(-1.0, 2.0, (T_, N)).astype(np.float32)
    values = rng.normal(-5.0, 3.0, (T_, N)).astype(np.float32)
    last = rng.normal(-5.0, 3.0, N).astype(np.float32)
    done = np.zeros((T_, N), np.uint8)
    actions = rng.integers(0, 6, (T_, N)).astype(np.int32)
    poison = np.zeros((T_, N), bool)
    poison_last = np.zeros(N, bool)
    bad = np.array([np.inf, -np.inf, np.nan], np.float32)
    for i in range(N):
        kind = i % 12
        if kind == 0:
            done[0, i] = 1
        elif kind == 1:
            done[T_ - 1, i] = 1
            last[i] = bad[i // 12 % 3]                                     # behind the end: never read into a sum
            poison_last[i] = True
        elif kind == 2 and T_ >= 2:
            t = int(rng.integers(0, T_ - 1))
            done[t, i] = done[t + 1, i] = 1
        elif kind == 3:
            done[:, i] = 1
        elif kind == 4:
            actions[:, i] = -1
            values[:, i] = 0.0
            reward[:, i] = 0.0
        elif kind == 5:                                                   # a dead tail behind a done byte
            t = int(rng.integers(0, T_))
            done[t, i] = int(rng.choice([1, 2, 4, 8, 3]))
            actions[t + 1:, i] = -1
            done[t + 1:, i] = done[t, i]
            values[t + 1:, i] = bad[i // 12 % 3]                          # garbage on dead rows is never read into a sum
            poison[t + 1:, i] = True
        elif kind == 6 and T_ >= 2:                                       # a non-finite value right behind an episode end
            t = int(rng.integers(0, T_ - 1))
            done[t, i] = 1
            values[t + 1, i] = bad[i // 12 % 3]
            poison[t + 1, i] = True
        elif kind == 7 and T_ >= 2:                                       # a non-finite reward behind an end
            t = int(rng.integers(0, T_ - 1))
            done[t, i] = 2
            reward[t + 1, i] = bad[i // 12 % 3]
            poison[t + 1, i] = True
        elif kind == 8:                                                   # a dead tail with no done byte in front
            t = int(rng.integers(0, T_))
            actions[t:, i] = -1
            last[i] = bad[i // 12 % 3]
            poison_last[i] = True
        elif kind == 9:                                                   # random ends, every done bit
            done[:, i] = np.where(rng.random(T_) < 0.3, rng.choice([1, 2, 4, 8, 16, 255], T_), 0)
        # kinds 10, 11: no end at all
    return dict(reward=reward, values=values, last_value=last, done=done, actions=actions, poison=poison,
                poison_last=poison_last)


def episode_sums(reward, done, actions=None):
    """float64 [T, N]: the sum of the rewards from t to the end of t's episode (the end of the slab for an episode still
    running), and int [T, N]: the number of steps in that sum.  Dead steps hold 0 and cut the sum like an end."""
    r = np.asarray(reward, np.float64)
    T_, N = r.shape
    s, k = np.zeros((T_, N)), np.zeros((T_, N), np.int64)
    absum = np.zeros((T_, N))
    run, cnt, ab = np.zeros(N), np.zeros(N, np.int64), np.zeros(N)
    for t in range(T_ - 1, -1, -1):
        term = np.asarray(done[t]) != 0
        dead = np.asarray(actions[t]) < 0 if actions is not None else np.zeros(N, bool)
        run = np.where(dead, 0.0, r[t] + np.where(term, 0.0, run))
        ab = np.where(dead, 0.0, np.abs(r[t]) + np.where(term, 0.0, ab))
        cnt = np.where(dead, 0, 1 + np.where(term, 0, cnt))
        s[t], k[t], absum[t] = run, cnt, ab
    return s, k, absum
