"""numpy twin of the recurrent policy, written from the text of include/abr_env.h: abr_policy_gru (not from the C++):
sig_c, tanh_c, the cell, the outputs, and a per-lane sequential runner that applies the c == 0 rule.  Every operation is
float32 with one rounding; policy_twin.fmaf is the fmaf, policy_sample_twin.exp_c the exponential."""
import numpy as np

import policy_sample_twin as ST
import policy_twin as T

f32 = np.float32
ONE, TWO = f32(1.0), f32(2.0)


def sig_c(v):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        e = ST.exp_c(-np.abs(v))
        q = (ONE + e).astype(f32)
        out = (np.where(v >= 0, ONE, e).astype(f32) / q).astype(f32)
    return np.where(np.isnan(v), v, out).astype(f32)


def tanh_c(v):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        e = ST.exp_c((-TWO * np.abs(v)).astype(f32))
        t = ((ONE - e).astype(f32) / (ONE + e).astype(f32)).astype(f32)
        out = np.copysign(t, v).astype(f32)
    return np.where(np.isnan(v), v, out).astype(f32)


def split_blob(blob, F, H, M):
    """(W_ih [3H, F], W_hh [3H, H], b_ih [3H], b_hh [3H], W_out [M, H], b_out [M]) views of the unpadded blob."""
    blob = np.asarray(blob, f32)
    sizes = [(3 * H, F), (3 * H, H), (3 * H,), (3 * H,), (M, H), (M,)]
    out, o = [], 0
    for sh in sizes:
        n = int(np.prod(sh))
        out.append(blob[o:o + n].reshape(sh))
        o += n
    assert o == blob.size, (o, blob.size)
    return out


def cell(parts, x, h):
    """h' [H, N] of features x [F, N] and h_in h [H, N]: six k-ordered chains per unit, gates r, z, n."""
    W_ih, W_hh, b_ih, b_hh = parts[:4]
    gi = T.layer(W_ih, b_ih, np.asarray(x, f32))
    gh = T.layer(W_hh, b_hh, np.asarray(h, f32))
    H = W_hh.shape[1]
    with np.errstate(all="ignore"):
        r = sig_c((gi[:H] + gh[:H]).astype(f32))
        z = sig_c((gi[H:2 * H] + gh[H:2 * H]).astype(f32))
        n = tanh_c(T.fmaf(r, gh[2 * H:], gi[2 * H:]))
        d = (np.asarray(h, f32) - n).astype(f32)
        return T.fmaf(z, d, n)


def forward(parts, x, h, head=None):
    """(scores [M, N], h' [H, N], value [N] or None)."""
    hp = cell(parts, x, h)
    s = T.layer(parts[4], parts[5], hp)
    v = None
    if head is not None:
        head = np.asarray(head, f32)
        v = T.layer(head[None, :-1], head[-1:], hp)[0]
    return s, hp, v


def h_in(state, c):
    """The state entering a decision: +0 in every unit where c == 0, else the lane's column.  state [H, N], c [N]."""
    return np.where(np.asarray(c)[None, :] == 0, f32(0.0), np.asarray(state, f32)).astype(f32)


def decide(parts, x, h, seed, thr, lane, c, episode, M, mode=ST.ARGMAX, iT=1.0, head=None):
    """dict(actions, scores, probs, value, hp) of one decision on live lanes (x [F, N], h [H, N] already h_in)."""
    s, hp, v = forward(parts, x, h, head)
    g = T.argmax_first(s)
    if mode == ST.ARGMAX:
        probs = (np.arange(M)[:, None] == g[None, :]).astype(f32)
        a, _ = T.explore(seed, thr, lane, c, episode, M, g)
    else:
        _, _, w2, _ = T.philox4(seed, lane, c, episode)
        pick, probs, _, _ = ST.softmax_sample(s, g, f32(iT), w2)
        a, _ = T.explore(seed, thr, lane, c, episode, M, pick)
    return dict(actions=a.astype(np.int32), scores=s, probs=probs, value=v, hp=hp)


def select(parts, x, state, live, seed, thr, lane, c, episode, M, mode=ST.ARGMAX, iT=1.0, head=None, commit=False):
    """One kernel launch: (outputs, new state).  Done lanes (~live): action -1, zero columns, value 0, state untouched."""
    h = h_in(state, c)
    o = decide(parts, x, h, seed, thr, lane, c, episode, M, mode, iT, head)
    live = np.asarray(live, bool)
    out = dict(actions=np.where(live, o["actions"], -1).astype(np.int32),
               features=np.where(live[None], x, f32(0)).astype(f32), scores=np.where(live[None], o["scores"], f32(0)),
               probs=np.where(live[None], o["probs"], f32(0)), hidden=np.where(live[None], h, f32(0)),
               value=None if o["value"] is None else np.where(live, o["value"], f32(0)))
    new = np.where(live[None] & bool(commit), o["hp"], np.asarray(state, f32)).astype(f32)
    return out, new


def run_lane(parts, xs, cs, lives, seed, thr, lane, episodes, M, mode=ST.ARGMAX, iT=1.0, head=None, state0=None):
    """The sequential runner of ONE lane over T decisions: xs [T, F], cs [T], lives [T], episodes [T].  Carries the state,
    restarts it where c == 0, leaves it where the lane is done.  Returns dict of [T, ...] arrays and the final state."""
    H = parts[1].shape[1]
    st = np.zeros((H, 1), f32) if state0 is None else np.asarray(state0, f32).reshape(H, 1)
    outs = []
    for t in range(len(cs)):
        o, st = select(parts, np.asarray(xs[t], f32).reshape(-1, 1), st, [bool(lives[t])], seed, thr,
                       np.asarray([lane], np.uint64), np.asarray([cs[t]]), np.asarray([episodes[t]]), M, mode, iT, head,
                       commit=True)
        outs.append(o)
    keys = [k for k in outs[0] if outs[0][k] is not None]
    return {k: np.stack([o[k][..., 0] for o in outs]) for k in keys}, st[:, 0]
