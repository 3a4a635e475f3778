"""Generalised advantage estimation over the [T, N] slabs of a fused rollout, on the device (include/abr_env.h: abr_gae;
the lane loop is csrc/abr_lane_jump.h: gae_lane).

    out = env.step_policy(ctl, 48, want_probs=True, want_values=True)
    adv, ret = gae(out["reward"], out["values"], out["last_value"], out["done"], out["actions"])

The bookkeeping is the contract's, not the trainer's: done[t] ends the recurrence at the step that ended the episode (row
t + 1 already belongs to the re-armed one), a step whose action is -1 took no decision and gets adv = ret = 0, and every
done bit -- a time-out included -- is a terminal state.  Any float32 reward slab will do: the environment's reward is a
cost with no quality term, and a trainer may shape it first.
"""
import torch

from . import _lib


def _slab(t, name, dtype, shape, device):
    if not torch.is_tensor(t) or t.dtype != dtype or t.device != device or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be a {dtype} tensor of shape {shape} on {device}")
    return t.contiguous()


def gae(reward, values, last_value, done, actions=None, gamma=0.99, lam=0.95, out=None):
    """(advantages, returns), float32 [T, N] each.  reward, values float32 [T, N]; last_value float32 [N] (the value of the
    state after the last row); done uint8 or bool [T, N]; actions int32 [T, N] or None (every step live).  gamma and lam
    in [0, 1], passed as float32.  out: an (advantages, returns) pair to fill instead of fresh tensors; it may not overlap
    the inputs.  Runs on the current stream of the tensors' device without synchronising."""
    if not torch.is_tensor(reward) or reward.dim() != 2 or reward.dtype != torch.float32:
        raise ValueError("reward must be a float32 tensor [T, N]")
    T, N = reward.shape
    dev = reward.device
    if dev.type != "cuda":
        raise ValueError("gae runs on the device: the slabs must be device tensors")
    if T < 1 or N < 1:
        raise ValueError("gae needs T >= 1 and N >= 1")
    reward = _slab(reward, "reward", torch.float32, (T, N), dev)
    values = _slab(values, "values", torch.float32, (T, N), dev)
    last_value = _slab(last_value, "last_value", torch.float32, (N,), dev)
    if torch.is_tensor(done) and done.dtype == torch.bool:
        done = done.view(torch.uint8)
    done = _slab(done, "done", torch.uint8, (T, N), dev)
    if actions is not None:
        actions = _slab(actions, "actions", torch.int32, (T, N), dev)
    for name, x in (("gamma", gamma), ("lam", lam)):
        if isinstance(x, bool) or not 0.0 <= float(x) <= 1.0:
            raise ValueError(f"{name} must be a number in [0, 1], got {x!r}")
    if out is None:
        adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    else:
        adv, ret = out
        for name, t in (("out[0]", adv), ("out[1]", ret)):
            if not torch.is_tensor(t) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous tensor")
            _slab(t, name, torch.float32, (T, N), dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        _lib.check(L.abr_gae(_lib.ptr(reward), _lib.ptr(values), _lib.ptr(last_value), _lib.ptr(done), _lib.ptr(actions),
                             T, N, float(gamma), float(lam), _lib.ptr(adv), _lib.ptr(ret), _lib.current_stream(dev)), L)
    return adv, ret
