"""A learned bitrate policy: a small MLP evaluated on the device on each lane's exact call-site state (Pensieve-style
learned ABR).  The contract -- the features, the fmaf order of the forward pass, the first argmax and the exploration
draw -- is include/abr_env.h: abr_policy; the arithmetic is csrc/abr_lane_jump.h (policy_features, policy_forward).

    net = torch.nn.Sequential(nn.Linear(F, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, M))
    ctl = PolicyController.from_module(EnvPlayer(env), net, window=8, explore=0.1)
    out = env.step_policy(ctl, 48, want_features=True)     # features, actions, rewards, done for a trainer
    ...train net in PyTorch...
    ctl.load_weights(net)                                   # refresh the device copy in place, no sync

A stochastic policy (A2C, PPO) samples on the device instead: PolicyController(..., sample="softmax", temperature=T)
draws each action from softmax(scores / T), and want_probs=True returns that distribution (include/abr_env.h:
abr_policy_sampling).

An actor-critic trainer whose critic shares the actor's trunk hands the controller the critic's Linear(in, 1) head
(value_head=...): select(want_value=True) and env.step_policy(ctl, n, want_values=True) then report V(s) of the state each
decision was taken in, computed in the same kernel (include/abr_env.h: abr_policy_value).  A critic that is a separate
network is the trainer's own business: one batched GEMM over the features slab, which torch does faster than any
per-lane kernel.

engine="matrix" evaluates the same network as f32 MFMA products (include/abr_env.h: abr_policy_mx): 0..3 hidden layers of
1..128 units (Pensieve's 128-wide actor, PPO's 3 x 128), every output bit for bit what engine="lane" gives on a shape both
can run.

    net = torch.nn.Sequential(nn.Linear(F, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, M))
    ctl = PolicyController.from_module(EnvPlayer(env), net, window=8, engine="matrix")

PolicyPopulation runs P networks of one shape in a single launch, member m on lanes [m * group, (m + 1) * group)
(include/abr_env.h: abr_policy_pop) -- evolution strategies, population-based training, checkpoint leagues, A/B runs:

    pop = PolicyPopulation(EnvPlayer(env), [net_0, ..., net_63], group=env.n_lanes // 64, window=8)
    out = env.step_policy(pop, 48)                          # every member on its own lanes, one launch per decision
    pop.load_weights(next_generation)                       # in place, no sync
    best = pop.member(3)                                    # an ordinary PolicyController over member 3's weights

RecurrentPolicyController is a GRU-cell actor whose hidden state lives on the device, one column per lane, persists
across decisions and launches and restarts with the lane's episode (include/abr_env.h: abr_policy_gru):

    ctl = RecurrentPolicyController(EnvPlayer(env), nn.GRUCell(F, 32), nn.Linear(32, M), window=8, sample="softmax")
    out = env.step_policy(ctl, 48, want_features=True, want_hidden=True)   # hidden[t]: the state decision t started from

RecurrentPolicyPopulation is the two together: P GRU cells of one shape, member m on its own lane group and its own
columns of the one hidden slab (include/abr_env.h: abr_env_gru_step_pop) -- a recurrent actor for evolution
strategies and population-based training, which need no backpropagation through time:

    pop = RecurrentPolicyPopulation(EnvPlayer(env), [(cell_0, head_0), ..., (cell_63, head_63)], group=env.n_lanes // 64)
    out = env.step_policy(pop, 48)                          # every member on its own lanes, one launch per decision
"""
import collections
import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

OBS_NAMES = ["buffer_level", "last_bitrate", "chunks_left", "latency"]
SAMPLE_MODES = {"argmax": _lib.POLICY_ARGMAX, "softmax": _lib.POLICY_SOFTMAX}

# One row per engine of each family: its limits (MLP: most hidden layers, widest hidden layer; GRU: most units), the C
# struct, the size query, and the (select, step) entry points of a single network and of a population.  The lane MLP
# alone has a pair per mode: plain, sampled, actor-critic (PolicyController.entries).
Engine = collections.namedtuple("Engine", "limits struct size_query single pop")
ENGINES = {
    "mlp": {"lane": Engine((_lib.POLICY_MAX_HIDDEN, _lib.POLICY_MAX_WIDTH), _lib.Policy, "abr_policy_weights_bytes",
                           (("abr_env_policy_select", "abr_env_step_policy"),
                            ("abr_env_policy_select_sampled", "abr_env_step_policy_sampled"),
                            ("abr_env_policy_select_ac", "abr_env_step_policy_ac")),
                           ("abr_env_policy_select_pop", "abr_env_step_policy_pop")),
            "matrix": Engine((_lib.POLICY_MX_MAX_HIDDEN, _lib.POLICY_MX_MAX_WIDTH), _lib.PolicyMx,
                             "abr_policy_mx_weights_bytes", (("abr_env_policy_select_mx", "abr_env_step_policy_mx"),),
                             ("abr_env_policy_select_mx_pop", "abr_env_step_policy_mx_pop"))},
    "gru": {"lane": Engine((_lib.POLICY_GRU_MAX_HIDDEN,), _lib.PolicyGru, "abr_policy_gru_weights_bytes",
                           (("abr_env_policy_select_gru", "abr_env_step_policy_gru"),),
                           ("abr_env_gru_select_pop", "abr_env_gru_step_pop")),
            "matrix": Engine((_lib.POLICY_GRU_MX_MAX_HIDDEN,), _lib.PolicyGruMx, "abr_policy_gru_mx_weights_bytes",
                             (("abr_env_gru_mx_select", "abr_env_gru_mx_step"),),
                             ("abr_env_gru_mx_select_pop", "abr_env_gru_mx_step_pop"))},
}


def _mlp_engine(engine):
    if engine not in ENGINES["mlp"]:
        raise ValueError(f"engine must be one of {sorted(ENGINES['mlp'])}, got {engine!r}")
    return ENGINES["mlp"][engine]


def _gru_engine(engine):
    if engine not in ENGINES["gru"]:
        raise ValueError(f"engine must be 'lane' or 'matrix', got {engine!r}")
    return ENGINES["gru"][engine]


def _as_f32(t, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t, np.float32))
    return t.detach().to(device=device, dtype=torch.float32)


def _is_array(t):
    return torch.is_tensor(t) or isinstance(t, np.ndarray)


def _fill(blob, tensors, device):
    """Copy `tensors`, in order, into blob [rows, words] at a running offset, each tensor holding its part of every row
    ([rows, ...]; one row: any shape): in place, on the current stream, without synchronising."""
    rows, o = blob.shape[0], 0
    with torch.no_grad():
        for t in tensors:
            t = _as_f32(t, device).reshape(rows, -1)
            blob[:, o:o + t.shape[1]].copy_(t, non_blocking=True)
            o += t.shape[1]
    assert o == blob.shape[1]


def pack_layers(layers):
    """The weight blob's layout on the host: per layer W [out][in] row-major, then b [out], layers in order (float32)."""
    parts = []
    for W, b in layers:
        for t in (W, b):
            t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            parts.append(np.asarray(t, np.float32).reshape(-1))
    return np.concatenate(parts)


def pack_gru(cell, head):
    """The recurrent policy's weight blob on the host: W_ih [3H, F], W_hh [3H, H], b_ih [3H], b_hh [3H] (torch.nn.GRUCell's
    own tensors, gates r, z, n), then the head's W [M, H] and b [M], concatenated (float32)."""
    return pack_layers([cell[:2], cell[2:], head])


def _select(ctl, want_features, want_scores, want_probs, want_value, want_hidden=False, commit=None):
    """The select of every controller: the outputs that are wanted, then the controller's select entry
    (BatchedABREnv._policy_call, which asks ctl.entries() which one that is)."""
    env = ctl.player.env
    N, dev = env.n_lanes, env.device
    f32 = lambda rows, want: torch.empty(rows, N, dtype=torch.float32, device=dev) if want else None
    out = dict(actions=torch.empty(N, dtype=torch.int32, device=dev), features=f32(ctl.feature_dim, want_features),
               scores=f32(ctl.n_rates, want_scores), probs=f32(ctl.n_rates, want_probs))
    pol = ctl.bound(env)
    val = ctl.value() if want_value else None
    if want_value:
        out["value"] = torch.empty(N, dtype=torch.float32, device=dev)
    if want_hidden:
        out["hidden"] = f32(ctl.hidden_size, True)
    env._policy_call(ctl, pol, val, out, commit=commit)
    return out


class _Controller:
    """What the two single-network controllers share: the constructor's preamble, the settings every policy has (norm,
    explore, sample, temperature), the value head, the copies into the device blobs and the environment check of bound().
    A subclass owns its shape: the checks, `_shape` (its engine's struct with the shape filled in, which the size query
    reads and `_struct` copies), `_struct` and its load_weights."""

    _commit = None        # what next_bitrate passes select's entry for commit: None where the entry takes none

    def _open(self, player, engine, row, window, device):
        """The preamble of both constructors: the player, the device, the window and the sizes the MPD gives.  Returns the
        MPD (for _norm)."""
        self.engine, self._row = engine, row
        self.player = player
        env = getattr(player, "env", None)
        self.device = torch.device(device) if device is not None else (env.device if env is not None else
                                                                       torch.device("cuda"))
        if isinstance(window, bool) or int(window) != window or not 0 <= int(window) <= _lib.POLICY_MAX_WINDOW:
            raise ValueError(f"window must be an integer in 0..{_lib.POLICY_MAX_WINDOW}")
        self.window = int(window)
        mpd = player.get_mpd()
        self.n_rates, self.video_length = len(mpd.chunk_list()[0].bitrates), int(mpd.video_length)
        self.feature_dim = 4 + self.window + self.n_rates
        return mpd

    def _blob_words(self):
        """The float32 words of the weight blob, by the engine's size query on `_shape`."""
        nbytes = C.c_size_t()
        _lib.check(getattr(_lib.lib(), self._row.size_query)(C.byref(self._shape), self.n_rates, C.byref(nbytes)))
        return nbytes.value // 4

    def _norm(self, norm, mpd):
        F = self.feature_dim
        if norm is None:
            return None
        if isinstance(norm, str):
            if norm != "default":
                raise ValueError("norm is 'default', None or (shift, scale)")
            top = max(float(b) for c in mpd.chunk_list() for b in c.bitrates)
            scale = np.empty(F)
            scale[0] = scale[3] = 1.0 / float(mpd.max_buffer)
            scale[1] = 1.0 / top
            scale[2] = 1.0 / self.video_length
            scale[4:] = 1.0 / top
            shift = np.zeros(F)
        else:
            shift, scale = (np.asarray(x, np.float64).ravel() for x in norm)
            if shift.size != F or scale.size != F:
                raise ValueError(f"shift and scale need {F} entries each")
        return torch.tensor(np.stack([shift, scale]), dtype=torch.float64, device=self.device).contiguous()

    @property
    def explore(self):
        return self._explore

    @explore.setter
    def explore(self, eps):
        eps = float(eps)
        if not 0.0 <= eps <= 1.0:
            raise ValueError("explore must be in [0, 1]")
        self._explore = eps
        self.explore_threshold = 1 << 32 if eps >= 1.0 else int(math.floor(eps * 2.0 ** 32))

    @property
    def sample(self):
        return self._sample

    @sample.setter
    def sample(self, mode):
        if mode not in SAMPLE_MODES:
            raise ValueError(f"sample must be one of {sorted(SAMPLE_MODES)}, got {mode!r}")
        self._sample = mode

    @property
    def temperature(self):
        return self._temperature

    @temperature.setter
    def temperature(self, t):
        if isinstance(t, bool):
            raise ValueError("temperature must be a finite number > 0")
        t = float(t)
        with np.errstate(all="ignore"):
            inv = np.float32(1.0 / t) if math.isfinite(t) and t > 0.0 else np.float32(0.0)
        if not (math.isfinite(t) and t > 0.0 and np.isfinite(inv) and inv > 0.0):
            raise ValueError(f"temperature must be finite and > 0 with a finite, nonzero float32 1/temperature; got {t}")
        self._temperature, self.inv_temperature = t, inv

    def sampling(self):
        """The abr_policy_sampling struct of the current sample mode and temperature."""
        smp = _lib.PolicySampling()
        smp.mode = SAMPLE_MODES[self._sample]
        smp.inv_temperature = float(self.inv_temperature)
        return smp

    def feature_names(self):
        return (OBS_NAMES + [f"throughput[-{self.window - k}]" for k in range(self.window)] +
                [f"bitrate[{m}]" for m in range(self.n_rates)])

    # -- the value head and the copies ---------------------------------------------
    def _head_parts(self, head):
        """(Wv, bv) of a value head -- an nn.Linear(value_in, 1) with a bias, or a (Wv, bv) pair -- after checking it
        against this policy's shape; ValueError otherwise."""
        if isinstance(head, torch.nn.Module):
            if type(head) is not torch.nn.Linear:
                raise ValueError(f"a value head is nn.Linear({self.value_in}, 1), got {type(head).__name__}")
            if head.bias is None:
                raise ValueError("value head: Linear without a bias")
            if head.in_features != self.value_in or head.out_features != 1:
                raise ValueError(f"value head: Linear({head.in_features}, {head.out_features}), this policy needs "
                                 f"Linear({self.value_in}, 1)")
            return head.weight, head.bias
        try:
            Wv, bv = head
        except (TypeError, ValueError):
            raise ValueError("value_head is nn.Linear(in, 1) or (Wv, bv)") from None
        if tuple(np.shape(Wv)) not in ((self.value_in,), (1, self.value_in)) or tuple(np.shape(bv)) not in ((), (1,)):
            raise ValueError(f"value head: Wv must be [{self.value_in}] or [1, {self.value_in}] and bv a scalar or [1], "
                             f"got {tuple(np.shape(Wv))} / {tuple(np.shape(bv))}")
        return Wv, bv

    def _new_head(self, value_head):
        """None without a value head, else a zeroed head [value_in + 1] once `value_head` has passed _head_parts."""
        if value_head is None:
            return None
        self._head_parts(value_head)
        return torch.zeros(self.value_in + 1, dtype=torch.float32, device=self.device)

    def _load(self, tensors, value_head):
        """Copy the blob's tensors, which the caller has checked, and the value head where one is given (refused by a
        controller built without one, and checked, before anything is copied)."""
        if value_head is not None:
            if self.value_head is None:
                raise ValueError("this controller was built without a value head")
            _fill(self.value_head[None], self._head_parts(value_head), self.device)
        _fill(self.weights[None], tensors, self.device)

    def value(self):
        """The abr_policy_value struct (it points into this controller's value head); ValueError without a head."""
        if self.value_head is None:
            raise ValueError(f"values need a value head: {type(self).__name__}(..., value_head=(Wv, bv))")
        v = _lib.PolicyValue()
        v.head_dev, v.head_bytes = self.value_head.data_ptr(), self.value_head.numel() * 4
        return v

    # -- decisions -------------------------------------------------------------------
    def _env(self, env):
        """The environment of a launch (the player's by default), refused where its ladder is not this policy's."""
        env = env if env is not None else self.player.env
        if env.n_rates != self.n_rates:
            raise ValueError(f"the policy is for {self.n_rates} bitrates, the environment has {env.n_rates}")
        return env

    def select(self, want_features=True, want_scores=True, want_probs=False, want_value=False):
        """One decision per lane on the environment's current state (no step): dict(actions int32 [N], features float32
        [F, N], scores float32 [M, N], probs float32 [M, N] -- the policy's distribution before exploration); a lane
        whose done bits are set answers -1 with zero columns.  An entry that is not wanted is None.  want_value=True
        (a controller with a value head) adds value float32 [N], the critic's V of the current state, 0 on a done lane."""
        return _select(self, want_features, want_scores, want_probs, want_value)

    def next_bitrate(self):
        """int32 [N]: the policy's action for each lane (-1 for finished lanes).  A recurrent policy commits the new
        hidden state: the player's loop steps these actions next."""
        return _select(self, False, False, False, False, False, self._commit)["actions"]


class PolicyController(_Controller):
    """An MLP policy over `player` (an EnvPlayer: the environment is player.env).

    layers: [(W [out, in], b [out]), ...], hidden layers first (0..2 of widths 1..64, ReLU after each), then the output
    layer of width n_rates; the input width is feature_dim = 4 + window + n_rates.  norm: "default" (shift 0; scale
    1/max_buffer for the buffer and the latency, 1/top bitrate for bitrates and throughputs, 1/video_length for the chunks
    left), None (raw values), or (shift [F], scale [F]).  explore in [0, 1]: the probability of taking the random policy's
    action instead of the argmax (threshold floor(explore * 2^32)), drawn with `seed` exactly as step_random draws.
    sample: "argmax" (the first argmax) or "softmax" (a draw from softmax(scores / temperature) with word 2 of the same
    philox block); temperature > 0, passed as float32(1 / temperature).  Both can be changed between launches.
    value_head: None, or (Wv [in] or [1, in], bv scalar or [1]) -- the critic's head over the last hidden layer's output
    (in = the last hidden width, or feature_dim without a hidden layer).
    engine: "lane" (one thread per lane; 0..2 hidden layers of 1..64 units) or "matrix" (f32 MFMA; 0..3 hidden layers of
    1..128 units).  The outputs of a shape both can run are bit-identical."""

    method = "policy"

    def __init__(self, player, layers, window=8, norm="default", explore=0.0, seed=0, device=None, sample="argmax",
                 temperature=1.0, value_head=None, engine="lane"):
        row = _mlp_engine(engine)
        max_hidden, max_width = row.limits
        mpd = self._open(player, engine, row, window, device)
        shapes = [tuple(np.shape(W)) for W, _ in layers]
        if not 1 <= len(layers) <= max_hidden + 1:
            raise ValueError(f"1..{max_hidden + 1} layers (0..{max_hidden} hidden)")
        fan_in = self.feature_dim
        for li, ((W, b), sh) in enumerate(zip(layers, shapes)):
            if len(sh) != 2 or sh[1] != fan_in or tuple(np.shape(b)) != (sh[0],):
                raise ValueError(f"layer {li}: W must be [out, {fan_in}] and b [out], got {sh} / {tuple(np.shape(b))}")
            last = li == len(layers) - 1
            if last and sh[0] != self.n_rates:
                raise ValueError(f"the output layer has width {sh[0]}, the MPD has {self.n_rates} bitrates")
            if not last and not 1 <= sh[0] <= max_width:
                raise ValueError(f"hidden width {sh[0]} outside 1..{max_width}")
            fan_in = sh[0]
        self.widths = [sh[0] for sh in shapes[:-1]]
        self.shapes = shapes
        self.value_in = self.widths[-1] if self.widths else self.feature_dim
        self._shape = row.struct()
        self._shape.window, self._shape.n_hidden = self.window, len(self.widths)
        for k, w in enumerate(self.widths):
            self._shape.width[k] = w
        self.weights = torch.zeros(self._blob_words(), dtype=torch.float32, device=self.device)
        self.value_head = self._new_head(value_head)                      # a bad head is refused before anything is copied
        self.load_weights(layers, value_head=value_head)
        self.norm = self._norm(norm, mpd)
        self.explore = explore
        self.seed = int(seed)
        self.sample = sample
        self.temperature = temperature

    # -- construction ----------------------------------------------------------
    @classmethod
    def from_module(cls, player, module, value_head=None, engine="lane", **kw):
        """From nn.Sequential(Linear, ReLU, ..., Linear) with 0..2 hidden layers (0..3 with engine="matrix"); any other
        shape is refused.  value_head: the critic's nn.Linear(in, 1) over the last hidden layer's output (or (Wv, bv))."""
        layers = cls.module_layers(module, _mlp_engine(engine).limits[0])
        return cls(player, layers, value_head=value_head, engine=engine, **kw)

    @staticmethod
    def module_layers(module, max_hidden=_lib.POLICY_MAX_HIDDEN):
        """[(weight, bias)] of nn.Sequential(Linear, ReLU, Linear, ...); ValueError for any other module."""
        nn = torch.nn
        mods = list(module) if isinstance(module, nn.Sequential) else None
        if not mods or len(mods) % 2 == 0 or len(mods) > 2 * max_hidden + 1:
            raise ValueError(f"a policy module is nn.Sequential(Linear, ReLU, ..., Linear) with 0..{max_hidden} hidden "
                             "layers")
        for k, m in enumerate(mods):
            want = nn.Linear if k % 2 == 0 else nn.ReLU
            if type(m) is not want:
                raise ValueError(f"module {k} is {type(m).__name__}, expected {want.__name__}")
            if want is nn.Linear and m.bias is None:
                raise ValueError(f"module {k}: Linear without a bias")
        return [(m.weight, m.bias) for m in mods[0::2]]

    # -- the weights -------------------------------------------------------------
    def _layers(self, layers):
        """`layers` (a list of (W, b), or an nn.Sequential) as a list of (W, b) of this controller's shapes; ValueError
        otherwise."""
        if isinstance(layers, torch.nn.Module):
            layers = self.module_layers(layers, self._row.limits[0])
        if [tuple(np.shape(W)) for W, _ in layers] != self.shapes:
            raise ValueError(f"layer shapes {[tuple(np.shape(W)) for W, _ in layers]}, this policy has {self.shapes}")
        return layers

    def load_weights(self, layers, value_head=None):
        """Copy new weights (a list of (W, b) of this controller's shapes, or an nn.Sequential) into the device blob in
        place, on the current stream, without synchronising.  value_head (nn.Linear(in, 1) or (Wv, bv)) refreshes the
        value head the same way; a controller built without one refuses it."""
        self._load([t for layer in self._layers(layers) for t in layer], value_head)

    def layers(self):
        """[(W, b)] views of the device blob."""
        out, o, fan_in = [], 0, self.feature_dim
        for out_w, _ in self.shapes:
            W = self.weights[o:o + out_w * fan_in].view(out_w, fan_in)
            o += out_w * fan_in
            out.append((W, self.weights[o:o + out_w]))
            o += out_w
            fan_in = out_w
        return out

    def _struct(self, wptr, nbytes, norm):
        p = self._row.struct.from_buffer_copy(self._shape)
        p.weights_dev, p.weights_bytes = wptr, nbytes
        p.norm_dev = norm.data_ptr() if norm is not None else None
        p.seed = self.seed & (2 ** 64 - 1)
        p.explore_threshold = self.explore_threshold
        return p

    def bound(self, env=None):
        """The struct of this controller's engine for the C ABI -- abr_policy, or abr_policy_mx for "matrix" (it points
        into this controller's tensors)."""
        self._env(env)
        return self._struct(self.weights.data_ptr(), self.weights.numel() * 4, self.norm)

    # -- decisions ---------------------------------------------------------------
    def entries(self, val, want_probs):
        """What BatchedABREnv._policy_call asks a controller: the (select, step) pair of C entry points it takes with the
        value struct `val` (None: no values) and with or without probs, the structs those take after the policy's, and
        how many optional output groups they have (0: none, 1: probs, 2: and value(s), 3: and hidden)."""
        smp, pairs = self.sampling(), self._row.single
        if len(pairs) == 1:                                               # one entry pair for every mode
            return pairs[0], (smp, val), 2
        plain, sampled, actor_critic = pairs
        if val is not None:
            return actor_critic, (smp, val), 2
        if self.uses_sampled_entries(want_probs):
            return sampled, (smp,), 1
        return plain, (), 0

    def uses_sampled_entries(self, want_probs):
        """An argmax policy without probs keeps the abr_policy entry points; anything else takes the sampled ones."""
        return self.sample != "argmax" or bool(want_probs)

    def features(self):
        """float32 [F, N]: the network's input on the current state."""
        return self.select(True, False)["features"]

    def scores(self):
        """float32 [M, N]: the network's output on the current state."""
        return self.select(False, True)["scores"]


class RecurrentPolicyController(_Controller):
    """A recurrent policy over `player`: one GRU cell per lane, then Linear(H, M) over the new hidden state
    (include/abr_env.h: abr_policy_gru).  The hidden state is per-lane device state that persists across decisions and
    across launches and restarts with the lane's episode: a decision at a lane's first chunk (chunk_id == 0) starts from
    zeros whatever `hidden` holds, so reset, a masked reset, an auto_reset re-arm and the episode sampler all restart the
    recurrence.

        cell, head = nn.GRUCell(F, 32), nn.Linear(32, M)
        ctl = RecurrentPolicyController(EnvPlayer(env), cell, head, window=8, sample="softmax")
        out = env.step_policy(ctl, 48, want_features=True, want_hidden=True)
        h1 = cell(out["features"][t].T, out["hidden"][t].T)      # the step again in torch, for the loss
        ctl.load_weights(cell, head)                              # in place, no sync

    cell: an nn.GRUCell(feature_dim, H) with bias, or (W_ih [3H, F], W_hh [3H, H], b_ih [3H], b_hh [3H]) in GRUCell's
    layout and gate order (r, z, n); 1 <= H <= 64, or 128 with engine="matrix".  head: nn.Linear(H, n_rates) or
    (W [M, H], b [M]).  value_head: None, nn.Linear(H, 1) or (Wv, bv), the critic's head over the new hidden state.
    window, norm, explore, seed, sample and temperature are PolicyController's.  It owns `weights` (the blob: the cell's
    four parameters, then the head's two, concatenated) and `hidden`, float32 [H, N], which starts at zero.

    engine: "lane" (the default: one thread per lane, abr_policy_gru) or "matrix" (the same chains as f32 MFMA products,
    abr_policy_gru_mx: H up to 128, and bit for bit the lane engine's outputs and state where both run).  Everything
    else -- the blob, `hidden`, load_weights, select, next_bitrate, value() -- is the same object either way.

    Populations: RecurrentPolicyPopulation (PolicyPopulation's members are MLPs).  Not covered: ShardedABREnv, LSTM cells
    and stacked cells.  A checkpoint taken
    mid-episode (env.state_dict()) does not contain the policy's state: save ctl.hidden next to it."""

    method = "policy_gru"
    engine = "lane"
    _commit = True

    def __init__(self, player, cell, head, window=8, norm="default", explore=0.0, seed=0, sample="argmax",
                 temperature=1.0, value_head=None, device=None, engine="lane"):
        row = _gru_engine(engine)
        self.max_hidden, = row.limits
        env = getattr(player, "env", None)
        if type(env).__name__ == "ShardedABREnv":
            raise ValueError("RecurrentPolicyController does not run on a ShardedABREnv: the hidden state is one slab "
                             "of one environment's lanes")
        mpd = self._open(player, engine, row, window, device)
        self.hidden_size = None
        parts = self._parts(cell, head)                                   # refuse bad shapes before anything is allocated
        self.hidden_size = self.value_in = int(np.shape(parts[1])[1])
        self.value_head = self._new_head(value_head)
        self.explore, self.seed, self.sample, self.temperature = explore, int(seed), sample, temperature
        self.norm = self._norm(norm, mpd)
        self._shape = row.struct()
        self._shape.window, self._shape.hidden = self.window, self.hidden_size
        words = self._blob_words()
        self.n_lanes = int(env.n_lanes) if env is not None else None
        if self.n_lanes is None:
            raise ValueError("RecurrentPolicyController needs player.env: the hidden state is [H, env.n_lanes]")
        self.weights = torch.zeros(words, dtype=torch.float32, device=self.device)
        self.hidden = torch.zeros(self.hidden_size, self.n_lanes, dtype=torch.float32, device=self.device)
        self._load(parts, value_head)

    # -- the weights -------------------------------------------------------------
    def _parts(self, cell, head):
        """(W_ih, W_hh, b_ih, b_hh, W_out, b_out) after checking every shape; ValueError otherwise."""
        F, M = self.feature_dim, self.n_rates
        if isinstance(cell, torch.nn.Module):
            if type(cell) is not torch.nn.GRUCell:
                raise ValueError(f"a recurrent policy's cell is nn.GRUCell({F}, H), got {type(cell).__name__}")
            if not cell.bias:
                raise ValueError("cell: GRUCell without a bias")
            cell = (cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)
        try:
            W_ih, W_hh, b_ih, b_hh = cell
        except (TypeError, ValueError):
            raise ValueError("cell is nn.GRUCell(F, H) or (W_ih, W_hh, b_ih, b_hh)") from None
        sh = tuple(np.shape(W_hh))
        H = sh[1] if len(sh) == 2 else -1
        if not 1 <= H <= self.max_hidden:
            raise ValueError(f"cell: W_hh must be [3H, H] with H in 1..{self.max_hidden}, got {sh}")
        if self.hidden_size is not None and H != self.hidden_size:
            raise ValueError(f"cell: {H} units, this policy has {self.hidden_size}")
        got = tuple(tuple(np.shape(t)) for t in (W_ih, W_hh, b_ih, b_hh))
        want = ((3 * H, F), (3 * H, H), (3 * H,), (3 * H,))
        if got != want:
            raise ValueError(f"cell: W_ih, W_hh, b_ih, b_hh must be {want}, got {got}")
        if isinstance(head, torch.nn.Module):
            if type(head) is not torch.nn.Linear:
                raise ValueError(f"a recurrent policy's head is nn.Linear({H}, {M}), got {type(head).__name__}")
            if head.bias is None:
                raise ValueError("head: Linear without a bias")
            head = (head.weight, head.bias)
        try:
            W, b = head
        except (TypeError, ValueError):
            raise ValueError("head is nn.Linear(H, n_rates) or (W, b)") from None
        if tuple(np.shape(W)) != (M, H) or tuple(np.shape(b)) != (M,):
            raise ValueError(f"head: W must be [{M}, {H}] and b [{M}], got {tuple(np.shape(W))} / {tuple(np.shape(b))}")
        return W_ih, W_hh, b_ih, b_hh, W, b

    def load_weights(self, cell, head, value_head=None):
        """Copy new weights (an nn.GRUCell and an nn.Linear of this controller's shapes, or the tuples) into the device
        blob in place, on the current stream, without synchronising; value_head refreshes the critic's head the same way.
        The hidden state is not touched."""
        self._load(self._parts(cell, head), value_head)

    def reset_hidden(self, mask=None):
        """Zero the hidden state of every lane, or of the lanes where mask (bool [N]) is set.  A new episode needs no call:
        a lane's first decision starts from zeros by the contract."""
        if mask is None:
            self.hidden.zero_()
        else:
            mask = torch.as_tensor(mask, device=self.device).to(torch.bool)
            if tuple(mask.shape) != (self.n_lanes,):
                raise ValueError(f"mask must be bool [{self.n_lanes}]")
            self.hidden.masked_fill_(mask[None, :], 0.0)

    # -- the C ABI ---------------------------------------------------------------
    def _struct(self, wptr, nbytes, norm, sptr, sbytes):
        p = self._row.struct.from_buffer_copy(self._shape)
        p.weights_dev, p.weights_bytes = wptr, nbytes
        p.norm_dev = norm.data_ptr() if norm is not None else None
        p.state_dev, p.state_bytes = sptr, sbytes
        p.seed = self.seed & (2 ** 64 - 1)
        p.explore_threshold = self.explore_threshold
        return p

    def bound(self, env=None):
        """The abr_policy_gru struct, or abr_policy_gru_mx with engine="matrix" (it points into this controller's tensors)."""
        env = self._env(env)
        if int(env.n_lanes) != self.n_lanes:
            raise ValueError(f"the hidden state is for {self.n_lanes} lanes, the environment has {env.n_lanes}")
        return self._struct(self.weights.data_ptr(), self.weights.numel() * 4, self.norm, self.hidden.data_ptr(),
                            self.hidden.numel() * 4)

    # -- decisions ---------------------------------------------------------------
    def select(self, want_features=True, want_scores=True, want_probs=False, want_value=False, want_hidden=False,
               commit=False):
        """One decision per lane on the environment's current state (no step): the dict of PolicyController.select, and
        with want_hidden=True hidden float32 [H, N], the state each decision was taken from (zeros at a lane's first
        chunk).  commit=False leaves `hidden` as it is, so that select can be called any number of times; commit=True
        advances it, which is right exactly when a step of the returned actions follows."""
        return _select(self, want_features, want_scores, want_probs, want_value, want_hidden, commit)

    def entries(self, val, want_probs):
        """As PolicyController.entries: one pair per engine for every mode, with the hidden outputs."""
        return self._row.single[0], (self.sampling(), val), 3


class _Population:
    """What the two populations share: P members of one shape over a prototype -- member 0 as an ordinary controller,
    which makes every check a controller makes and holds the settings all members share -- the lane arithmetic, the
    value heads, and the copies into `weights` [P, words] and `value_heads` [P, in + 1].  A subclass owns the forms its
    members come in, and its load_weights refuses a bad generation whole, before anything is copied."""

    _commit = None        # as _Controller._commit

    def __init__(self, player, group, engine):
        if isinstance(group, bool) or int(group) != group or int(group) < _lib.POLICY_POP_BLOCK or \
                int(group) % _lib.POLICY_POP_BLOCK:
            raise ValueError(f"group must be a positive multiple of {_lib.POLICY_POP_BLOCK}, got {group!r}")
        self.group = int(group)
        self.player, self.engine = player, engine

    def _adopt(self, proto, with_heads):
        """Take `proto` -- member 0, through the controller's own checks -- as the prototype, check that n_members cover
        the player's environment, and allocate the population's tensors; the prototype becomes a view of row 0."""
        self._proto, self._row = proto, proto._row
        self.device, self.window, self.n_rates = proto.device, proto.window, proto.n_rates
        self.feature_dim, self.value_in = proto.feature_dim, proto.value_in
        env = getattr(self.player, "env", None)
        if env is not None:
            self._check_cover(env)
        self.weights = torch.zeros(self.n_members, proto.weights.numel(), dtype=torch.float32, device=self.device)
        self.value_heads = (torch.zeros(self.n_members, self.value_in + 1, dtype=torch.float32, device=self.device)
                            if with_heads else None)
        proto.weights = self.weights[0]                                    # the prototype is member 0: no second copy
        proto.value_head = self.value_heads[0] if with_heads else None

    @staticmethod
    def _member_heads(heads, P):
        if heads is None:
            return None
        if not isinstance(heads, torch.nn.Module) and len(heads) == 2 and _is_array(heads[0]) and _is_array(heads[1]) \
                and np.ndim(heads[0]) == 2 and np.ndim(heads[1]) == 1 and np.shape(heads[1])[0] == P:
            if np.shape(heads[0])[0] != P:
                raise ValueError(f"stacked value heads: Wv must be [{P}, in] and bv [{P}]")
            return [(heads[0][m], heads[1][m]) for m in range(P)]
        heads = list(heads)
        if len(heads) != P:
            raise ValueError(f"{len(heads)} value heads for {P} members")
        return heads

    def _load_heads(self, value_heads):
        """None, or one head per member from either form, refused by a population built without heads.  A head's shape is
        the subclass's to check, in its own order (the prototype's _head_parts)."""
        heads = self._member_heads(value_heads, self.n_members)
        if heads is not None and self.value_heads is None:
            raise ValueError("this population was built without value heads")
        return heads

    def _check_cover(self, env):
        want = -(-int(env.n_lanes) // self.group)
        if self.n_members != want:
            raise ValueError(f"{self.n_members} members, {env.n_lanes} lanes in groups of {self.group} need {want}")

    # -- what all members share (checked by the controller's own setters) ------------
    explore = property(lambda self: self._proto.explore, lambda self, v: setattr(self._proto, "explore", v))
    sample = property(lambda self: self._proto.sample, lambda self, v: setattr(self._proto, "sample", v))
    temperature = property(lambda self: self._proto.temperature, lambda self, v: setattr(self._proto, "temperature", v))
    seed = property(lambda self: self._proto.seed, lambda self, v: setattr(self._proto, "seed", int(v)))
    norm = property(lambda self: self._proto.norm)
    explore_threshold = property(lambda self: self._proto.explore_threshold)
    inv_temperature = property(lambda self: self._proto.inv_temperature)

    def sampling(self):
        return self._proto.sampling()

    def feature_names(self):
        return self._proto.feature_names()

    # -- the weights -----------------------------------------------------------------
    def _index(self, m):
        if isinstance(m, bool) or int(m) != m or not 0 <= int(m) < self.n_members:
            raise IndexError(f"member {m!r} outside 0..{self.n_members - 1}")
        return int(m)

    def _member(self, m):
        """The prototype over row m of the weights and of the heads: a shallow copy over views."""
        c = copy.copy(self._proto)
        c.weights = self.weights[m]
        c.value_head = self.value_heads[m] if self.value_heads is not None else None
        return c

    def _copy(self, tensors, stacked, heads):
        """Copy a generation that has passed every check: `tensors` in blob order -- stacked [P, ...], one copy per
        tensor whatever P is, or a list per member -- and heads, None or (Wv, bv) per member."""
        if stacked:
            _fill(self.weights, tensors, self.device)
        else:
            for m, row in enumerate(tensors):
                _fill(self.weights[m:m + 1], row, self.device)
        if heads is not None:
            for m, head in enumerate(heads):
                _fill(self.value_heads[m:m + 1], head, self.device)

    # -- the lanes ---------------------------------------------------------------------
    def _n_lanes(self, env=None):
        env = env if env is not None else self.player.env
        return int(env.n_lanes)

    def member_of_lane(self):
        """int32 [N]: the member each local lane belongs to."""
        return (torch.arange(self._n_lanes(), dtype=torch.int64, device=self.device) // self.group).to(torch.int32)

    def lanes_of(self, m):
        """The slice of local lanes member m owns."""
        m = self._index(m)
        return slice(m * self.group, min((m + 1) * self.group, self._n_lanes()))

    # -- the C ABI ---------------------------------------------------------------------
    def population(self):
        """The abr_policy_pop struct."""
        p = _lib.PolicyPop()
        p.n_members, p.group = self.n_members, self.group
        return p

    def value(self):
        """abr_policy_value over member 0's head with ONE head's byte count; ValueError without heads."""
        if self.value_heads is None:
            raise ValueError(f"values need value heads: {type(self).__name__}(..., value_heads=[...])")
        v = _lib.PolicyValue()
        v.head_dev, v.head_bytes = self.value_heads.data_ptr(), self.value_heads.shape[1] * 4
        return v

    # -- decisions ---------------------------------------------------------------------
    def select(self, want_features=True, want_scores=True, want_probs=False, want_value=False):
        """One decision per lane on the environment's current state, every lane by its own member: the same dict as
        PolicyController.select."""
        return _select(self, want_features, want_scores, want_probs, want_value)

    def next_bitrate(self):
        """int32 [N]: each lane's action by its member's network (-1 for finished lanes).  A recurrent population
        commits the new hidden state: the player's loop steps these actions next."""
        return _select(self, False, False, False, False, False, self._commit)["actions"]


class PolicyPopulation(_Population):
    """P networks of ONE shape over `player`, each deciding for its own group of lanes in the same launch
    (include/abr_env.h: abr_policy_pop): local lane i belongs to member i // group, group is a positive multiple of 256,
    and P == ceil(n_lanes / group) -- the last member may own fewer lanes.  For every lane of member m every output is
    bit for bit what member(m), an ordinary PolicyController over that member's weights, gives on that lane.

    members: a list of P layer lists [(W, b), ...] or nn.Sequentials of one shape, or the stacked tensors
    [(W [P, out, in], b [P, out]), ...].  value_heads: None, a list of P heads (nn.Linear(in, 1) or (Wv, bv)), or the
    stacked pair (Wv [P, in], bv [P]).  Every other argument is PolicyController's and is shared by all members, with the
    same limits per engine; explore, sample, temperature and seed can be changed between launches.
    It owns weights float32 [P, words] and value_heads float32 [P, in + 1] (or None) on the device.

    Not covered: ShardedABREnv (it has no step_policy); per-member exploration, temperature or norm; and common random
    numbers across members under the episode sampler, which draws (trace, offset) per lane -- until the sampler can
    repeat a sequence per group, tile explicit reset(trace_id, start_offset) pairs over the groups."""

    method = "policy_population"

    def __init__(self, player, members, group, window=8, norm="default", explore=0.0, seed=0, sample="argmax",
                 temperature=1.0, value_heads=None, engine="lane", device=None):
        row = _mlp_engine(engine)
        super().__init__(player, group, engine)
        layer_lists = self._member_layers(members, row.limits[0])
        self.n_members = len(layer_lists)
        heads = self._member_heads(value_heads, self.n_members)
        # member 0 through the controller's own checks: shape, window, norm, explore, sample, temperature, head
        self._adopt(PolicyController(player, layer_lists[0], window=window, norm=norm, explore=explore, seed=seed,
                                     device=device, sample=sample, temperature=temperature,
                                     value_head=heads[0] if heads is not None else None, engine=engine),
                    heads is not None)
        self.widths, self.shapes = self._proto.widths, self._proto.shapes
        self.load_weights(layer_lists, value_heads=heads)

    @classmethod
    def from_modules(cls, player, nets, group, value_heads=None, **kw):
        """From P nn.Sequential(Linear, ReLU, ..., Linear) of one shape (as PolicyController.from_module)."""
        nets = list(nets)
        if not nets or not all(isinstance(n, torch.nn.Module) for n in nets):
            raise ValueError("from_modules takes a non-empty list of nn.Sequential")
        return cls(player, nets, group, value_heads=value_heads, **kw)

    # -- the members' inputs -------------------------------------------------------
    @staticmethod
    def _stacked(members):
        return (len(members) > 0 and not isinstance(members[0], torch.nn.Module) and len(members[0]) == 2 and
                _is_array(members[0][0]) and np.ndim(members[0][0]) == 3)

    @classmethod
    def _member_layers(cls, members, max_hidden):
        """A list of P layer lists from any of the three forms; ValueError for anything else."""
        if getattr(members, "method", None) == "policy_gru" or isinstance(members, torch.nn.GRUCell) or (
                isinstance(members, (list, tuple)) and any(getattr(m, "method", None) == "policy_gru" or
                                                           isinstance(m, torch.nn.GRUCell) for m in members)):
            raise ValueError("a population's members are MLPs: a recurrent policy (RecurrentPolicyController, GRUCell) "
                             "has per-lane state and is not supported in a PolicyPopulation")
        members = list(members) if not isinstance(members, torch.nn.Sequential) else None
        if not members:
            raise ValueError("members is a non-empty list of layer lists or nn.Sequentials, or stacked (W, b) tensors")
        if cls._stacked(members):
            P = int(np.shape(members[0][0])[0])
            for li, (W, b) in enumerate(members):
                if np.ndim(W) != 3 or np.ndim(b) != 2 or np.shape(W)[0] != P or np.shape(b)[0] != P:
                    raise ValueError(f"stacked layer {li}: W must be [{P}, out, in] and b [{P}, out], got "
                                     f"{tuple(np.shape(W))} / {tuple(np.shape(b))}")
            if P < 1:
                raise ValueError("a population has at least one member")
            return [[(W[m], b[m]) for W, b in members] for m in range(P)]
        out = []
        for m in members:
            out.append(PolicyController.module_layers(m, max_hidden) if isinstance(m, torch.nn.Module) else list(m))
        return out

    # -- the weights -----------------------------------------------------------------
    def member(self, m):
        """Member m as an ordinary PolicyController whose weights (and value head) are VIEWS of row m of this
        population's tensors, with the population's current explore, sample, temperature and seed: for equivalence
        tests, and for promoting a winner (clone its weights to keep them past the next load)."""
        return self._member(self._index(m))

    def load_member(self, m, net, value_head=None):
        """Copy new weights for member m alone (layers or an nn.Sequential of the population's shape; value_head as
        PolicyController.load_weights) in place, on the current stream, without synchronising."""
        self.member(m).load_weights(net, value_head=value_head)

    def load_weights(self, members, value_heads=None):
        """Copy new weights for EVERY member (any form the constructor takes, P unchanged) in place, on the current
        stream, without synchronising.  Stacked tensors take one copy per tensor, whatever P is.  A generation that is
        refused leaves `weights` and `value_heads` as they were."""
        stacked = not isinstance(members, torch.nn.Sequential) and self._stacked(list(members))
        if stacked:
            members = list(members)
            shapes = [tuple(np.shape(W))[1:] for W, _ in members]
            if shapes != self.shapes or any(np.shape(W)[0] != self.n_members or
                                            tuple(np.shape(b)) != (self.n_members, sh[0])
                                            for (W, b), sh in zip(members, shapes)):
                raise ValueError(f"stacked layer shapes {[tuple(np.shape(W)) for W, _ in members]}, this population "
                                 f"has {self.n_members} x {self.shapes}")
            tensors = [t for layer in members for t in layer]
        else:
            tensors = self._member_layers(members, self._row.limits[0])
            if len(tensors) != self.n_members:
                raise ValueError(f"{len(tensors)} members, this population has {self.n_members}")
        heads = self._load_heads(value_heads)
        for m in range(self.n_members):                                    # member by member: its layers, then its head
            if not stacked:
                tensors[m] = [t for layer in self._proto._layers(tensors[m]) for t in layer]
            if heads is not None:
                heads[m] = self._proto._head_parts(heads[m])
        self._copy(tensors, stacked, heads)

    # -- the C ABI ---------------------------------------------------------------------
    def bound(self, env=None):
        """abr_policy / abr_policy_mx over member 0's blob with ONE member's byte count (the population entries' rule)."""
        self._check_cover(self._proto._env(env))
        return self._proto._struct(self.weights.data_ptr(), self.weights.shape[1] * 4, self._proto.norm)

    def entries(self, val, want_probs):
        """As PolicyController.entries: one pair per engine, every mode (abr_policy_pop before smp)."""
        return self._row.pop, (self.population(), self.sampling(), val), 2


class RecurrentPolicyPopulation(_Population):
    """P recurrent policies of ONE shape over `player`, each deciding for its own group of lanes in the same launch
    (include/abr_env.h: abr_policy_pop over abr_policy_gru / abr_policy_gru_mx): local lane i belongs to member
    i // group, group is a positive multiple of 256, and P == ceil(n_lanes / group) -- the last member may own fewer
    lanes.  For every lane of member m every output and the committed column of `hidden` are bit for bit what a
    RecurrentPolicyController over member_parts(m) gives on that lane.

        pop = RecurrentPolicyPopulation(EnvPlayer(env), [(cell_m, head_m) for m in range(P)], group=env.n_lanes // P)
        out = env.step_policy(pop, 48, want_obs=False, want_actions=False)
        fitness = led.per_member(pop.group, pop.n_members)["qoe"]           # led = env.set_episode_ledger(rows)
        pop.load_weights(next_generation)                                    # in place, no sync; hidden is left alone

    members: a non-empty list of (cell, head) pairs, each what RecurrentPolicyController takes (an nn.GRUCell or
    (W_ih, W_hh, b_ih, b_hh); an nn.Linear or (W, b)), or the six stacked tensors (W_ih [P, 3H, F], W_hh [P, 3H, H],
    b_ih [P, 3H], b_hh [P, 3H], W [P, M, H], b [P, M]).  value_heads: None, a list of P heads (nn.Linear(H, 1) or
    (Wv, bv)), or the stacked pair (Wv [P, H], bv [P]).  Every other argument is RecurrentPolicyController's and is shared
    by all members, with the same H limit per engine; explore, sample, temperature and seed can be changed between
    launches.  It owns weights float32 [P, words] (row m is pack_gru of member m), hidden float32 [H, N] -- ONE slab,
    members own disjoint columns, zeros at construction -- and value_heads float32 [P, H + 1] (or None).

    Not covered: ShardedABREnv, LSTM cells and stacked cells; per-member exploration, temperature or norm."""

    method = "policy_gru_population"
    _commit = True

    def __init__(self, player, members, group, window=8, norm="default", explore=0.0, seed=0, sample="argmax",
                 temperature=1.0, value_heads=None, engine="lane", device=None):
        _gru_engine(engine)
        super().__init__(player, group, engine)
        if type(getattr(player, "env", None)).__name__ == "ShardedABREnv":
            raise ValueError("RecurrentPolicyPopulation does not run on a ShardedABREnv: the hidden state is one slab of "
                             "one environment's lanes")
        pairs = self._member_pairs(members)
        self.n_members = len(pairs)
        heads = self._member_heads(value_heads, self.n_members)
        # member 0 through the controller's own checks: shape, H, window, norm, explore, sample, temperature, head
        self._adopt(RecurrentPolicyController(player, pairs[0][0], pairs[0][1], window=window, norm=norm, explore=explore,
                                              seed=seed, sample=sample, temperature=temperature,
                                              value_head=heads[0] if heads is not None else None, device=device,
                                              engine=engine), heads is not None)
        self.n_lanes, self.hidden_size, self.hidden = self._proto.n_lanes, self._proto.hidden_size, self._proto.hidden
        self.load_weights(members, value_heads=value_heads)                 # every member has member 0's shape

    # -- the members' inputs -------------------------------------------------------
    @staticmethod
    def _stacked(members):
        return (not isinstance(members, torch.nn.Module) and len(members) == 6 and
                all(_is_array(t) for t in members) and np.ndim(members[0]) == 3)

    @classmethod
    def _member_pairs(cls, members):
        """A list of P (cell, head) pairs from either form; ValueError for anything else."""
        if isinstance(members, torch.nn.Module) or not isinstance(members, (list, tuple)) or len(members) == 0:
            raise ValueError("members is a non-empty list of (cell, head) pairs, or the six stacked tensors")
        if cls._stacked(members):
            P = int(np.shape(members[0])[0])
            if P < 1:
                raise ValueError("a population has at least one member")
            want = (3, 3, 2, 2, 3, 2)
            if any(np.ndim(t) != d or np.shape(t)[0] != P for t, d in zip(members, want)):
                raise ValueError(f"stacked members: W_ih [{P}, 3H, F], W_hh [{P}, 3H, H], b_ih [{P}, 3H], b_hh [{P}, 3H], "
                                 f"W [{P}, M, H], b [{P}, M]; got {[tuple(np.shape(t)) for t in members]}")
            return [(tuple(t[m] for t in members[:4]), tuple(t[m] for t in members[4:])) for m in range(P)]
        out = []
        for k, pair in enumerate(members):
            try:
                cell, head = pair
            except (TypeError, ValueError):
                raise ValueError(f"member {k} is not a (cell, head) pair") from None
            out.append((cell, head))
        return out

    # -- the weights -----------------------------------------------------------------
    def member_parts(self, m):
        """(cell, head) of member m -- (W_ih, W_hh, b_ih, b_hh), (W, b) -- as VIEWS of row m of `weights`: what a
        RecurrentPolicyController on another environment takes (it copies them)."""
        row = self.weights[self._index(m)]
        F, H, M = self.feature_dim, self.hidden_size, self.n_rates
        out, o = [], 0
        for shape in ((3 * H, F), (3 * H, H), (3 * H,), (3 * H,), (M, H), (M,)):
            n = int(np.prod(shape))
            out.append(row[o:o + n].view(*shape))
            o += n
        assert o == row.numel()
        return tuple(out[:4]), tuple(out[4:])

    def load_member(self, m, cell, head, value_head=None):
        """Copy new weights for member m alone (as RecurrentPolicyController.load_weights) in place, on the current
        stream, without synchronising.  `hidden` is not touched."""
        self._member(self._index(m)).load_weights(cell, head, value_head=value_head)

    def load_weights(self, members, value_heads=None):
        """Copy new weights for EVERY member (either form the constructor takes, P unchanged) in place, on the current
        stream, without synchronising.  Stacked tensors take one copy per tensor, whatever P is.  `hidden` is not
        touched, and a generation that is refused leaves `weights` and `value_heads` as they were."""
        pairs = self._member_pairs(members)
        if len(pairs) != self.n_members:
            raise ValueError(f"{len(pairs)} members, this population has {self.n_members}")
        heads = self._load_heads(value_heads)
        parts = [self._proto._parts(cell, head) for cell, head in pairs]    # every shape, before anything is copied
        if heads is not None:
            heads = [self._proto._head_parts(h) for h in heads]
        stacked = self._stacked(members)
        self._copy(members if stacked else parts, stacked, heads)

    def reset_hidden(self, mask=None):
        """Zero the hidden state of every lane, or of the lanes where mask (bool [N]) is set, whatever member owns them.
        A new episode needs no call: a lane's first decision starts from zeros by the contract."""
        self._proto.reset_hidden(mask)

    # -- the C ABI ---------------------------------------------------------------------
    def bound(self, env=None):
        """abr_policy_gru / abr_policy_gru_mx over member 0's blob with ONE member's byte count and the whole slab (the
        population entries' rule)."""
        env = self._proto._env(env)
        if int(env.n_lanes) != self.n_lanes:
            raise ValueError(f"the hidden state is for {self.n_lanes} lanes, the environment has {env.n_lanes}")
        self._check_cover(env)
        return self._proto._struct(self.weights.data_ptr(), self.weights.shape[1] * 4, self._proto.norm,
                                   self.hidden.data_ptr(), self.hidden.numel() * 4)

    # -- decisions ---------------------------------------------------------------------
    def select(self, want_features=True, want_scores=True, want_probs=False, want_value=False, want_hidden=False,
               commit=False):
        """One decision per lane on the environment's current state, every lane by its own member: the same dict, and the
        same commit rule, as RecurrentPolicyController.select."""
        return _select(self, want_features, want_scores, want_probs, want_value, want_hidden, commit)

    def entries(self, val, want_probs):
        """As RecurrentPolicyController.entries: one pair per engine, every mode (abr_policy_pop before smp)."""
        return self._row.pop, (self.population(), self.sampling(), val), 3
