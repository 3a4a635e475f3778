"""Policy populations without a GPU (include/abr_env.h: abr_policy_pop): the ABI struct, the four symbols and every
refusal before the handle; the member mapping the kernels use (csrc/abr_lane_jump.h: pop_member and the offsets)
compiled for the host; PolicyPopulation's weight packing, views and lane arithmetic on device="cpu"; and
EpisodeLedger.per_member on a hand-filled ledger."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from helpers import c_abi_output, native_harness
from ledger_twin import FLOATS
from test_episode_ledger_cpu import W as QOE_W
from test_episode_ledger_cpu import cpu_ledger, episode_ends
from test_policy_cpu import _layers

ENTRIES = ("abr_env_policy_select_pop", "abr_env_step_policy_pop", "abr_env_policy_select_mx_pop",
           "abr_env_step_policy_mx_pop")


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(scope="module")
def PH():
    h = native_harness("policy_population_harness")
    for f in (h.pp_member, h.pp_blob_offset, h.pp_head_offset):
        f.restype, f.argtypes = C.c_int64, [C.c_int64, C.c_int32]
    h.pp_lane.restype, h.pp_lane.argtypes = None, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    return h


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def test_struct_layout_and_symbols(L):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %d\n", sizeof(abr_policy_pop), offsetof(abr_policy_pop, n_members),
         offsetof(abr_policy_pop, group), offsetof(abr_policy_pop, reserved_), ABR_ABI_VERSION);
  return 0;
}'''
    got = list(map(int, c_abi_output(prog)[0].split()))
    S = L.PolicyPop
    assert got[:4] == [C.sizeof(S), S.n_members.offset, S.group.offset, S.reserved_.offset] == [32, 0, 4, 8]
    assert got[4] == 4 == L.ABI_VERSION == L.lib().abr_abi_version()
    names = [s[0] for s in L.SYMBOLS]
    for sym in ENTRIES:
        assert sym in names and hasattr(L.lib(), sym)


def _pop(L, P=4, group=256, reserved=None):
    p = L.PolicyPop()
    p.n_members, p.group = P, group
    if reserved is not None:
        p.reserved_[reserved] = 1
    return p


def _pols(L):
    lane, mx = L.Policy(), L.PolicyMx()
    for p, w in ((lane, (64, 64)), (mx, (128, 128))):
        p.window, p.n_hidden, p.weights_dev, p.weights_bytes, p.seed = 8, 2, 4096, 100, 1
        p.width[0], p.width[1] = w
    return lane, mx


def _calls(L):
    """(select, step) callables per engine: f(env, pol, pop, smp, val, ...)."""
    lib = L.lib()
    lane, mx = _pols(L)
    out = []
    for pol, sel, stp in ((lane, lib.abr_env_policy_select_pop, lib.abr_env_step_policy_pop),
                          (mx, lib.abr_env_policy_select_mx_pop, lib.abr_env_step_policy_mx_pop)):
        def select(pop, smp, val, probs=None, value=None, pol=pol, sel=sel):
            return sel(None, C.byref(pol) if pol is not None else None, pop, smp, val, C.c_void_p(8192), None, None,
                       probs, value, None)

        def step(pop, smp, val, n=4, probs=None, values=None, last=None, pol=pol, stp=stp):
            return stp(None, C.byref(pol) if pol is not None else None, pop, smp, val, n, None, None, None, None, None,
                       None, probs, values, last, None)
        out.append((select, step))
    return out


def test_every_refusal_before_the_handle(L):
    lib = L.lib()
    err = lib.abr_last_error
    smp = L.PolicySampling()
    smp.mode, smp.inv_temperature = L.POLICY_SOFTMAX, 1.0
    val = L.PolicyValue()
    val.head_dev, val.head_bytes = 4096, 4 * 65
    S, Vv, ptr = C.byref(smp), C.byref(val), C.c_void_p(8192)
    ok = C.byref(_pop(L))
    for select, step in _calls(L):
        # pop itself: NULL, P = 0 (and below), the groups, a reserved field, the overflow
        assert select(None, None, None) == -1 and b"population is NULL" in err()
        assert step(None, S, Vv) == -1 and b"population is NULL" in err()
        for P in (0, -1):
            assert select(C.byref(_pop(L, P=P)), None, None) == -1 and b"n_members" in err()
            assert step(C.byref(_pop(L, P=P)), None, None) == -1 and b"n_members" in err()
        for group in (0, 255, 257, 384, -256):
            assert select(C.byref(_pop(L, group=group)), None, None) == -1 and b"group" in err(), group
            assert step(C.byref(_pop(L, group=group)), S, Vv) == -1 and b"group" in err(), group
        for r in (0, 5):
            assert select(C.byref(_pop(L, reserved=r)), None, None) == -1 and b"population reserved_" in err()
            assert step(C.byref(_pop(L, reserved=r)), None, None) == -1 and b"population reserved_" in err()
        big = C.byref(_pop(L, P=2 ** 31 - 1, group=2 ** 31 - 256))
        assert select(big, None, None) == -1 and b"overflows" in err()
        assert step(big, None, None) == -1 and b"overflows" in err()
        # pol, smp and val are looked at before pop; n_steps after it
        bad = L.PolicySampling()
        bad.mode, bad.inv_temperature = 2, 1.0
        assert step(None, C.byref(bad), None) == -1 and b"sampling" in err()
        bv = L.PolicyValue()
        bv.head_dev, bv.head_bytes = 4098, 4 * 65
        assert step(None, None, C.byref(bv)) == -1 and b"value head" in err()
        for n in (0, -1):
            assert step(ok, None, None, n=n) == -1 and b"n_steps" in err()
            assert step(None, None, None, n=n) == -1 and b"population is NULL" in err()
        # outputs that need a struct that is absent
        assert select(ok, None, None, probs=ptr) == -1 and b"probs need" in err()
        assert step(ok, None, Vv, probs=ptr) == -1 and b"probs need" in err()
        assert select(ok, S, None, value=ptr) == -1 and b"values need" in err()
        assert step(ok, S, None, values=ptr) == -1 and b"values need" in err()
        assert step(ok, None, None, last=ptr) == -1 and b"values need" in err()
        # valid structs reach the handle in every mode
        for s_, v_, kw in ((None, None, {}), (S, None, dict(probs=ptr)), (None, Vv, dict(values=ptr, last=ptr)),
                           (S, Vv, dict(probs=ptr, values=ptr, last=ptr))):
            assert step(ok, s_, v_, n=1, **kw) == -1 and b"env is NULL" in err()
            assert select(ok, s_, v_) == -1 and b"NULL argument" in err()
        for P, group in ((1, 256), (2 ** 31 - 1, 256), (1, 2 ** 31 - 256)):
            assert step(C.byref(_pop(L, P=P, group=group)), None, None, n=1) == -1 and b"env is NULL" in err()
    # a NULL policy comes first of all
    assert lib.abr_env_step_policy_pop(None, None, None, None, None, 0, *([None] * 10)) == -1 and b"policy is NULL" in err()
    assert lib.abr_env_policy_select_mx_pop(None, None, None, None, None, *([None] * 6)) == -1 and b"policy is NULL" in err()


# ---------------------------------------------------------------------------------------------------------------------
# the member mapping the kernels compile

@pytest.mark.parametrize("group", (256, 512, 1024))
def test_member_of_every_lane_and_its_offsets(PH, group):
    words, head = 5574, 65
    out = (C.c_int64 * 3)()
    for i in range(4 * group + 1):
        PH.pp_lane(i, group, words, head, out)
        assert list(out) == [i // group, (i // group) * words, (i // group) * head], i
    for first in range(0, 4 * group + 1, 256):                             # a block's first and last lane: one member
        assert PH.pp_member(first, group) == (first + 255) // group == first // group
    # no 32-bit wrap: the last member of the largest population of the widest blob
    assert PH.pp_member((2 ** 32 - 2) * 256, 256) == 2 ** 32 - 2
    assert PH.pp_blob_offset(2 ** 31 - 2, 39824) == (2 ** 31 - 2) * 39824
    assert PH.pp_head_offset(2 ** 31 - 2, 129) == (2 ** 31 - 2) * 129


# ---------------------------------------------------------------------------------------------------------------------
# PolicyPopulation on the CPU

class _Player:
    def __init__(self, n_lanes):
        self.env = types.SimpleNamespace(n_lanes=n_lanes, n_rates=6, device=torch.device("cpu"))

    def get_mpd(self):
        from abrsimulator_amd.datamodel import MPD, Chunk
        return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))


def _net(layers):
    nn = torch.nn
    mods = []
    for k, (Wt, b) in enumerate(layers):
        lin = nn.Linear(Wt.shape[1], Wt.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(Wt))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([nn.ReLU()] if k < len(layers) - 1 else [])
    return nn.Sequential(*mods)


@pytest.mark.parametrize("engine,hidden", (("lane", []), ("lane", [64, 64]), ("matrix", [128, 33, 7])))
def test_weights_rows_views_and_loads(L, engine, hidden):
    import abrsimulator_amd as A
    from abrsimulator_amd.policy import pack_layers
    rng = np.random.default_rng(3)
    P, group, Wn, M = 3, 256, 8, 6
    F, vin = 4 + Wn + M, (hidden[-1] if hidden else 4 + Wn + M)
    members = [_layers(rng, F, list(hidden), M, special=(m == 1)) for m in range(P)]
    heads = [(rng.normal(0, 1, vin).astype(np.float32), np.float32(rng.normal())) for _ in range(P)]
    stacked = [(np.stack([mem[l][0] for mem in members]), np.stack([mem[l][1] for mem in members]))
               for l in range(len(hidden) + 1)]
    shead = (np.stack([h[0] for h in heads]), np.array([h[1] for h in heads], np.float32))
    want = np.stack([pack_layers(m) for m in members])
    want_h = np.stack([np.append(h[0], h[1]).astype(np.float32) for h in heads])
    player = _Player(700)
    kw = dict(window=Wn, engine=engine, device="cpu")
    pops = [A.PolicyPopulation(player, members, group, value_heads=heads, **kw),
            A.PolicyPopulation.from_modules(player, [_net(m) for m in members], group, value_heads=heads, **kw),
            A.PolicyPopulation(player, stacked, group, value_heads=shead, **kw),
            A.PolicyPopulation(player, [(torch.from_numpy(Wt), torch.from_numpy(b)) for Wt, b in stacked], group,
                               value_heads=tuple(map(torch.from_numpy, shead)), **kw)]
    for pop in pops:
        assert pop.n_members == P and pop.weights.shape == want.shape and pop.weights.dtype == torch.float32
        assert pop.weights.numpy().tobytes() == want.tobytes()              # NaN payloads and -0 included
        assert pop.value_heads.numpy().tobytes() == want_h.tobytes()
        assert pop.bound().weights_bytes == 4 * want.shape[1] and pop.bound().weights_dev == pop.weights.data_ptr()
        assert pop.value().head_bytes == 4 * (vin + 1) and pop.value().head_dev == pop.value_heads.data_ptr()
        assert (pop.population().n_members, pop.population().group) == (P, group)
        assert type(pop.bound()) is (L.PolicyMx if engine == "matrix" else L.Policy)
    pop = pops[0]
    # member(m) is an ordinary controller over row m, as a view
    for m in range(P):
        c = pop.member(m)
        assert type(c) is A.PolicyController and c.engine == engine and c.shapes == pop.shapes
        assert c.weights.data_ptr() == pop.weights[m].data_ptr() and c.weights.shape == (want.shape[1],)
        assert c.value_head.data_ptr() == pop.value_heads[m].data_ptr()
        assert c.bound(player.env).weights_bytes == 4 * want.shape[1]
        for (Wt, b), (Wm, bm) in zip(c.layers(), members[m]):
            assert Wt.numpy().tobytes() == Wm.tobytes() and b.numpy().tobytes() == bm.tobytes()
    pop.member(2).weights[0] = 7.0
    assert pop.weights[2, 0] == 7.0
    # load_member touches only row m (and only that head)
    before, before_h = pop.weights.clone(), pop.value_heads.clone()
    fresh, fresh_h = _layers(rng, F, list(hidden), M), (rng.normal(0, 1, vin).astype(np.float32), np.float32(0.25))
    pop.load_member(1, fresh, value_head=fresh_h)
    assert pop.weights[1].numpy().tobytes() == pack_layers(fresh).tobytes()
    assert pop.value_heads[1].numpy().tobytes() == np.append(fresh_h[0], fresh_h[1]).astype(np.float32).tobytes()
    for m in (0, 2):
        assert torch.equal(pop.weights[m], before[m]) and torch.equal(pop.value_heads[m], before_h[m])
    pop.load_member(0, _net(fresh))
    assert pop.weights[0].numpy().tobytes() == pack_layers(fresh).tobytes() and torch.equal(pop.value_heads[0], before_h[0])
    # load_weights: every member, in place
    ptr = pop.weights.data_ptr()
    for form, hform in ((members, heads), (stacked, shead), ([_net(m) for m in members], None)):
        pop.weights.zero_()
        pop.load_weights(form, value_heads=hform)
        assert pop.weights.data_ptr() == ptr and pop.weights.numpy().tobytes() == want.tobytes()
        assert pop.value_heads.numpy().tobytes() == want_h.tobytes()
    # settings are shared and checked as the controller checks them
    pop.explore, pop.sample, pop.temperature = 0.25, "softmax", 0.5
    c = pop.member(1)
    assert (c.explore, c.sample, c.temperature, c.explore_threshold) == (0.25, "softmax", 0.5, 1 << 30)
    assert pop.sampling().mode == L.POLICY_SOFTMAX and pop.sampling().inv_temperature == 2.0
    for attr, v in (("explore", 1.5), ("sample", "greedy"), ("temperature", 0.0)):
        with pytest.raises(ValueError):
            setattr(pop, attr, v)


def test_lane_arithmetic():
    import abrsimulator_amd as A
    rng = np.random.default_rng(4)
    for N, group in ((256, 256), (257, 256), (700, 256), (1024, 256), (1000, 512)):
        P = -(-N // group)
        pop = A.PolicyPopulation(_Player(N), [_layers(rng, 18, [5], 6) for _ in range(P)], group, device="cpu")
        mol = pop.member_of_lane()
        assert mol.dtype == torch.int32 and mol.shape == (N,)
        assert mol.tolist() == [i // group for i in range(N)]
        seen = []
        for m in range(P):
            sl = pop.lanes_of(m)
            assert isinstance(sl, slice) and (mol[sl] == m).all() and sl.stop - sl.start == int((mol == m).sum())
            seen += list(range(N))[sl]
        assert seen == list(range(N))
        for bad in (-1, P, 1.5, True):
            with pytest.raises(IndexError):
                pop.lanes_of(bad)


def test_refusals():
    import abrsimulator_amd as A
    rng = np.random.default_rng(5)
    mk = lambda hidden=(5,), F=18, M=6: _layers(rng, F, list(hidden), M)
    ok = [mk(), mk(), mk()]
    A.PolicyPopulation(_Player(700), ok, 256, device="cpu")
    for group in (0, 255, 257, 384, -256, 256.5, True, None):             # the group
        with pytest.raises((ValueError, TypeError)):
            A.PolicyPopulation(_Player(700), ok, group, device="cpu")
    for N in (512, 769, 1024):                                           # P is not ceil(N / group)
        with pytest.raises(ValueError, match="members"):
            A.PolicyPopulation(_Player(N), ok, 256, device="cpu")
    with pytest.raises(ValueError):                                       # one shape
        A.PolicyPopulation(_Player(700), [mk(), mk((6,)), mk()], 256, device="cpu")
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), [mk(), mk((5, 5)), mk()], 256, device="cpu")
    with pytest.raises(ValueError):                                       # the controller's own limits, per engine
        A.PolicyPopulation(_Player(700), [mk((65,)) for _ in range(3)], 256, device="cpu")
    A.PolicyPopulation(_Player(700), [mk((65,)) for _ in range(3)], 256, device="cpu", engine="matrix")
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), [mk((129,)) for _ in range(3)], 256, device="cpu", engine="matrix")
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), ok, 256, device="cpu", engine="tensor")
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), [], 256, device="cpu")
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), [mk(F=19) for _ in range(3)], 256, device="cpu")
    for kw in (dict(explore=1.5), dict(sample="greedy"), dict(temperature=0.0), dict(window=17), dict(norm="other")):
        with pytest.raises(ValueError):
            A.PolicyPopulation(_Player(700), ok, 256, device="cpu", **kw)
    head = lambda: (rng.normal(0, 1, 5).astype(np.float32), np.float32(0.5))
    with pytest.raises(ValueError):                                       # heads: one per member, of the shape
        A.PolicyPopulation(_Player(700), ok, 256, device="cpu", value_heads=[head(), head()])
    with pytest.raises(ValueError):
        A.PolicyPopulation(_Player(700), ok, 256, device="cpu",
                           value_heads=[head(), (np.zeros(6, np.float32), np.float32(0)), head()])
    pop = A.PolicyPopulation(_Player(700), ok, 256, device="cpu")
    with pytest.raises(ValueError, match="value heads"):
        pop.value()
    with pytest.raises(ValueError):
        pop.load_weights(ok, value_heads=[head(), head(), head()])
    with pytest.raises(ValueError):
        pop.load_weights(ok[:2])
    with pytest.raises(ValueError):
        pop.load_member(0, mk((6,)))
    with pytest.raises(IndexError):
        pop.load_member(3, mk())
    with pytest.raises(ValueError):                                       # another environment: P no longer fits
        pop.bound(types.SimpleNamespace(n_lanes=1024, n_rates=6))
    with pytest.raises(ValueError):
        pop.bound(types.SimpleNamespace(n_lanes=700, n_rates=5))


REFUSED_LOADS = ("stacked, bv of the wrong length", "stacked, Wv of the wrong width", "list, last member's hidden width",
                 "list, last member's head", "list of P - 1 members")


@pytest.mark.parametrize("case", REFUSED_LOADS)
def test_a_refused_load_writes_nothing(case):
    """load_weights is all or nothing: a generation with a fault anywhere -- in the last member, or in the heads, which
    come after the weights -- raises ValueError and leaves weights and value_heads bit for bit as they were."""
    import abrsimulator_amd as A
    rng = np.random.default_rng(6)
    P, H = 3, 5
    mk = lambda hidden=H: _layers(rng, 18, [hidden], 6)
    head = lambda n=H: (rng.normal(0, 1, n).astype(np.float32), np.float32(rng.normal()))
    stack = lambda ms: [(np.stack([m[l][0] for m in ms]), np.stack([m[l][1] for m in ms])) for l in range(2)]
    hstack = lambda hs: (np.stack([h[0] for h in hs]), np.array([h[1] for h in hs], np.float32))
    pop = A.PolicyPopulation(_Player(700), [mk() for _ in range(P)], 256, value_heads=[head() for _ in range(P)],
                             device="cpu")
    new, heads = [mk() for _ in range(P)], [head() for _ in range(P)]
    Wv, bv = hstack(heads)
    members, value_heads = {
        REFUSED_LOADS[0]: (stack(new), (Wv, bv[:-1])),
        REFUSED_LOADS[1]: (stack(new), (np.concatenate([Wv, Wv[:, :1]], axis=1), bv)),
        REFUSED_LOADS[2]: (new[:-1] + [mk(H + 1)], heads),
        REFUSED_LOADS[3]: (new, heads[:-1] + [head(H + 1)]),
        REFUSED_LOADS[4]: (new[:-1], heads[:-1]),
    }[case]
    before, before_h = pop.weights.numpy().tobytes(), pop.value_heads.numpy().tobytes()
    with pytest.raises(ValueError):
        pop.load_weights(members, value_heads=value_heads)
    assert pop.weights.numpy().tobytes() == before and pop.value_heads.numpy().tobytes() == before_h
    pop.load_weights(new, value_heads=heads)                                # the same generation without the fault loads
    assert pop.weights.numpy().tobytes() != before and pop.value_heads.numpy().tobytes() != before_h


# ---------------------------------------------------------------------------------------------------------------------
# EpisodeLedger.per_member

def test_per_member_counts_are_exact_and_means_within_the_summation_bound():
    n, rows, group = 1000, 2, 256                                           # far more episodes per lane than rows
    P = -(-n // group)
    rng = np.random.default_rng(12)
    lanes = rng.integers(0, n, 6000)
    lanes = lanes[(lanes < 512) | (lanes >= 768)]                           # member 2 never finishes an episode
    lane, f, w = episode_ends(rng, n, 0, lanes)
    led, t = cpu_ledger(n, rows, lane, f, w)
    assert t.count.max() > rows                                             # the ring has dropped records
    pm = led.per_member(group, P)
    assert pm["count"].dtype == torch.int64 and pm["count"].shape == (P,)
    member = lane // group
    assert pm["count"].tolist() == [int((member == m).sum()) for m in range(P)]
    assert pm["count"].sum() == lane.size and pm["count"][2] == 0 and pm["count"][3] > 0
    assert pm["count"].tolist() == [int(t.count[m * group:(m + 1) * group].sum()) for m in range(P)]
    qoe = ((QOE_W[0] * f[:, 0] + QOE_W[1] * f[:, 3]) + QOE_W[2] * f[:, 1]) + QOE_W[3] * f[:, 2]
    terms = dict(zip(FLOATS, [f[:, 0], f[:, 1], f[:, 2], f[:, 3], qoe]))
    u = 2.0 ** -53
    for k in FLOATS:
        assert pm[k].dtype == torch.float64 and not torch.isnan(pm[k]).any()
        assert float(pm[k][2]) == 0.0
        for m in (0, 1, 3):
            x = terms[k][member == m]
            cnt = x.size
            # as per_trace: a float64 sum of cnt terms in any order, then the division and the multiplication undoing it
            bound = cnt * u * math.fsum(np.abs(x)) / (1 - cnt * u)
            exact = math.fsum(x)
            assert abs(float(pm[k][m]) * cnt - exact) <= bound + 2 * u * abs(exact), (k, m)
    for group_, P_ in ((256, 3), (256, 5), (0, 4), (512, 4)):
        with pytest.raises(ValueError):
            led.per_member(group_, P_)
    assert led.per_member(512, 2)["count"].tolist() == [int((lane // 512 == m).sum()) for m in range(2)]
