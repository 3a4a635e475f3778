"""Recurrent policy populations without a GPU (include/abr_env.h: abr_policy_pop over abr_policy_gru and
abr_policy_gru_mx): the four symbols; every refusal before the handle, in the documented order, with the message the
single-network GRU entries and the MLP population entries give for the same mistake; the member mapping the POP
instances compile (csrc/abr_lane_jump.h: pop_member and the offsets) with the GRU blob's word count, compiled for the
host; and RecurrentPolicyPopulation's packing, views, lane arithmetic and refusals on device="cpu"."""
import ctypes as C
import re
import types

import numpy as np
import pytest
import torch

from helpers import native_harness

f32 = np.float32
E_INVALID = -1
ENTRIES = ("abr_env_gru_select_pop", "abr_env_gru_step_pop", "abr_env_gru_mx_select_pop",
           "abr_env_gru_mx_step_pop")
W, M = 8, 6
F = 4 + W + M


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


@pytest.fixture(scope="module")
def PH():
    h = native_harness("policy_gru_population_harness")
    for f in (h.pgp_member, h.pgp_blob_offset, h.pgp_head_offset):
        f.restype, f.argtypes = C.c_int64, [C.c_int64, C.c_int32]
    h.pgp_blob_words.restype, h.pgp_blob_words.argtypes = C.c_int64, [C.c_int32] * 3
    h.pgp_head_words.restype, h.pgp_head_words.argtypes = C.c_int64, [C.c_int32]
    h.pgp_lane.restype, h.pgp_lane.argtypes = None, [C.c_int64] + [C.c_int32] * 4 + [C.POINTER(C.c_int64)]
    return h


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def test_symbols_are_declared_exported_and_bound(L):
    import os
    header = open(os.path.join(os.path.dirname(L.CSRC), "..", "include", "abr_env.h")).read()
    names = [s[0] for s in L.SYMBOLS]
    singles = dict(zip(ENTRIES, ("abr_env_policy_select_gru", "abr_env_step_policy_gru", "abr_env_gru_mx_select",
                                 "abr_env_gru_mx_step")))
    for sym in ENTRIES:
        assert re.search(r"^int %s\(abr_env \*env, const abr_policy_gru(_mx)? \*pol, const abr_policy_pop \*pop," % sym,
                         header, re.M), sym
        assert sym in names and hasattr(L.lib(), sym)
        # the single-network entry's parameter list with the population struct after pol
        args, single = dict((s[0], s[2]) for s in L.SYMBOLS)[sym], dict((s[0], s[2]) for s in L.SYMBOLS)[singles[sym]]
        assert args[:2] == single[:2] and args[2] is C.POINTER(L.PolicyPop) and args[3:] == single[2:]
    assert L.lib().abr_abi_version() == 4 == L.ABI_VERSION
    assert "Not covered: populations" not in header


def _good(L, buf, mx):
    p = (L.PolicyGruMx if mx else L.PolicyGru)()
    p.window, p.hidden = 8, 32
    p.weights_dev = p.state_dev = C.addressof(buf)
    p.weights_bytes = p.state_bytes = 4
    return p


def _pop(L, P=4, group=256, reserved=None):
    p = L.PolicyPop()
    p.n_members, p.group = P, group
    if reserved is not None:
        p.reserved_[reserved] = 1
    return p


def _ref(x):
    return C.byref(x) if x is not None else None


def test_every_refusal_before_the_handle_in_order_with_the_existing_messages(L):
    lib = L.lib()
    buf = (C.c_double * 4)()
    base = C.addressof(buf)
    msg = lambda: lib.abr_last_error().decode()

    def smp(mode=0, it=1.0, r=0):
        s = L.PolicySampling()
        s.mode, s.inv_temperature = mode, it
        s.reserved_[2] = r
        return s

    def val(head=base, r=0):
        v = L.PolicyValue()
        v.head_dev, v.head_bytes = head, 132
        v.reserved_[1] = r
        return v

    # the MLP population entries: the yardstick for the messages about pop itself
    mlp = L.Policy()
    mlp.window, mlp.n_hidden, mlp.weights_dev, mlp.weights_bytes = 8, 0, base, 4

    def mlp_pop_message(pp):
        assert lib.abr_env_step_policy_pop(None, C.byref(mlp), _ref(pp), None, None, 1, *([None] * 10)) == E_INVALID
        return msg()

    for mx in (False, True):
        sel_pop, stp_pop = ((lib.abr_env_gru_mx_select_pop, lib.abr_env_gru_mx_step_pop) if mx else
                            (lib.abr_env_gru_select_pop, lib.abr_env_gru_step_pop))
        sel_one, stp_one = ((lib.abr_env_gru_mx_select, lib.abr_env_gru_mx_step) if mx else
                            (lib.abr_env_policy_select_gru, lib.abr_env_step_policy_gru))

        def select(p, pp, s=None, v=None, probs=None, value=None):
            return sel_pop(None, _ref(p), _ref(pp), _ref(s), _ref(v), 0, base, None, None, probs, value, None, None)

        def step(p, pp, s=None, v=None, n=1, probs=None, values=None, last=None):
            return stp_pop(None, _ref(p), _ref(pp), _ref(s), _ref(v), n, None, None, None, None, None, None, probs, values,
                           last, None, None)

        def select1(p, s=None, v=None, probs=None, value=None):
            return sel_one(None, _ref(p), _ref(s), _ref(v), 0, base, None, None, probs, value, None, None)

        def step1(p, s=None, v=None, n=1, probs=None, values=None, last=None):
            return stp_one(None, _ref(p), _ref(s), _ref(v), n, None, None, None, None, None, None, probs, values, last,
                           None, None)

        good, ok = (lambda: _good(L, buf, mx)), _pop(L)
        # a good call reaches the handle, in every mode
        for s_, v_, kw in ((None, None, {}), (smp(1, 0.5), None, dict(probs=base)), (None, val(), dict(values=base, last=base)),
                           (smp(), val(), dict(probs=base, values=base, last=base))):
            assert step(good(), ok, s_, v_, **kw) == E_INVALID and msg() == "env is NULL"
            assert select(good(), ok, s_, v_) == E_INVALID and "NULL argument" in msg()

        # 1. everything the single-network entry checks before the handle comes BEFORE pop: with a NULL (or bad) pop the
        #    message is the single-network entry's own, word for word
        cases = []
        for field, value in (("window", -1), ("window", 17), ("hidden", 0), ("hidden", 129 if mx else 65),
                             ("weights_dev", None), ("weights_dev", base + 2), ("norm_dev", base + 4), ("state_dev", None),
                             ("state_dev", base + 1), ("explore_threshold", (1 << 32) + 1)):
            p = good()
            setattr(p, field, value)
            cases.append(dict(p=p))
        p = good()
        p.reserved_[3] = 1
        cases.append(dict(p=p))
        cases.append(dict(p=None))
        for s in (smp(mode=2), smp(it=0.0), smp(it=float("inf")), smp(it=float("nan")), smp(r=1)):
            cases.append(dict(p=good(), s=s))
        for v in (val(head=None), val(head=base + 2), val(r=1)):
            cases.append(dict(p=good(), v=v))
        for kw in cases:
            for bad_pop in (None, _pop(L, group=255)):
                assert select1(**kw) == E_INVALID
                want = msg()
                assert "env" not in want and "population" not in want
                assert select(kw["p"], bad_pop, kw.get("s"), kw.get("v")) == E_INVALID and msg() == want
                assert step1(**kw) == E_INVALID and msg() == want
                assert step(kw["p"], bad_pop, kw.get("s"), kw.get("v")) == E_INVALID and msg() == want
        # outputs that need a struct that is absent: also before pop
        assert select1(good(), probs=base) == E_INVALID and "probs need" in msg()
        want = msg()
        assert select(good(), None, probs=base) == E_INVALID and msg() == want
        assert step(good(), None, probs=base) == E_INVALID and msg() == want
        assert step1(good(), values=base) == E_INVALID and "values need" in msg()
        want = msg()
        assert select(good(), None, value=base) == E_INVALID and msg() == want
        assert step(good(), None, values=base) == E_INVALID and msg() == want
        assert step(good(), None, last=base) == E_INVALID and msg() == want

        # 2. pop itself, after val and before n_steps: the MLP population entries' messages
        bad_pops = [None, _pop(L, P=0), _pop(L, P=-1), _pop(L, group=0), _pop(L, group=255), _pop(L, group=257),
                    _pop(L, group=384), _pop(L, group=-256), _pop(L, reserved=0), _pop(L, reserved=5),
                    _pop(L, P=2 ** 31 - 1, group=2 ** 31 - 256)]
        words = ["population is NULL", "n_members", "n_members", "group", "group", "group", "group", "group",
                 "population reserved_", "population reserved_", "overflows"]
        for pp, word in zip(bad_pops, words):
            want = mlp_pop_message(pp)
            assert word in want
            for s_, v_ in ((None, None), (smp(1, 2.0), val())):
                assert select(good(), pp, s_, v_) == E_INVALID and msg() == want, word
                assert step(good(), pp, s_, v_) == E_INVALID and msg() == want, word
                assert step(good(), pp, s_, v_, n=0) == E_INVALID and msg() == want, word     # pop before n_steps

        # 3. n_steps after pop and before the handle
        for n in (0, -3):
            assert step1(good(), n=n) == E_INVALID and "n_steps" in msg()
            want = msg()
            assert step(good(), ok, n=n) == E_INVALID and msg() == want
        # the largest valid structs reach the handle
        for P, group in ((1, 256), (2 ** 31 - 1, 256), (1, 2 ** 31 - 256)):
            assert step(good(), _pop(L, P=P, group=group)) == E_INVALID and msg() == "env is NULL"


# ---------------------------------------------------------------------------------------------------------------------
# the member mapping the kernels compile

def _words(H, Fd=F, Md=M):
    return 3 * H * (Fd + H + 2) + Md * (H + 1)


@pytest.mark.parametrize("group", (256, 512, 1024))
def test_member_of_every_lane_and_its_offsets(PH, group):
    out = (C.c_int64 * 3)()
    for H in (1, 33, 64, 128):
        assert PH.pgp_blob_words(F, H, M) == _words(H) and PH.pgp_head_words(H) == H + 1
        for i in range(4 * group):
            PH.pgp_lane(i, group, F, H, M, out)
            assert list(out) == [i // group, (i // group) * _words(H), (i // group) * (H + 1)], (H, i)
    for first in range(0, 4 * group, 256):                                 # a block's first and last lane: one member
        assert PH.pgp_member(first, group) == (first + 255) // group == first // group
    # the blob sizes the issue quotes: 66 KB at H = 64, 230 KB at H = 128 (W = 8, 6 rates)
    assert 4 * _words(64) == 66072 and 4 * _words(128) == 230424


def test_offsets_past_2_to_the_32_words(PH):
    words = int(PH.pgp_blob_words(4 + 16 + 16, 128, 16))                    # the widest blob: 65 808 words
    assert words == _words(128, 36, 16) == 65808
    for m in (2 ** 16 + 1, 2 ** 20, 2 ** 31 - 2):
        assert m * words > 2 ** 32
        assert PH.pgp_blob_offset(m, words) == m * words
        assert PH.pgp_member(m * 256, 256) == m and PH.pgp_member(m * 1024 + 768, 1024) == m
    assert PH.pgp_head_offset(2 ** 31 - 2, 129) == (2 ** 31 - 2) * 129
    assert PH.pgp_member((2 ** 32 - 2) * 256, 256) == 2 ** 32 - 2


# ---------------------------------------------------------------------------------------------------------------------
# RecurrentPolicyPopulation on the CPU

class _Player:
    def __init__(self, n_lanes):
        self.env = types.SimpleNamespace(n_lanes=n_lanes, n_rates=M, device=torch.device("cpu"))

    def get_mpd(self):
        from abrsimulator_amd.datamodel import MPD, Chunk
        return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))


def _member(rng, H, special=False, Fd=F, Md=M):
    cell = tuple((rng.standard_normal(s) * 0.5).astype(f32) for s in ((3 * H, Fd), (3 * H, H), (3 * H,), (3 * H,)))
    head = tuple((rng.standard_normal(s) * 0.5).astype(f32) for s in ((Md, H), (Md,)))
    if special:
        cell[0][0, :5] = [np.nan, np.inf, -np.inf, -0.0, 1e-41]
        head[1][0] = f32(-0.0)
    return cell, head


def _modules(cell, head):
    H = cell[1].shape[1]
    c, h = torch.nn.GRUCell(cell[0].shape[1], H), torch.nn.Linear(H, head[0].shape[0])
    with torch.no_grad():
        for dst, src in zip((c.weight_ih, c.weight_hh, c.bias_ih, c.bias_hh, h.weight, h.bias), cell + head):
            dst.copy_(torch.from_numpy(src))
    return c, h


def _stack(members):
    return tuple(np.stack([(c + h)[k] for c, h in members]) for k in range(6))


@pytest.mark.parametrize("engine,H", (("lane", 1), ("lane", 64), ("matrix", 33), ("matrix", 128)))
def test_weights_rows_views_and_loads(L, engine, H):
    import abrsimulator_amd as A
    from abrsimulator_amd.policy import pack_gru
    rng = np.random.default_rng(3 + H)
    P, group, N = 3, 256, 700
    members = [_member(rng, H, special=(m == 1)) for m in range(P)]
    heads = [(rng.standard_normal(H).astype(f32), f32(rng.standard_normal())) for _ in range(P)]
    shead = (np.stack([h[0] for h in heads]), np.array([h[1] for h in heads], f32))
    want = np.stack([pack_gru(c, h) for c, h in members])
    want_h = np.stack([np.append(h[0], h[1]).astype(f32) for h in heads])
    assert want.shape == (P, _words(H))
    player = _Player(N)
    kw = dict(window=W, engine=engine, device="cpu")
    pops = [A.RecurrentPolicyPopulation(player, members, group, value_heads=heads, **kw),
            A.RecurrentPolicyPopulation(player, [_modules(c, h) for c, h in members], group, value_heads=heads, **kw),
            A.RecurrentPolicyPopulation(player, _stack(members), group, value_heads=shead, **kw),
            A.RecurrentPolicyPopulation(player, tuple(map(torch.from_numpy, _stack(members))), group,
                                        value_heads=tuple(map(torch.from_numpy, shead)), **kw)]
    for pop in pops:
        assert pop.n_members == P and pop.weights.shape == want.shape and pop.weights.dtype == torch.float32
        assert pop.weights.numpy().tobytes() == want.tobytes()              # NaN payloads and -0 included
        assert pop.value_heads.numpy().tobytes() == want_h.tobytes()
        assert pop.hidden.shape == (H, N) and pop.hidden.dtype == torch.float32 and not pop.hidden.any()
        b = pop.bound()
        assert type(b) is (L.PolicyGruMx if engine == "matrix" else L.PolicyGru)
        assert b.weights_bytes == 4 * want.shape[1] and b.weights_dev == pop.weights.data_ptr()
        assert b.state_bytes == 4 * H * N and b.state_dev == pop.hidden.data_ptr() and b.hidden == H
        assert pop.value().head_bytes == 4 * (H + 1) and pop.value().head_dev == pop.value_heads.data_ptr()
        assert (pop.population().n_members, pop.population().group) == (P, group)
        names, structs, groups = pop.entries(None, False)
        assert names == (ENTRIES[2:] if engine == "matrix" else ENTRIES[:2]) and groups == 3
        assert type(structs[0]) is L.PolicyPop and type(structs[1]) is L.PolicySampling and structs[2] is None
        assert pop.method == "policy_gru_population" and len(pop.feature_names()) == F
    pop = pops[0]
    # member_parts(m): views of row m, in the shapes a RecurrentPolicyController takes
    for m in range(P):
        cell, head = pop.member_parts(m)
        row, o = pop.weights[m], 0
        for t, src in zip(cell + head, members[m][0] + members[m][1]):
            assert t.shape == src.shape and t.numpy().tobytes() == src.tobytes()
            assert t.data_ptr() == row.data_ptr() + 4 * o
            o += t.numel()
        ctl = A.RecurrentPolicyController(_Player(64), cell, head, window=W, engine=engine, device="cpu")
        assert ctl.weights.numpy().tobytes() == want[m].tobytes()
    pop.member_parts(2)[0][0][0, 0] = 7.0
    assert pop.weights[2, 0] == 7.0
    # load_member touches only row m (and only that head), and never the state
    pop.hidden.copy_(torch.from_numpy(rng.standard_normal((H, N)).astype(f32)))
    state = pop.hidden.clone()
    before, before_h = pop.weights.clone(), pop.value_heads.clone()
    fresh, fresh_h = _member(rng, H), (rng.standard_normal(H).astype(f32), f32(0.25))
    pop.load_member(1, *fresh, value_head=fresh_h)
    assert pop.weights[1].numpy().tobytes() == pack_gru(*fresh).tobytes()
    assert pop.value_heads[1].numpy().tobytes() == np.append(fresh_h[0], fresh_h[1]).astype(f32).tobytes()
    for m in (0, 2):
        assert torch.equal(pop.weights[m], before[m]) and torch.equal(pop.value_heads[m], before_h[m])
    pop.load_member(0, *_modules(*fresh))
    assert pop.weights[0].numpy().tobytes() == pack_gru(*fresh).tobytes() and torch.equal(pop.value_heads[0], before_h[0])
    assert torch.equal(pop.hidden, state)
    # load_weights: every member, in place
    ptr = pop.weights.data_ptr()
    for form, hform in ((members, heads), (_stack(members), shead), ([_modules(c, h) for c, h in members], None)):
        pop.weights.zero_()
        pop.load_weights(form, value_heads=hform)
        assert pop.weights.data_ptr() == ptr and pop.weights.numpy().tobytes() == want.tobytes()
        assert pop.value_heads.numpy().tobytes() == want_h.tobytes()
    assert torch.equal(pop.hidden, state)
    # reset_hidden: the masked lanes, whatever member owns them; then all
    mask = torch.zeros(N, dtype=torch.bool)
    mask[250:260] = True
    pop.reset_hidden(mask)
    assert not pop.hidden[:, mask].any() and torch.equal(pop.hidden[:, ~mask], state[:, ~mask])
    with pytest.raises(ValueError):
        pop.reset_hidden(mask[:-1])
    pop.reset_hidden()
    assert not pop.hidden.any()
    # settings are shared and checked as the controller checks them
    pop.explore, pop.sample, pop.temperature, pop.seed = 0.25, "softmax", 0.5, 9
    assert pop.sampling().mode == L.POLICY_SOFTMAX and pop.sampling().inv_temperature == 2.0
    assert pop.bound().explore_threshold == 1 << 30 and pop.bound().seed == 9
    for attr, v in (("explore", 1.5), ("sample", "greedy"), ("temperature", 0.0)):
        with pytest.raises(ValueError):
            setattr(pop, attr, v)


def test_lane_arithmetic():
    import abrsimulator_amd as A
    rng = np.random.default_rng(4)
    for N, group in ((256, 256), (257, 256), (700, 256), (1024, 256), (1000, 512)):
        P = -(-N // group)
        pop = A.RecurrentPolicyPopulation(_Player(N), [_member(rng, 5) for _ in range(P)], group, device="cpu")
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
            with pytest.raises(IndexError):
                pop.member_parts(bad)


def test_refusals():
    import abrsimulator_amd as A
    rng = np.random.default_rng(5)
    mk = lambda H=5, **kw: _member(rng, H, **kw)
    ok = [mk(), mk(), mk()]
    R = A.RecurrentPolicyPopulation
    R(_Player(700), ok, 256, device="cpu")
    for group in (0, 255, 257, 384, -256, 256.5, True, None):             # the group
        with pytest.raises((ValueError, TypeError)):
            R(_Player(700), ok, group, device="cpu")
    for N in (512, 769, 1024):                                           # P is not ceil(N / group)
        with pytest.raises(ValueError, match="members"):
            R(_Player(N), ok, 256, device="cpu")
    for bad in ([mk(), mk(6), mk()], [mk(), mk(Fd=19), mk()], [mk(), mk(Md=5), mk()],         # one shape
                [mk(), (mk()[0][:3], mk()[1]), mk()], [mk(), mk()[0], mk()], [], None, torch.nn.GRUCell(F, 5)):
        with pytest.raises(ValueError):
            R(_Player(700), bad, 256, device="cpu")
    st = _stack(ok)
    for bad in (st[:5] + (st[5][:2],), st[:1] + (st[1][:, :, :4],) + st[2:]):                 # stacked: P and H disagree
        with pytest.raises(ValueError):
            R(_Player(700), bad, 256, device="cpu")
    # H limits per engine are RecurrentPolicyController's
    with pytest.raises(ValueError):
        R(_Player(700), [mk(65) for _ in range(3)], 256, device="cpu")
    R(_Player(700), [mk(65) for _ in range(3)], 256, device="cpu", engine="matrix")
    with pytest.raises(ValueError):
        R(_Player(700), [mk(129) for _ in range(3)], 256, device="cpu", engine="matrix")
    with pytest.raises(ValueError):
        R(_Player(700), ok, 256, device="cpu", engine="tensor")
    for kw in (dict(explore=1.5), dict(sample="greedy"), dict(temperature=0.0), dict(window=17), dict(norm="other")):
        with pytest.raises(ValueError):
            R(_Player(700), ok, 256, device="cpu", **kw)
    head = lambda n=5: (rng.standard_normal(n).astype(f32), f32(0.5))
    with pytest.raises(ValueError):                                       # heads: one per member, of the shape
        R(_Player(700), ok, 256, device="cpu", value_heads=[head(), head()])
    with pytest.raises(ValueError):
        R(_Player(700), ok, 256, device="cpu", value_heads=[head(), head(6), head()])
    pop = R(_Player(700), ok, 256, device="cpu")
    with pytest.raises(ValueError, match="value heads"):
        pop.value()
    with pytest.raises(ValueError, match="value heads"):                  # heads for a population built without them
        pop.load_weights(ok, value_heads=[head(), head(), head()])
    with pytest.raises(ValueError):
        pop.load_member(0, *mk(), value_head=head())
    with pytest.raises(ValueError):
        pop.load_weights(ok[:2])
    with pytest.raises(ValueError):
        pop.load_member(0, *mk(6))
    with pytest.raises(IndexError):
        pop.load_member(3, *mk())
    for env in (types.SimpleNamespace(n_lanes=1024, n_rates=6), types.SimpleNamespace(n_lanes=700, n_rates=5)):
        with pytest.raises(ValueError):                                   # another environment: the slab, P, the rates
            pop.bound(env)

    class Sharded:
        n_lanes, n_rates, device = 700, 6, torch.device("cpu")
    Sharded.__name__ = "ShardedABREnv"
    pl = _Player(700)
    pl.env = Sharded()
    with pytest.raises(ValueError, match="ShardedABREnv"):
        R(pl, ok, 256, device="cpu")
    # PolicyPopulation keeps refusing a recurrent member
    with pytest.raises(ValueError, match="recurrent"):
        A.PolicyPopulation(_Player(700), [torch.nn.GRUCell(F, 5)], group=256)


REFUSED_LOADS = ("stacked, bv of the wrong length", "stacked, Wv of the wrong width", "list, last member's hidden width",
                 "list, last member's head", "list of P - 1 members")


@pytest.mark.parametrize("case", REFUSED_LOADS)
def test_a_refused_load_writes_nothing(case):
    """load_weights is all or nothing: a generation with a fault anywhere -- in the last member, or in the heads, which
    come after the weights -- raises ValueError and leaves weights and value_heads bit for bit as they were."""
    import abrsimulator_amd as A
    rng = np.random.default_rng(6)
    P, H = 3, 5
    head = lambda n=H: (rng.standard_normal(n).astype(f32), f32(rng.standard_normal()))
    hstack = lambda hs: (np.stack([h[0] for h in hs]), np.array([h[1] for h in hs], f32))
    pop = A.RecurrentPolicyPopulation(_Player(700), [_member(rng, H) for _ in range(P)], 256,
                                      value_heads=[head() for _ in range(P)], device="cpu")
    new, heads = [_member(rng, H) for _ in range(P)], [head() for _ in range(P)]
    Wv, bv = hstack(heads)
    members, value_heads = {
        REFUSED_LOADS[0]: (_stack(new), (Wv, bv[:-1])),
        REFUSED_LOADS[1]: (_stack(new), (np.concatenate([Wv, Wv[:, :1]], axis=1), bv)),
        REFUSED_LOADS[2]: (new[:-1] + [_member(rng, H + 1)], heads),
        REFUSED_LOADS[3]: (new, heads[:-1] + [head(H + 1)]),
        REFUSED_LOADS[4]: (new[:-1], heads[:-1]),
    }[case]
    before, before_h = pop.weights.numpy().tobytes(), pop.value_heads.numpy().tobytes()
    with pytest.raises(ValueError):
        pop.load_weights(members, value_heads=value_heads)
    assert pop.weights.numpy().tobytes() == before and pop.value_heads.numpy().tobytes() == before_h
    assert not pop.hidden.any()
    pop.load_weights(new, value_heads=heads)                                # the same generation without the fault loads
    assert pop.weights.numpy().tobytes() != before and pop.value_heads.numpy().tobytes() != before_h
