"""Which check of a learned-policy entry point fails first, and with which message (include/abr_env.h documents the order
entry by entry): one table over the 20 select and rollout entries of the four engines, called on a NULL handle with
every single fault and every pair of simultaneous faults -- a bad reserved_ in the policy and in smp, a bad smp and
n_steps = 0, probs without smp and a bad pop, n_steps = 0 and the NULL handle, a misaligned value head and probs without
smp, and so on.  With several faults in one call the entry must report the one its order puts first.  The substrings and
the order lists below are literals recorded from the library: the 20 entries share one host path, and this table is what
keeps a change to that path from moving a check for one of them."""
import ctypes as C
import itertools

import pytest

PTR = C.c_void_p(8192)

# fault -> the substring of abr_last_error() that names it
MESSAGE = {
    "pol.null": b"policy is NULL",
    "pol.window": b"policy window 17 outside",
    "pol.n_hidden": b"policy n_hidden -1 outside",
    "pol.width": b"policy width[0] = 0 outside",
    "pol.hidden": b"policy hidden 0 outside",
    "pol.reserved": b"policy reserved_ must be 0",
    "pol.weights": b"policy weights must be non-NULL and 4-byte aligned",
    "pol.norm": b"policy norm must be 8-byte aligned",
    "pol.state": b"policy state must be non-NULL and 4-byte aligned",
    "pol.explore": b"explore_threshold 4294967297 above 2^32",
    "smp.null": b"sampling is NULL",
    "smp.mode": b"sampling mode 2 is neither",
    "smp.inv_temperature": b"sampling inv_temperature must be finite and > 0",
    "smp.reserved": b"sampling reserved_ must be 0",
    "val.null": b"value is NULL",
    "val.head": b"value head must be non-NULL and 4-byte aligned",
    "val.reserved": b"value reserved_ must be 0",
    "probs_without_smp": b"probs need a sampling struct",
    "values_without_val": b"values need a value struct",
    "last_value_without_val": b"values need a value struct",
    "pop.null": b"population is NULL",
    "pop.n_members": b"population n_members 0 must be >= 1",
    "pop.group": b"population group 100 must be a positive multiple of 256",
    "pop.reserved": b"population reserved_ must be 0",
    "pop.overflow": b"overflows the lanes of a launch",
    "n_steps": b"n_steps must be >= 1",
    "handle.select": b"NULL argument (env or action_out_dev)",
    "handle.step": b"env is NULL",
}

# the order in which an entry's checks fire, in pieces
MLP = ("pol.null", "pol.window", "pol.n_hidden", "pol.width", "pol.reserved", "pol.weights", "pol.norm", "pol.explore")
GRU = ("pol.null", "pol.window", "pol.hidden", "pol.reserved", "pol.weights", "pol.norm", "pol.state", "pol.explore")
SMP = ("smp.mode", "smp.inv_temperature", "smp.reserved")
VAL = ("val.head", "val.reserved")
SMP_REQUIRED, VAL_REQUIRED = ("smp.null",) + SMP, ("val.null",) + VAL
ABSENT = ("probs_without_smp", "values_without_val")
ABSENT_STEP = ABSENT + ("last_value_without_val",)
POP = ("pop.null", "pop.n_members", "pop.group", "pop.reserved", "pop.overflow")
N = ("n_steps",)

# (entry, policy struct, smp, val: "required" / "optional" / None, pop, the checks before the handle in firing order)
ENTRIES = [
    ("abr_env_policy_select", "Policy", None, None, False, MLP),
    ("abr_env_step_policy", "Policy", None, None, False, MLP + N),
    ("abr_env_policy_select_sampled", "Policy", "required", None, False, MLP + SMP_REQUIRED),
    ("abr_env_step_policy_sampled", "Policy", "required", None, False, MLP + SMP_REQUIRED + N),
    ("abr_env_policy_select_ac", "Policy", "required", "required", False, MLP + SMP_REQUIRED + VAL_REQUIRED),
    ("abr_env_step_policy_ac", "Policy", "required", "required", False, MLP + SMP_REQUIRED + VAL_REQUIRED + N),
    ("abr_env_policy_select_mx", "PolicyMx", "optional", "optional", False, MLP + SMP + VAL + ABSENT),
    ("abr_env_step_policy_mx", "PolicyMx", "optional", "optional", False, MLP + SMP + VAL + ABSENT_STEP + N),
    ("abr_env_policy_select_pop", "Policy", "optional", "optional", True, MLP + SMP + VAL + ABSENT + POP),
    ("abr_env_step_policy_pop", "Policy", "optional", "optional", True, MLP + SMP + VAL + ABSENT_STEP + POP + N),
    ("abr_env_policy_select_mx_pop", "PolicyMx", "optional", "optional", True, MLP + SMP + VAL + ABSENT + POP),
    ("abr_env_step_policy_mx_pop", "PolicyMx", "optional", "optional", True, MLP + SMP + VAL + ABSENT_STEP + POP + N),
    ("abr_env_policy_select_gru", "PolicyGru", "optional", "optional", False, GRU + SMP + VAL + ABSENT),
    ("abr_env_step_policy_gru", "PolicyGru", "optional", "optional", False, GRU + SMP + VAL + ABSENT_STEP + N),
    ("abr_env_gru_mx_select", "PolicyGruMx", "optional", "optional", False, GRU + SMP + VAL + ABSENT),
    ("abr_env_gru_mx_step", "PolicyGruMx", "optional", "optional", False, GRU + SMP + VAL + ABSENT_STEP + N),
    ("abr_env_gru_select_pop", "PolicyGru", "optional", "optional", True, GRU + SMP + VAL + ABSENT + POP),
    ("abr_env_gru_step_pop", "PolicyGru", "optional", "optional", True, GRU + SMP + VAL + ABSENT_STEP + POP + N),
    ("abr_env_gru_mx_select_pop", "PolicyGruMx", "optional", "optional", True, GRU + SMP + VAL + ABSENT + POP),
    ("abr_env_gru_mx_step_pop", "PolicyGruMx", "optional", "optional", True, GRU + SMP + VAL + ABSENT_STEP + POP + N),
]
RECURRENT = ("PolicyGru", "PolicyGruMx")
# each recurrent struct's own limit on `hidden`: every valid call is made at the limit, and
# test_each_engine_has_its_own_limits calls one past it
HIDDEN = {"PolicyGru": 64, "PolicyGruMx": 128}


def _is_step(name):
    return "_step" in name


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


def _valid(L, struct, smp, val, pop):
    """A call every check before the handle lets through: the arguments by name."""
    p = getattr(L, struct)()
    p.window, p.weights_dev, p.weights_bytes, p.seed = 8, 4096, 100, 1
    if struct in RECURRENT:
        p.hidden, p.state_dev, p.state_bytes = HIDDEN[struct], 8192, 100
    else:
        p.n_hidden, p.width[0], p.width[1] = 2, 64, 64
    a = dict(pol=p, smp=None, val=None, pop=None, n=4, probs=None, values=None, last=None)
    if smp:
        a["smp"] = L.PolicySampling()
        a["smp"].mode, a["smp"].inv_temperature = L.POLICY_SOFTMAX, 1.0
    if val:
        a["val"] = L.PolicyValue()
        a["val"].head_dev, a["val"].head_bytes = 4096, 4 * 65
    if pop:
        a["pop"] = L.PolicyPop()
        a["pop"].n_members, a["pop"].group = 2, 256
    return a


def _field(arg, name, value):
    def apply(a):
        if name == "reserved_":
            a[arg].reserved_[0] = value
        elif name == "width":
            a[arg].width[0] = value
        else:
            setattr(a[arg], name, value)
    return (arg, name), apply


def _whole(arg, **also):
    def apply(a):
        a[arg] = None
        a.update(also)
    return (arg, None), apply


def _pop_overflow(a):
    a["pop"].n_members, a["pop"].group = 2 ** 31 - 1, 2 ** 31 - 256


# fault -> ((the argument it touches, the field or None for the whole argument), how to inject it)
FAULTS = {
    "pol.null": _whole("pol"),
    "pol.window": _field("pol", "window", 17),
    "pol.n_hidden": _field("pol", "n_hidden", -1),
    "pol.width": _field("pol", "width", 0),
    "pol.hidden": _field("pol", "hidden", 0),
    "pol.reserved": _field("pol", "reserved_", 1),
    "pol.weights": _field("pol", "weights_dev", 4098),
    "pol.norm": _field("pol", "norm_dev", 4100),
    "pol.state": _field("pol", "state_dev", None),
    "pol.explore": _field("pol", "explore_threshold", 2 ** 32 + 1),
    "smp.null": _whole("smp"),
    "smp.mode": _field("smp", "mode", 2),
    "smp.inv_temperature": _field("smp", "inv_temperature", 0.0),
    "smp.reserved": _field("smp", "reserved_", 1),
    "val.null": _whole("val"),
    "val.head": _field("val", "head_dev", 4098),
    "val.reserved": _field("val", "reserved_", 1),
    "probs_without_smp": _whole("smp", probs=PTR),
    "values_without_val": _whole("val", values=PTR),
    "last_value_without_val": _whole("val", last=PTR),
    "pop.null": _whole("pop"),
    "pop.n_members": _field("pop", "n_members", 0),
    "pop.group": _field("pop", "group", 100),
    "pop.reserved": _field("pop", "reserved_", 1),
    "pop.overflow": (("pop", "n_members+group"), _pop_overflow),
    "n_steps": (("n", None), lambda a: a.update(n=0)),
}


def _compatible(f, g):
    """Two faults can be injected into one call: they touch different arguments, or different fields of one struct."""
    (fa, ff), (ga, gf) = FAULTS[f][0], FAULTS[g][0]
    if "pop.overflow" in (f, g) and {f, g} & {"pop.n_members", "pop.group"}:
        return False
    return fa != ga or (ff is not None and gf is not None and ff != gf)


def call(lib, entry, a):
    """The entry on a NULL handle: (return code, abr_last_error())."""
    name, struct, smp, val, pop, _ = entry
    step, ref = _is_step(name), lambda s: C.byref(s) if s is not None else None
    args = [None, ref(a["pol"])] + ([ref(a["pop"])] if pop else []) + ([ref(a["smp"])] if smp else []) + \
        ([ref(a["val"])] if val else [])
    if step:
        args += [a["n"]] + [None] * 6                                       # obs, reward, done, actions, features, scores
    else:
        args += ([0] if struct in RECURRENT else []) + [PTR, None, None]  # commit; action, features, scores
    args += ([a["probs"]] if smp else []) + ([a["values"]] if val else []) + ([a["last"]] if val and step else [])
    args += ([None] if struct in RECURRENT else []) + [None]              # hidden; stream
    rc = getattr(lib, name)(*args)
    return rc, lib.abr_last_error()


def cases(entry):
    """(the optional structs left out, the faults injected, the fault that must be reported) for every call of `entry`."""
    name, _, smp, val, _, order = entry
    handle = "handle.step" if _is_step(name) else "handle.select"
    variants = [()]
    if smp == "optional":
        variants += [("smp",), ("val",), ("smp", "val")]
    for absent in variants:
        live = [f for f in order if FAULTS[f][0][0] not in absent or FAULTS[f][0][1] is None]
        yield absent, (), handle
        for f in live:
            yield absent, (f,), f
        for f, g in itertools.combinations(live, 2):                       # f fires before g
            if _compatible(f, g):
                yield absent, (f, g), f


def run(L, entry, absent, faults):
    _, struct, smp, val, pop, _ = entry
    a = _valid(L, struct, smp, val, pop)
    for k in absent:
        a[k] = None
    for f in faults:
        FAULTS[f][1](a)
    return call(L.lib(), entry, a)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e[0])
def test_first_failing_check_and_its_message(L, entry):
    n = 0
    for absent, faults, first in cases(entry):
        rc, err = run(L, entry, absent, faults)
        assert rc == -1 and MESSAGE[first] in err, (entry[0], absent, faults, first, err)
        n += 1
    assert n > len(entry[5]) * (len(entry[5]) - 1) // 3                     # singles and most pairs ran


LIMITS = [  # (entry, struct, size query, field, its limit, the message one past it)
    ("abr_env_policy_select", "Policy", "abr_policy_weights_bytes", "n_hidden", 2, b"policy n_hidden 3 outside 0..2"),
    ("abr_env_policy_select", "Policy", "abr_policy_weights_bytes", "width", 64, b"policy width[0] = 65 outside 1..64"),
    ("abr_env_policy_select_mx", "PolicyMx", "abr_policy_mx_weights_bytes", "n_hidden", 3, b"policy n_hidden 4 outside 0..3"),
    ("abr_env_policy_select_mx", "PolicyMx", "abr_policy_mx_weights_bytes", "width", 128,
     b"policy width[0] = 129 outside 1..128"),
    ("abr_env_policy_select_gru", "PolicyGru", "abr_policy_gru_weights_bytes", "hidden", 64, b"policy hidden 65 outside 1..64"),
    ("abr_env_gru_mx_select", "PolicyGruMx", "abr_policy_gru_mx_weights_bytes", "hidden", 128,
     b"policy hidden 129 outside 1..128"),
]


@pytest.mark.parametrize("limit", LIMITS, ids=lambda t: t[1] + "." + t[3])
def test_each_engine_has_its_own_limits(L, limit):
    """A shape at an engine's limit passes every check before the handle and its size query; one past the limit fails
    with that engine's bound in the message, in the entry and in the query alike."""
    name, struct, query, field, top, message = limit
    entry = next(e for e in ENTRIES if e[0] == name)

    def calls(value):
        a = _valid(L, struct, entry[2], entry[3], entry[4])
        if field == "n_hidden":
            a["pol"].n_hidden = value
            for l in range(min(value, len(a["pol"].width))):
                a["pol"].width[l] = 32
        elif field == "width":
            a["pol"].width[0] = value
        else:
            setattr(a["pol"], field, value)
        n = C.c_size_t(0)
        rc = getattr(L.lib(), query)(C.byref(a["pol"]), 6, C.byref(n))
        return call(L.lib(), entry, a), (rc, L.lib().abr_last_error())

    (rc, err), (qrc, _) = calls(top)
    assert rc == -1 and MESSAGE["handle.select"] in err and qrc == 0
    (rc, err), (qrc, qerr) = calls(top + 1)
    assert rc == -1 and message in err and qrc == -1 and message in qerr


def test_table_covers_the_abi(L):
    names = [s[0] for s in L.SYMBOLS if s[0].startswith(("abr_env_policy_select", "abr_env_step_policy", "abr_env_gru_"))]
    assert sorted(names) == sorted(e[0] for e in ENTRIES) and len(names) == 20
    assert set(FAULTS) | {"handle.select", "handle.step"} == set(MESSAGE)
    for f, g in (("pol.reserved", "smp.reserved"), ("smp.mode", "n_steps"), ("probs_without_smp", "pop.group"),
                 ("val.head", "probs_without_smp"), ("values_without_val", "pop.null")):
        assert _compatible(f, g)                                            # the pairs the order matters most for


def test_the_python_engine_table_is_the_abi(L):
    """policy.ENGINES, which every entries() reads, names exactly the 20 entries of the table above and the four size
    queries, all of them bound symbols; and each entry is what exactly one (class, engine) pair launches -- one pair per
    class and engine, but for the lane MLP, which has a pair per mode (plain, sampled, actor-critic)."""
    import types

    import numpy as np
    import torch

    import abrsimulator_amd as A
    from abrsimulator_amd import policy
    from abrsimulator_amd.datamodel import MPD, Chunk
    rows = [row for family in policy.ENGINES.values() for row in family.values()]
    assert [sorted(family) for family in policy.ENGINES.values()] == [["lane", "matrix"]] * 2
    names = [n for row in rows for pair in row.single + (row.pop,) for n in pair]
    assert sorted(names) == sorted(e[0] for e in ENTRIES) and len(set(names)) == 20
    symbols = [s[0] for s in L.SYMBOLS]
    assert all(n in symbols for n in names)
    assert sorted(row.size_query for row in rows) == sorted(s for s in symbols if s.endswith("_weights_bytes"))
    assert len(rows) == 4

    class Player:
        env = types.SimpleNamespace(n_lanes=256, n_rates=6, device=torch.device("cpu"))

        def get_mpd(self):
            return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))

    F, M, z = 18, 6, lambda *shape: np.zeros(shape, np.float32)
    mlp, gru, head = [(z(M, F), z(M))], ((z(3, F), z(3, 1), z(3), z(3)), (z(M, 1), z(M))), lambda n: (z(n), np.float32(0))
    reached = {}
    for engine in ("lane", "matrix"):
        kw = dict(engine=engine, device="cpu")
        for ctl in (A.PolicyController(Player(), mlp, value_head=head(F), **kw),
                    A.PolicyPopulation(Player(), [mlp], 256, value_heads=[head(F)], **kw),
                    A.RecurrentPolicyController(Player(), *gru, value_head=head(1), **kw),
                    A.RecurrentPolicyPopulation(Player(), [gru], 256, value_heads=[head(1)], **kw)):
            pairs = set()
            for sample, val, probs in itertools.product(policy.SAMPLE_MODES, (None, ctl.value()), (False, True)):
                ctl.sample = sample
                pair, structs, groups = ctl.entries(val, probs)
                assert "select" in pair[0] and "step" in pair[1] and (val is None or any(s is val for s in structs))
                pairs.add(pair)
            assert len(pairs) == (3 if (type(ctl), engine) == (A.PolicyController, "lane") else 1)
            for n in (n for pair in pairs for n in pair):
                assert reached.setdefault(n, (type(ctl).__name__, engine)) == (type(ctl).__name__, engine)
    assert sorted(reached) == sorted(names)
