"""The proven form of chain_segment (csrc/abr_exact_jump.h: GUARDS_PROVEN) on the DEVICE, and the routing of handles that
fail its proof.

Part one, through abr_debug_chain with bit 8 of its kind argument: 64 threads x 300 chains per stop kind plus the edges of
the proven form's domain (budgets of 1 and of exactly 2^20, a zero constant, a start at zero, subnormal constants, 1e298
per tick against a finite target, stops already behind the value, values of 2^1023 and more), with the estimate as it is
and spoiled by +4 and -4, against the naive loop run on the host (tests/native/chain_settle_harness.cpp asserts chain ==
naive there, so the host values ARE the naive loop's).

Part two, through the environment: 130 lanes (two full waves and a partial one), a video of 5 chunks at three rates, 13
decisions fused in one scripted launch with auto_reset, one trace each of the outage, burst, short, tiny and extreme
families, on the jump, split and split3 kernels -- whose no-speeds instances run the proven chains -- and on the tick
kernel as the cross-check, against the oracle's replay: observations, rewards, done bits, and the workspace read back in
full.

Part three: the same run with a trace interval below one tick.  The handle fails the proof, says that it runs the
general instances, and still equals the oracle on all three kernels."""
import numpy as np
import pytest
import torch

from test_chain_guards_cpu import CAP, _precondition_edges
from test_chain_settle_cpu import GE, LE, LT, H, _block, run_block  # noqa: F401  (host harness; H is its fixture)
from test_chain_settle_gpu import _chains, _device

pytestmark = pytest.mark.gpu

PROVEN = 0x100                           # abr_debug_chain: stop_kind + 0x100 runs the proven form


def _domain_chains(kind):
    """test_chain_settle_gpu's 19 200 chains of one stop kind with their budgets inside 1..2^20, then the domain's edges."""
    x0, c, thr, n = _chains(kind)
    n = np.clip(n, 1, CAP).astype(np.int32)
    n[:3] = (1, 1, CAP)
    edges = [b for b in _precondition_edges() if b[0] == kind]
    cat = lambda i, first: np.concatenate([first] + [b[i] for b in edges])
    return cat(2, x0), cat(3, c), cat(4, thr), cat(5, n).astype(np.int32)


@pytest.mark.parametrize("kind", [GE, LE, LT], ids=["ge", "le", "lt"])
def test_proven_chains_against_the_host_naive_loop(H, kind):
    x0, c, thr, n = _domain_chains(kind)
    assert n.min() >= 1 and n.max() == CAP and np.isfinite(x0).all() and np.isfinite(c).all() and np.isfinite(thr).all()
    xh, ah, hh, _ = run_block(H, _block(kind, 0, x0, c, thr, n))        # chain == naive loop is asserted inside
    for bias in (0, 4, -4):
        xd, ad, hd = _device(kind | PROVEN, bias, x0, c, thr, n)
        bad = np.flatnonzero((xd.view(np.uint64) != xh.view(np.uint64)) | (ad != ah) | (hd != hh))
        assert bad.size == 0, (kind, bias, bad[:3], x0[bad[:3]], c[bad[:3]], thr[bad[:3]], n[bad[:3]], xd[bad[:3]],
                               xh[bad[:3]], ad[bad[:3]], ah[bad[:3]])


# ---------------------------------------------------------------------------------------------------------------------
# through the environment

ENV_IMPLS = ("jump", "split", "split3", "tick")
FAMILIES = ("outage", "burst", "short", "tiny", "extreme")


def _env_case(interval):
    """130 lanes, V = 5, a three-rate ladder, 13 decisions in one fused scripted launch (auto_reset: two whole episodes and
    three decisions of a third) on one trace of each family; the oracle's replays are computed here, before any launch."""
    import closed_loop_check as K
    import trace_families as TF
    from oracle import oracle as O
    V, N, T = 5, 130, 13
    rng = np.random.default_rng(78)
    traces = [TF.make(f, rng, 3 if f == "short" else 100) for f in FAMILIES]
    tl = np.array([len(t) for t in traces])
    tid = (np.arange(N) % len(traces)).astype(np.int32)
    off = (rng.integers(0, 1 << 20, N) % tl[tid]).astype(np.int32)
    meta = dict(ladder=[0.3, 1.2, 4.3], chunk_length=2.0, video_length=V, max_buffer=6.0, start_up_length=2.0,
                interval=interval, weights=[4.3, 1.0, 1.0, 0.1], speed=1.0)
    n_ep = -(-T // V)
    script = rng.integers(0, 3, (n_ep * V, N)).astype(np.int32)
    case = dict(seed=0, ctl="script", feature="config", impl=None, vbr=False, auto_reset=True, n_lanes=N, meta=meta,
                traces=traces, tid=tid, off=off, br=None, params={}, n_steps=T, script=script, launch="script", philox=0,
                trace_family="guards", pieces=[T])
    case["replays"] = []
    for e in range(n_ep):
        a = np.ascontiguousarray(script[e * V:(e + 1) * V].T)
        steps, bw, fin, _ = O.env_batch(K.env_cfg(case), traces, tid, off, a, max_ticks=TF.TICK_ORACLE_BOUND)
        case["replays"].append((steps, bw, fin, a))
    case["max_ticks"] = max(int(r[2]["ticks"].max()) for r in case["replays"]) + 1000
    assert case["max_ticks"] <= CAP
    return case


@pytest.fixture(scope="module")
def env_case():
    return _env_case(0.5)


@pytest.fixture(scope="module")
def unproven_case():
    return _env_case(0.004)                  # 2.5 trace samples per tick: intervals that span no tick at all


def _general_instance(case, impl):
    """What the handle of `case` says about its instances (a handle of its own: nothing is launched on it)."""
    import abrsimulator_amd as A
    m = case["meta"]
    env = A.BatchedABREnv(A.MPD(m["video_length"], m["chunk_length"], m["max_buffer"], m["start_up_length"], A.Chunk(m["ladder"])),
                          A.QOEMetric(*m["weights"]), A.NetworkInfo(m["interval"], case["traces"]), case["n_lanes"],
                          speed=m["speed"], impl=impl, auto_reset=True, max_ticks=case["max_ticks"])
    try:
        return env.general_instance(fused=True), env.general_instance(fused=False)
    finally:
        env.close()


def _run_and_check(case, impl):
    import closed_loop_check as K
    from test_trace_edges_gpu import frame_extras, run_open_case
    out = run_open_case(dict(case, impl=impl), impl)
    assert ((out["done"] & K.DONE_TIMEOUT) == 0).all()
    with np.errstate(over="ignore"):
        mm = K.check(case, out) + frame_extras(case, out["frames"])
    assert not mm, (impl, len(mm), mm[:6])


@pytest.mark.parametrize("impl", ENV_IMPLS)
def test_thirteen_fused_decisions_on_the_proven_chains(env_case, impl):
    if impl != "tick":
        assert _general_instance(env_case, impl) == (False, False)       # the no-speeds instances: the proven chains
    _run_and_check(env_case, impl)


@pytest.mark.parametrize("impl", ["jump", "split", "split3"])
def test_a_handle_that_fails_the_proof_runs_the_general_instances(unproven_case, impl):
    assert _general_instance(unproven_case, impl) == (True, True)
    _run_and_check(unproven_case, impl)
