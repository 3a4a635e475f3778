"""The remainder settlement of chain_segment (csrc/abr_exact_jump.h) on the DEVICE.

Part one, through the diagnostic entry point abr_debug_chain: a few hundred chains per thread of a workgroup for each
stop kind (one chain per thread is how that entry point launches: 19 200 threads), with the estimate as it is and
spoiled by +4 (the repair path) and -4 (short jumps), against the naive loop run on the host
(tests/native/chain_settle_harness.cpp asserts chain == naive there, so the host values ARE the naive loop's).

Part two, through the environment: 130 lanes (two full waves and a partial one), a video of 5 chunks at three rates, 13
decisions fused in one scripted launch with auto_reset, on the jump, split, split3 and tick kernels against the oracle's
replay -- observations, rewards, done bits, and the workspace read back in full (every float64 field, the flags, the
history rows, the episode QoE).  One trace each of the outage, burst and short families, so that zero constants (no jump),
chunks that finish on their first tick and intervals whose budget is spent between two segments run on the device too."""
import numpy as np
import pytest
import torch

from test_chain_settle_cpu import GE, LE, LT, H, _block, run_block  # noqa: F401  (host harness; H is its fixture)

pytestmark = pytest.mark.gpu

THREADS, PER_THREAD = 64, 300            # a workgroup's worth of chains at 300 per thread; abr_debug_chain runs one chain per
                                         # thread in workgroups of 64, so they go down as one launch of 19 200 chains


def _device(kind, bias, x0, c, thr, n):
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a, d)).cuda()
    x0, c, thr, n = t(x0, np.float64), t(c, np.float64), t(thr, np.float64), t(n, np.int32)
    N = x0.numel()
    xo = torch.empty(N, dtype=torch.float64, device="cuda")
    ao = torch.empty(N, dtype=torch.int32, device="cuda")
    ho = torch.empty(N, dtype=torch.uint8, device="cuda")
    _lib.check(lib.abr_debug_chain(kind, bias, _lib.ptr(x0), _lib.ptr(c), _lib.ptr(thr), _lib.ptr(n), N,
                                   _lib.ptr(xo), _lib.ptr(ao), _lib.ptr(ho), None))
    torch.cuda.synchronize()
    return xo.cpu().numpy(), ao.cpu().numpy(), ho.cpu().numpy()


def _chains(kind):
    """THREADS * PER_THREAD chains of one stop kind: simulator shapes, exact thresholds (r == 0, r == dm) in [1, 2), ties,
    and a few budgets of 0, 1 and past the segment cap."""
    rng = np.random.default_rng(50 + kind)
    N = THREADS * PER_THREAD
    u = 2.0 ** -52
    cg = rng.integers(1, 1 << 30, N) * u * rng.choice([1.0, 2.0 ** 8, 2.0 ** 16], N)       # on the grid of [1, 2)
    M = rng.integers(1, 2000, N)
    du = rng.integers(-1, 2, N) * u
    base = np.ldexp(1.0, rng.integers(-8, 6, N))
    ct = rng.integers(1, 1 << 44, N).astype(np.float64) * (base * u) + base * u / 2            # ties
    km = rng.integers(0, 1 << 20, N)
    pick = rng.integers(0, 3, N)
    if kind == GE:
        x_sim = np.where(rng.random(N) < 0.4, 0.0, rng.uniform(0, 20, N))
        c_sim = rng.uniform(0.05, 12.0, N).astype(np.float32).astype(np.float64) * 0.01
        t_sim = rng.choice([0.3, 0.75, 1.2, 1.85, 2.85, 4.3], N) * rng.choice([1.0, 2.0, 4.0], N)
        x_edge = 1.0 + rng.integers(0, 1 << 40, N) * u
        x_tie = base * (1.0 + km * u)
        x0 = np.choose(pick, [x_sim, x_edge, x_tie])
        c = np.choose(pick, [c_sim, cg, ct])
        thr = np.choose(pick, [t_sim, x_edge + M * cg + du, x_tie + ct * rng.integers(1, 600, N)])
    else:
        x_sim = np.where(rng.random(N) < 0.5, rng.integers(1, 7, N) * 4.0, rng.uniform(0.001, 30, N))
        sd = rng.choice([0.01, 0.0125, 0.005, 0.02], N)
        t_sim = np.zeros(N) if kind == LE else rng.choice([20.0, 3.0, 4.0, 9.0], N)
        x_sim = x_sim if kind == LE else t_sim + rng.uniform(0, 5, N)
        x_edge = 2.0 - rng.integers(1, 1 << 40, N) * u
        x_tie = base * (2.0 - km * u)
        x0 = np.choose(pick, [x_sim, x_edge, x_tie])
        c = -np.choose(pick, [sd, cg, ct])
        thr = np.choose(pick, [t_sim, np.maximum(x_edge - M * cg + du, 1.0),
                               np.maximum(x_tie - ct * rng.integers(1, 600, N), 0.0)])
    n = np.where(pick == 1, np.maximum(M + rng.integers(-2, 4, N), 0), rng.integers(1, 3000, N)).astype(np.int32)
    n[:3] = (0, 1, (1 << 20) + 1)
    return x0, c, thr, n


@pytest.mark.parametrize("kind", [GE, LE, LT], ids=["ge", "le", "lt"])
def test_chains_against_the_host_naive_loop(H, kind):
    x0, c, thr, n = _chains(kind)
    # the host's answers once: chain == naive loop is asserted inside, so these are the naive loop's values
    xh, ah, hh, _ = run_block(H, _block(kind, 0, x0, c, thr, n))
    for bias in (0, 4, -4):
        xd, ad, hd = _device(kind, bias, x0, c, thr, n)
        bad = np.flatnonzero((xd.view(np.uint64) != xh.view(np.uint64)) | (ad != ah) | (hd != hh))
        assert bad.size == 0, (kind, bias, bad[:3], x0[bad[:3]], c[bad[:3]], thr[bad[:3]], n[bad[:3]], xd[bad[:3]],
                               xh[bad[:3]], ad[bad[:3]], ah[bad[:3]])


# ---------------------------------------------------------------------------------------------------------------------
# through the environment

ENV_IMPLS = ("jump", "split", "split3", "tick")


@pytest.fixture(scope="module")
def env_case():
    """130 lanes, V = 5, a three-rate ladder, 13 decisions in one fused scripted launch (auto_reset: two whole episodes and
    three decisions of a third); the oracle's replays are computed here, once, before any launch."""
    import closed_loop_check as K
    import trace_families as TF
    from oracle import oracle as O
    V, N, T = 5, 130, 13
    rng = np.random.default_rng(77)
    traces = [TF.make("outage", rng, 120), TF.make("burst", rng, 90), TF.make("short", rng, 3)]
    tl = np.array([len(t) for t in traces])
    tid = (np.arange(N) % 3).astype(np.int32)
    off = (rng.integers(0, 1 << 20, N) % tl[tid]).astype(np.int32)
    meta = dict(ladder=[0.3, 1.2, 4.3], chunk_length=2.0, video_length=V, max_buffer=6.0, start_up_length=2.0,
                interval=0.5, weights=[4.3, 1.0, 1.0, 0.1], speed=1.0)
    n_ep = -(-T // V)
    script = rng.integers(0, 3, (n_ep * V, N)).astype(np.int32)
    case = dict(seed=0, ctl="script", feature="config", impl=None, vbr=False, auto_reset=True, n_lanes=N, meta=meta,
                traces=traces, tid=tid, off=off, br=None, params={}, n_steps=T, script=script, launch="script", philox=0,
                trace_family="settle", pieces=[T])
    case["replays"] = []
    for e in range(n_ep):
        a = np.ascontiguousarray(script[e * V:(e + 1) * V].T)
        steps, bw, fin, _ = O.env_batch(K.env_cfg(case), traces, tid, off, a, max_ticks=TF.TICK_ORACLE_BOUND)
        case["replays"].append((steps, bw, fin, a))
    case["max_ticks"] = max(int(r[2]["ticks"].max()) for r in case["replays"]) + 1000
    return case


@pytest.mark.parametrize("impl", ENV_IMPLS)
def test_thirteen_fused_decisions_against_the_oracle_replay(env_case, impl):
    import closed_loop_check as K
    from test_trace_edges_gpu import frame_extras, run_open_case
    out = run_open_case(dict(env_case, impl=impl), impl)
    assert ((out["done"] & K.DONE_TIMEOUT) == 0).all()
    with np.errstate(over="ignore"):
        mm = K.check(env_case, out) + frame_extras(env_case, out["frames"])
    assert not mm, (impl, len(mm), mm[:6])
