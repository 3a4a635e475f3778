"""The bitrate rules without a GPU: the device source (csrc/abr_lane_jump.h: rule_select) compiled for the host against
the numpy twin on seeded cases with their knife edges, the ABI struct and validation, the controllers' parameters, and
the compiled MODE 4 instances."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import c_abi_output, native_harness
from rules_twin import BOLA, BUFFER, RATE, rule_scalar, rule_vec

HMAX = 64


@pytest.fixture(scope="module")
def H():
    return native_harness("rules_harness")


def _cases(rng, n, kind):
    """n seeded call sites of one rule kind, a quarter of them on a knife edge."""
    M = rng.integers(1, 17, n).astype(np.int32)
    br = np.zeros((n, 16))
    for i in range(n):
        b = np.sort(rng.uniform(0.1, 8.0, M[i]))
        if rng.random() < 0.25:
            b = rng.permutation(b)                      # non-ascending ladders
        br[i, :M[i]] = b
    c = rng.integers(0, HMAX, n).astype(np.int32)
    c[: n // 8] = rng.integers(0, 4, n // 8)           # c < W
    B = rng.uniform(0.0, 40.0, n)
    B[rng.random(n) < 0.05] = 0.0
    h = rng.uniform(0.05, 10.0, (n, HMAX))
    window = rng.integers(1, 12, n).astype(np.int32)
    reservoir = rng.uniform(0.0, 10.0, n)
    reservoir[rng.random(n) < 0.1] = 0.0
    cushion = rng.uniform(0.5, 20.0, n)
    safety = rng.uniform(0.3, 1.5, n)
    safety[rng.random(n) < 0.3] = 1.0
    bola_v = rng.uniform(0.1, 5.0, n)
    bola_gp = rng.uniform(-2.0, 8.0, n)
    u = np.zeros((n, 16))
    for i in range(n):
        u[i, :M[i]] = np.log(br[i, :M[i]] / br[i, 0])
    edge = rng.random(n)
    for i in range(n):
        e, m_ = edge[i], M[i]
        if kind == BUFFER:
            if e < 0.08:
                B[i] = reservoir[i]                                     # B == r
            elif e < 0.16:
                B[i] = reservoir[i] + cushion[i]                        # B == r + k
            elif e < 0.30 and m_ >= 3:
                # X exactly a ladder rate: the rate map's X, written into an interior rung (X depends on br[0], br[M-1] only)
                B[i] = reservoir[i] + rng.uniform(0.0, 1.0) * cushion[i]
                X = br[i, 0] + ((B[i] - reservoir[i]) / cushion[i]) * (br[i, m_ - 1] - br[i, 0])
                br[i, rng.integers(1, m_ - 1)] = X
        elif kind == RATE:
            if e < 0.15 and m_ >= 2 and c[i] > 0:
                n_ = min(window[i], c[i])
                S = 0.0
                for j in range(c[i] - n_, c[i]):
                    S = S + 1.0 / h[i, j]
                br[i, rng.integers(1, m_)] = safety[i] * (float(n_) / S)   # X exactly a ladder rate
            elif e < 0.25:
                h[i, :] = h[i, 0]                                        # constant history
        else:
            if e < 0.2 and m_ >= 2:
                # exactly tied scores: two rungs with the same bitrate and utility
                a_, b_ = sorted(rng.choice(m_, 2, replace=False))
                br[i, b_] = br[i, a_]
                u[i, b_] = u[i, a_]
            elif e < 0.3 and m_ >= 2:
                u[i, :m_] = 0.0                                          # all utilities equal
                br[i, :m_] = br[i, 0]
    return dict(M=M, br=br, c=c, B=B, h=h, window=window, reservoir=reservoir, cushion=cushion, safety=safety,
                bola_v=bola_v, bola_gp=bola_gp, u=u)


def _run(H, kind, k):
    n = len(k["M"])
    kinds = np.full(n, kind, np.int32)
    out = np.zeros(n, np.int32)
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    arrs = [np.ascontiguousarray(x) for x in (kinds, k["window"], k["reservoir"], k["cushion"], k["safety"], k["bola_v"],
                                               k["bola_gp"], k["c"], k["B"], k["M"], k["br"], k["h"], k["u"])]
    types = [C.c_int32, C.c_int32] + [C.c_double] * 5 + [C.c_int32, C.c_double, C.c_int32, C.c_double, C.c_double,
                                                         C.c_double]
    ptrs = [P(a, t) for a, t in zip(arrs, types)]
    H.rh_select(C.c_int64(n), *ptrs[:12], C.c_int32(HMAX), ptrs[12], out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def _params(k, i, kind):
    return dict(kind=kind, window=int(k["window"][i]), reservoir=k["reservoir"][i], cushion=k["cushion"][i],
                safety=k["safety"][i], v=k["bola_v"][i], gp=k["bola_gp"][i])


@pytest.mark.parametrize("kind", [BUFFER, RATE, BOLA])
def test_host_build_matches_twin(H, kind):
    rng = np.random.default_rng(1000 + kind)
    n = 40000
    k = _cases(rng, n, kind)
    got = _run(H, kind, k)
    # the scalar twin on every case
    want = np.array([rule_scalar(_params(k, i, kind), k["c"][i], k["B"][i], k["h"][i], k["br"][i, :k["M"][i]],
                                 k["u"][i, :k["M"][i]]) for i in range(n)], np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    # the vectorised twin on each (M, parameter set) group: one parameter set, lanes over cases
    for M in (1, 2, 6, 16):
        sel = np.flatnonzero(k["M"] == M)[:400]
        for i0 in sel[:3]:
            p = _params(k, i0, kind)
            kk = dict(k, window=np.full(n, p["window"], np.int32), reservoir=np.full(n, p["reservoir"]),
                      cushion=np.full(n, p["cushion"]), safety=np.full(n, p["safety"]), bola_v=np.full(n, p["v"]),
                      bola_gp=np.full(n, p["gp"]))
            g = _run(H, kind, {x: (v[sel] if x not in ("h",) else v[sel]) for x, v in kk.items()})
            w = rule_vec(p, k["c"][sel], k["B"][sel], k["h"][sel].T, k["br"][sel][:, :M], k["u"][sel][:, :M])
            assert np.array_equal(g, w), (kind, M)
    # the knife edges occurred and both sides of the branches were taken
    assert len(set(got.tolist())) > 3


def test_knife_edges_take_the_contract_branch(H):
    """B == r gives 0; B == r + k gives M-1; X == a rung takes that rung; tied BOLA scores take the first index."""
    base = dict(window=np.array([3], np.int32), reservoir=np.array([5.0]), cushion=np.array([10.0]),
                safety=np.array([1.0]), bola_v=np.array([1.0]), bola_gp=np.array([0.0]), c=np.array([4], np.int32),
                M=np.array([4], np.int32), h=np.full((1, HMAX), 2.0))
    br = np.zeros((1, 16))
    br[0, :4] = [1.0, 2.0, 3.0, 4.0]
    u = np.zeros((1, 16))
    assert _run(H, BUFFER, dict(base, B=np.array([5.0]), br=br, u=u))[0] == 0
    assert _run(H, BUFFER, dict(base, B=np.array([15.0]), br=br, u=u))[0] == 3
    assert _run(H, BUFFER, dict(base, B=np.array([10.0]), br=br, u=u))[0] == 1       # X = 1 + 0.5 * 3 = 2.5
    assert _run(H, RATE, dict(base, B=np.array([0.0]), br=br, u=u))[0] == 1          # X = 2.0 exactly: rung 1
    assert _run(H, RATE, dict(base, c=np.array([0], np.int32), B=np.array([0.0]), br=br, u=u))[0] == 0
    br2 = br.copy()
    br2[0, :4] = [1.0, 2.0, 2.0, 4.0]
    u2 = np.zeros((1, 16))
    u2[0, :4] = [0.0, 3.0, 3.0, 0.0]
    assert _run(H, BOLA, dict(base, B=np.array([0.0]), br=br2, u=u2))[0] == 1         # scores 0, 1.5, 1.5, 0


def test_rule_struct_layout_matches_header():
    from abrsimulator_amd import _lib
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_rule_config), offsetof(abr_rule_config, kind),
         offsetof(abr_rule_config, window), offsetof(abr_rule_config, reservoir), offsetof(abr_rule_config, cushion),
         offsetof(abr_rule_config, safety), offsetof(abr_rule_config, bola_v), offsetof(abr_rule_config, bola_gp),
         offsetof(abr_rule_config, utility_dev));
  printf("%d %d %d\n", ABR_RULE_BUFFER, ABR_RULE_RATE, ABR_RULE_BOLA);
  return 0;
}'''
    out = c_abi_output(prog)
    R = _lib.RuleConfig
    assert list(map(int, out[0].split())) == [C.sizeof(R), R.kind.offset, R.window.offset, R.reservoir.offset,
                                              R.cushion.offset, R.safety.offset, R.bola_v.offset, R.bola_gp.offset,
                                              R.utility_dev.offset]
    assert list(map(int, out[1].split())) == [_lib.RULE_BUFFER, _lib.RULE_RATE, _lib.RULE_BOLA]


def _rc(**kw):
    from abrsimulator_amd import _lib
    c = _lib.RuleConfig()
    c.kind, c.window, c.reservoir, c.cushion, c.safety, c.bola_v, c.bola_gp = 1, 5, 5.0, 10.0, 1.0, 1.0, 5.0
    c.utility_dev = 256
    for k, v in kw.items():
        setattr(c, k, v)
    return c


BAD_RULES = [dict(kind=0), dict(kind=4), dict(kind=1, reservoir=float("nan")), dict(kind=2, safety=float("inf")),
             dict(kind=3, bola_gp=float("nan")), dict(kind=1, reservoir=-1.0), dict(kind=1, cushion=0.0),
             dict(kind=1, cushion=-2.0), dict(kind=2, window=0), dict(kind=2, window=-3), dict(kind=2, safety=0.0),
             dict(kind=3, bola_v=0.0), dict(kind=3, bola_v=-1.0), dict(kind=3, utility_dev=None)]


@pytest.mark.parametrize("bad", BAD_RULES, ids=[str(b) for b in BAD_RULES])
def test_rule_validation_before_the_handle(bad):
    """Every bad config answers ABR_E_INVALID with a message that names it, with a NULL handle: nothing is launched and
    no GPU is touched."""
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    one = C.c_void_p(256)
    assert lib.abr_env_step_rule(None, C.byref(_rc(**bad)), 4, None, None, None, None, None) == -1
    msg = lib.abr_last_error().decode()
    assert "NULL" not in msg and "env" not in msg, msg
    assert lib.abr_env_rule_select(None, C.byref(_rc(**bad)), one, None) == -1
    assert "env" not in lib.abr_last_error().decode()


def test_rule_validation_n_steps_and_good_configs_reach_the_handle():
    from abrsimulator_amd import _lib
    lib = _lib.lib()
    assert lib.abr_env_step_rule(None, C.byref(_rc()), 0, None, None, None, None, None) == -1
    assert "n_steps" in lib.abr_last_error().decode()
    assert lib.abr_env_step_rule(None, None, 4, None, None, None, None, None) == -1
    for kind in (1, 2, 3):             # a valid config gets as far as the handle
        assert lib.abr_env_step_rule(None, C.byref(_rc(kind=kind)), 4, None, None, None, None, None) == -1
        assert "env is NULL" in lib.abr_last_error().decode()
        assert lib.abr_env_rule_select(None, C.byref(_rc(kind=kind)), C.c_void_p(256), None) == -1
        assert "NULL" in lib.abr_last_error().decode()


class _Stub:
    def __init__(self, mpd):
        self.mpd = mpd

    def get_mpd(self):
        return self.mpd


def test_controller_defaults_and_errors():
    import math

    import abrsimulator_amd as A
    mpd = A.MPD(10, 4.0, 20.0, 8.0, A.Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))
    p = _Stub(mpd)
    b = A.BufferBasedController(p)
    assert (b.reservoir, b.cushion) == (5.0, 10.0)
    c = b.config()
    assert (c.kind, c.reservoir, c.cushion) == (1, 5.0, 10.0)
    assert A.BufferBasedController(p, reservoir=0.0, cushion=3.0).config().cushion == 3.0
    for kw in (dict(reservoir=-1.0), dict(cushion=0.0), dict(cushion=float("nan"))):
        with pytest.raises(ValueError):
            A.BufferBasedController(p, **kw)
    r = A.RateBasedController(p)
    assert (r.window, r.safety) == (5, 1.0) and (r.config().kind, r.config().window) == (2, 5)
    for kw in (dict(window=0), dict(window=2.5), dict(safety=0.0), dict(safety=-1.0)):
        with pytest.raises(ValueError):
            A.RateBasedController(p, **kw)
    bo = A.BolaController(p)
    assert bo.gamma_p == 5.0 and bo.v == (20.0 - 4.0) / (math.log(4.3 / 0.3) + 5.0)
    assert bo.utility.shape == (10, 6) and bo.utility.dtype == np.float64
    assert np.array_equal(bo.utility[3], np.log(np.array([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]) / 0.3))
    assert A.BolaController(p, gamma_p=2.0, v=3.0).v == 3.0
    with pytest.raises(ValueError):
        A.BolaController(_Stub(A.MPD(10, 4.0, 4.0, 0.0, A.Chunk([1.0, 2.0]))))        # max_buffer <= chunk_length
    assert A.BolaController(_Stub(A.MPD(10, 4.0, 4.0, 0.0, A.Chunk([1.0, 2.0]))), v=1.0).v == 1.0
    with pytest.raises(ValueError):
        A.BolaController(p, v=0.0)
    # a per-chunk MPD: the utility follows each chunk's own ladder
    vbr = A.MPD(3, 4.0, 20.0, 0.0, [A.Chunk([1.0, 2.0]), A.Chunk([2.0, 8.0]), A.Chunk([1.0, 3.0])])
    assert np.array_equal(A.BolaController(_Stub(vbr)).utility[:, 1], np.log([2.0, 4.0, 3.0]))


def _product_asm():
    """The product's ISA (`make asm`: abrsimulator_amd/csrc/abr_env.s), regenerated when older than its sources; skips
    without hipcc."""
    src = os.path.join(ROOT, "abrsimulator_amd", "csrc")
    asm = os.path.join(src, "abr_env.s")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".hip", ".h"))]
    deps.append(os.path.join(ROOT, "include", "abr_env.h"))
    if not os.path.exists(asm) or os.path.getmtime(asm) < max(os.path.getmtime(d) for d in deps):
        if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("no hipcc here: the ISA cannot be regenerated")
        subprocess.run(["make", "-C", src, "-s", "asm"], check=True, capture_output=True, timeout=600)
    return open(asm).read()


def test_mode4_instances_have_no_scratch_and_no_calls():
    """make asm: env_jump_kernel<4>, env_advance_kernel<4> and rule_select_kernel exist with a 0 B private segment and no
    calls."""
    text = _product_asm()
    found = set()
    for name, desc in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        k = re.search(r"env_(jump|advance)_kernelILi4E|rule_select_kernel", name)
        if not k:
            continue
        found.add(k.group(1) or "select")
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1)) == 0, name
        body = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M).group(0)
        assert "s_swappc" not in body and "s_setpc" not in body, name
    assert found == {"jump", "advance", "select"}


def test_mpc_case_table_covers_every_compiled_search_instance():
    """tests/mpc_matrix.py: the mpc_select_kernel<H, BC, WVM> instances the case table dispatches to (launch_mpc's rule
    as data) are exactly the ones compiled -- 52 today.  An instance added to the dispatch, or a case dropped from the
    table, fails here until the GPU parity tests (test_mpc_instances_gpu.py) run it."""
    from mpc_matrix import MPC_CASES, isa_instances, mpc_instance
    compiled = isa_instances(_product_asm())
    covered = {mpc_instance(B, H, wv) for B, H, wv in MPC_CASES}
    assert covered == compiled, (sorted(compiled - covered), sorted(covered - compiled))
    assert len(compiled) == 52
