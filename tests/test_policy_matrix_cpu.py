"""The matrix engine of the learned policy without a GPU (include/abr_env.h: abr_policy_mx): the ABI struct, the size
query and every refusal before the handle; the controller's engine keyword; and the engine's index maps
(csrc/abr_lane_jump.h: mx_*) compiled for the host -- bijections, and a whole layer chain packed into the operands of an
emulated v_mfma_f32_32x32x2_f32 and unpacked again through them, against the numpy twin bit for bit.  The emulation takes
the instruction's lane maps and its k order from the programming guide; that the hardware follows them is what
tests/test_policy_matrix_gpu.py checks."""
import ctypes as C

import numpy as np
import pytest

from helpers import c_abi_output, native_harness
import actor_critic_twin as AC
import policy_twin as T
from test_policy_cpu import _layers, same_bits

P_ = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


@pytest.fixture(scope="module")
def MH():
    h = native_harness("policy_matrix_harness")
    h.pm_index.restype = C.c_int32
    h.pm_index.argtypes = [C.c_int32] * 3
    h.pm_lds_floats.restype = h.pm_score_offset.restype = C.c_int32
    return h


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.build()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def test_struct_layout_matches_header(L):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_policy_mx), offsetof(abr_policy_mx, window),
         offsetof(abr_policy_mx, n_hidden), offsetof(abr_policy_mx, width), offsetof(abr_policy_mx, weights_dev),
         offsetof(abr_policy_mx, weights_bytes), offsetof(abr_policy_mx, norm_dev), offsetof(abr_policy_mx, seed),
         offsetof(abr_policy_mx, explore_threshold), offsetof(abr_policy_mx, reserved_));
  printf("%d %d %d %d\n", ABR_POLICY_MX_MAX_HIDDEN, ABR_POLICY_MX_MAX_WIDTH, ABR_ABI_VERSION,
         (int)(sizeof(((abr_policy_mx *)0)->width) / sizeof(int32_t)));
  return 0;
}'''
    out = c_abi_output(prog)
    P = L.PolicyMx
    got = list(map(int, out[0].split()))
    assert got == [C.sizeof(P), P.window.offset, P.n_hidden.offset, P.width.offset, P.weights_dev.offset,
                   P.weights_bytes.offset, P.norm_dev.offset, P.seed.offset, P.explore_threshold.offset,
                   P.reserved_.offset]
    assert got[0] == 80
    assert list(map(int, out[1].split())) == [L.POLICY_MX_MAX_HIDDEN, L.POLICY_MX_MAX_WIDTH, 4, 4]
    assert L.ABI_VERSION == 4 and L.lib().abr_abi_version() == 4
    names = [s[0] for s in L.SYMBOLS]
    for sym in ("abr_policy_mx_weights_bytes", "abr_env_policy_select_mx", "abr_env_step_policy_mx"):
        assert sym in names


def _pol(L, **kw):
    p = L.PolicyMx()
    p.window, p.n_hidden = 8, 3
    p.width[0], p.width[1], p.width[2] = 128, 128, 128
    p.weights_dev, p.weights_bytes, p.seed = 4096, 100, 1
    for k, v in kw.items():
        if k == "width":
            for j in range(4):
                p.width[j] = v[j] if j < len(v) else 0
        elif k == "reserved":
            p.reserved_[v] = 1
        else:
            setattr(p, k, v)
    return p


def _lane_pol(L, window, widths):
    p = L.Policy()
    p.window, p.n_hidden = window, len(widths)
    for j, w in enumerate(widths):
        p.width[j] = w
    return p


def test_size_query(L):
    lib = L.lib()
    b, b2 = C.c_size_t(), C.c_size_t()
    assert lib.abr_policy_mx_weights_bytes(C.byref(_pol(L, window=16)), 16, C.byref(b)) == 0
    assert b.value == 159296                                              # the largest blob: 3 x 128 at W 16, M 16
    assert b.value == 4 * (128 * 36 + 128 + 2 * (128 * 128 + 128) + 16 * 128 + 16)
    for window, widths, M in ((8, [64, 64], 6), (0, [], 1), (16, [1], 16), (3, [64, 1], 8), (5, [33], 2)):
        mx = _pol(L, window=window, n_hidden=len(widths), width=widths)
        assert lib.abr_policy_mx_weights_bytes(C.byref(mx), M, C.byref(b)) == 0
        assert lib.abr_policy_weights_bytes(C.byref(_lane_pol(L, window, widths)), M, C.byref(b2)) == 0
        assert b.value == b2.value > 0, (window, widths, M)
    assert lib.abr_policy_mx_weights_bytes(C.byref(_pol(L, weights_dev=None)), 6, C.byref(b)) == 0   # no look at pointers
    for m in (0, 17):
        assert lib.abr_policy_mx_weights_bytes(C.byref(_pol(L)), m, C.byref(b)) == -1
    assert lib.abr_policy_mx_weights_bytes(C.byref(_pol(L)), 6, None) == -1
    assert lib.abr_policy_mx_weights_bytes(None, 6, C.byref(b)) == -1
    for kw in (dict(n_hidden=4), dict(width=(0, 128, 128)), dict(width=(129, 128, 128)), dict(window=17)):
        assert lib.abr_policy_mx_weights_bytes(C.byref(_pol(L, **kw)), 6, C.byref(b)) == -1, kw


STRUCT_REFUSALS = [dict(window=-1), dict(window=17), dict(n_hidden=-1), dict(n_hidden=4), dict(width=(0, 128, 128)),
                   dict(width=(128, 129, 128)), dict(width=(128, 128, 0)), dict(n_hidden=2, width=(128, 128, 128)),
                   dict(n_hidden=0, width=(8,)), dict(width=(128, 128, 128, 1)), dict(reserved=0), dict(reserved=3),
                   dict(weights_dev=None), dict(weights_dev=4098), dict(norm_dev=4100),
                   dict(explore_threshold=2 ** 32 + 1), dict(explore_threshold=2 ** 64 - 1)]


def _select(lib, env, pol, smp, val, probs=None, value=None, act=8192):
    return lib.abr_env_policy_select_mx(env, pol, smp, val, C.c_void_p(act), None, None, probs, value, None)


def _step(lib, env, pol, smp, val, n=4, probs=None, values=None, last=None):
    return lib.abr_env_step_policy_mx(env, pol, smp, val, n, None, None, None, None, None, None, probs, values, last, None)


def test_every_refusal_before_the_handle(L):
    lib = L.lib()
    smp = L.PolicySampling()
    smp.mode, smp.inv_temperature = L.POLICY_SOFTMAX, 1.0
    val = L.PolicyValue()
    val.head_dev, val.head_bytes = 4096, 4 * 129
    S, Vv = C.byref(smp), C.byref(val)
    for kw in STRUCT_REFUSALS:
        p = C.byref(_pol(L, **kw))
        for s_, v_ in ((None, None), (S, Vv)):
            assert _select(lib, None, p, s_, v_) == -1, kw
            assert b"policy" in lib.abr_last_error() or b"explore" in lib.abr_last_error(), kw
            assert _step(lib, None, p, s_, v_) == -1, kw
            assert b"policy" in lib.abr_last_error() or b"explore" in lib.abr_last_error(), kw
    assert _select(lib, None, None, None, None) == -1 and b"policy is NULL" in lib.abr_last_error()
    assert _step(lib, None, None, None, None) == -1 and b"policy is NULL" in lib.abr_last_error()
    ok = C.byref(_pol(L))
    ptr = C.c_void_p(8192)
    # a bad sampling or value struct
    for field, v in (("mode", 2), ("inv_temperature", 0.0), ("inv_temperature", float("inf"))):
        bad = L.PolicySampling()
        bad.mode, bad.inv_temperature = L.POLICY_SOFTMAX, 1.0
        setattr(bad, field, v)
        assert _select(lib, None, ok, C.byref(bad), None) == -1 and b"sampling" in lib.abr_last_error()
        assert _step(lib, None, ok, C.byref(bad), None) == -1 and b"sampling" in lib.abr_last_error()
    bad = L.PolicySampling()
    bad.mode, bad.inv_temperature, bad.reserved_[5] = 0, 1.0, 1
    assert _step(lib, None, ok, C.byref(bad), None) == -1 and b"sampling" in lib.abr_last_error()
    for head in (None, 4098):
        bv = L.PolicyValue()
        bv.head_dev, bv.head_bytes = head, 4 * 129
        assert _select(lib, None, ok, S, C.byref(bv)) == -1 and b"value head" in lib.abr_last_error()
        assert _step(lib, None, ok, S, C.byref(bv)) == -1 and b"value head" in lib.abr_last_error()
    bv = L.PolicyValue()
    bv.head_dev, bv.head_bytes, bv.reserved_[0] = 4096, 4 * 129, 1
    assert _step(lib, None, ok, None, C.byref(bv)) == -1 and b"value reserved_" in lib.abr_last_error()
    # outputs that need a struct that is absent
    assert _select(lib, None, ok, None, None, probs=ptr) == -1 and b"probs need" in lib.abr_last_error()
    assert _step(lib, None, ok, None, Vv, probs=ptr) == -1 and b"probs need" in lib.abr_last_error()
    assert _select(lib, None, ok, S, None, value=ptr) == -1 and b"values need" in lib.abr_last_error()
    assert _step(lib, None, ok, S, None, values=ptr) == -1 and b"values need" in lib.abr_last_error()
    assert _step(lib, None, ok, None, None, last=ptr) == -1 and b"values need" in lib.abr_last_error()
    for n in (0, -1):
        for s_, v_ in ((None, None), (S, Vv)):
            assert _step(lib, None, ok, s_, v_, n=n) == -1 and b"n_steps" in lib.abr_last_error()
    # valid structs reach the handle, in every mode and over the whole threshold range
    for s_, v_, kw in ((None, None, {}), (S, None, dict(probs=ptr)), (None, Vv, dict(values=ptr, last=ptr)),
                       (S, Vv, dict(probs=ptr, values=ptr, last=ptr))):
        assert _step(lib, None, ok, s_, v_, n=1, **kw) == -1 and b"env is NULL" in lib.abr_last_error()
        assert _select(lib, None, ok, s_, v_) == -1 and b"NULL argument" in lib.abr_last_error()
    for thr in (0, 1, 2 ** 31, 2 ** 32):
        assert _step(lib, None, C.byref(_pol(L, explore_threshold=thr)), None, None, n=1) == -1
        assert b"env is NULL" in lib.abr_last_error()
    for widths in ((), (1,), (128,), (1, 128), (128, 1, 128)):
        p = C.byref(_pol(L, n_hidden=len(widths), width=widths))
        assert _step(lib, None, p, None, None, n=1) == -1 and b"env is NULL" in lib.abr_last_error(), widths


# ---------------------------------------------------------------------------------------------------------------------
# the controller

class _Player:
    env = None

    def get_mpd(self):
        from abrsimulator_amd.datamodel import MPD, Chunk
        return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))


def _net(nn, F, hidden, M):
    mods, fan = [], F
    for w in hidden:
        mods += [nn.Linear(fan, w), nn.ReLU()]
        fan = w
    return nn.Sequential(*mods, nn.Linear(fan, M))


def test_controller_engine_keyword(L):
    torch = pytest.importorskip("torch")
    from abrsimulator_amd.policy import PolicyController
    nn = torch.nn
    F, M = 4 + 8 + 6, 6
    rng = np.random.default_rng(3)
    layers = _layers(rng, F, [128, 128, 128], M)
    ctl = PolicyController(_Player(), layers, window=8, engine="matrix", device="cpu")
    assert ctl.engine == "matrix" and ctl.widths == [128, 128, 128]
    assert ctl.weights.numel() * 4 == 4 * (128 * F + 128 + 2 * (128 * 128 + 128) + M * 128 + M)
    blob = np.concatenate([np.concatenate([W.ravel(), b]) for W, b in layers])
    assert np.array_equal(ctl.weights.numpy(), blob)
    net = _net(nn, F, [128, 128, 128], M)
    head = nn.Linear(128, 1)
    ctl = PolicyController.from_module(_Player(), net, window=8, engine="matrix", device="cpu", value_head=head)
    assert ctl.engine == "matrix" and ctl.value_head.numel() == 129
    ctl.load_weights(net, value_head=head)                                 # an nn.Sequential of three hidden layers again
    for (W, b), lin in zip(ctl.layers(), list(net)[0::2]):
        assert torch.equal(W, lin.weight.detach()) and torch.equal(b, lin.bias.detach())

    class Env:                                                              # bound() looks at n_rates only
        n_rates = M
    st = ctl.bound(Env())
    assert type(st) is L.PolicyMx and list(st.width) == [128, 128, 128, 0] and st.n_hidden == 3
    assert st.weights_bytes == ctl.weights.numel() * 4 and st.weights_dev == ctl.weights.data_ptr()
    # refusals of the matrix engine
    with pytest.raises(ValueError):
        PolicyController(_Player(), _layers(rng, F, [8, 8, 8, 8], M), window=8, engine="matrix", device="cpu")
    with pytest.raises(ValueError):
        PolicyController(_Player(), _layers(rng, F, [129], M), window=8, engine="matrix", device="cpu")
    with pytest.raises(ValueError):
        PolicyController.from_module(_Player(), _net(nn, F, [8, 8, 8, 8], M), window=8, engine="matrix", device="cpu")
    with pytest.raises(ValueError):
        PolicyController.from_module(_Player(), _net(nn, F, [129], M), window=8, engine="matrix", device="cpu")
    for bad in ("x", "", None, "MATRIX"):
        with pytest.raises(ValueError):
            PolicyController(_Player(), _layers(rng, F, [8], M), window=8, engine=bad, device="cpu")
        with pytest.raises(ValueError):
            PolicyController.from_module(_Player(), _net(nn, F, [8], M), window=8, engine=bad, device="cpu")
    # the default engine is untouched: "lane", its struct, its limits
    ctl = PolicyController(_Player(), _layers(rng, F, [64, 64], M), window=8, device="cpu")
    assert ctl.engine == "lane" and type(ctl.bound(Env())) is L.Policy
    assert PolicyController.from_module(_Player(), _net(nn, F, [64], M), window=8, device="cpu").engine == "lane"
    for hidden in ([65], [8, 8, 8]):
        with pytest.raises(ValueError):
            PolicyController(_Player(), _layers(rng, F, hidden, M), window=8, device="cpu")
        with pytest.raises(ValueError):
            PolicyController.from_module(_Player(), _net(nn, F, hidden, M), window=8, device="cpu", engine="lane")
    # a shape both engines hold: the same blob
    both = _layers(rng, F, [64, 33], M)
    a = PolicyController(_Player(), both, window=8, device="cpu")
    b = PolicyController(_Player(), both, window=8, device="cpu", engine="matrix")
    assert torch.equal(a.weights, b.weights)


# ---------------------------------------------------------------------------------------------------------------------
# the index maps

def test_index_maps_are_bijections(MH):
    ix = MH.pm_index
    rows = [ix(0, u, 0) for u in range(32)]
    assert sorted(rows) == list(range(32))
    assert [ix(1, r, 0) for r in rows] == list(range(32))                  # row_unit inverts unit_row
    # A and B: the 64 lanes cover [32][2] and [2][32] once each
    assert sorted((ix(4, l, 0), ix(5, l, 0)) for l in range(64)) == [(i, k) for i in range(32) for k in range(2)]
    assert sorted((ix(6, l, 0), ix(7, l, 0)) for l in range(64)) == [(k, j) for k in range(2) for j in range(32)]
    # D: (lane, register) covers [32][32] once
    cells = sorted((ix(2, l, r), ix(8, l, 0)) for l in range(64) for r in range(16))
    assert cells == [(i, j) for i in range(32) for j in range(32)]
    # the guide's maps
    for l in range(64):
        assert (ix(4, l, 0), ix(5, l, 0)) == (l & 31, l >> 5) and (ix(6, l, 0), ix(7, l, 0)) == (l >> 5, l & 31)
        for r in range(16):
            assert ix(2, l, r) == (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
            # register r of lane half h holds unit 2 r + h: the next layer's input k of step r, k-slot h
            assert ix(3, l, r) == 2 * r + (l >> 5)
            assert ix(9, ix(3, l, r), 0) == r and ix(10, ix(3, l, r), 0) == l >> 5


def test_lds_budget(MH):
    w = lambda *a: (C.c_int32 * 3)(*a)
    assert MH.pm_lds_floats(36, 16, 3, w(128, 128, 128), 1, 256) * 4 == 65536     # a 128 x 128 layer: all of it
    assert MH.pm_lds_floats(36, 16, 0, w(), 1, 256) == 18 * 64 + 16 * 256
    assert MH.pm_lds_floats(36, 16, 0, w(), 0, 256) == 18 * 64
    for F, M, hid in ((18, 6, [64, 64]), (5, 1, [1]), (36, 16, [128]), (17, 6, [33, 17]), (36, 16, [128, 1, 128])):
        for sampled in (0, 1):
            cap = MH.pm_lds_floats(F, M, len(hid), w(*hid), sampled, 256)
            fan, need = F, 0
            for h in hid:
                need = max(need, -(-h // 32) * ((fan + 1) // 2) * 64)
                fan = h
            off = MH.pm_score_offset(F, len(hid), w(*hid))
            assert off == ((fan + 1) // 2) * 64                            # behind the output layer's one tile
            assert cap == max(need, off + sampled * M * 256) and cap * 4 <= 65536


SHAPES = ([], [1], [31], [33], [65], [128, 1], [17, 64, 5], [128, 128, 128])


def _forward(MH, layers, head, F, M, x):
    n = x.shape[1]
    widths = [W.shape[0] for W, _ in layers[:-1]]
    blob = np.concatenate([np.concatenate([W.ravel(), b]) for W, b in layers]).astype(np.float32)
    hd = np.concatenate([head[0], [head[1]]]).astype(np.float32)
    s, v = np.zeros((n, M), np.float32), np.zeros(n, np.float32)
    MH.pm_forward(C.c_int64(n), C.c_int32(F), C.c_int32(M), C.c_int32(len(widths)), (C.c_int32 * 3)(*widths),
                  P_(blob, C.c_float), P_(hd, C.c_float), P_(np.ascontiguousarray(x.T), C.c_float), P_(s, C.c_float),
                  P_(v, C.c_float))
    s2 = np.zeros((n, M), np.float32)
    MH.pm_forward(C.c_int64(n), C.c_int32(F), C.c_int32(M), C.c_int32(len(widths)), (C.c_int32 * 3)(*widths),
                  P_(blob, C.c_float), None, P_(np.ascontiguousarray(x.T), C.c_float), P_(s2, C.c_float), None)
    assert np.array_equal(s.view(np.uint32), s2.view(np.uint32))           # the head's row feeds nothing back
    return s.T, v


@pytest.mark.parametrize("hidden", SHAPES, ids=lambda h: "x".join(map(str, h)) or "none")
def test_layer_chain_through_the_emulated_instruction_matches_twin(MH, hidden):
    rng = np.random.default_rng(1000 + sum(hidden))
    n = 70                                                                  # a full wave and a partial one
    combos = [(7, 6, False), (8, 6, True), (15, 16, True), (16, 16, False)]  # F = 17, 18, 35, 36
    if sum(hidden) > 200:
        combos = [(8, 6, True), (15, 16, False)]                            # F even with special weights, F odd without
    finite = 0
    for W, M, special in combos:
        F = 4 + W + M
        layers = _layers(rng, F, list(hidden), M, special)
        n_in = hidden[-1] if hidden else F
        hl = _layers(rng, n_in, [], 1, special)[0]
        head = (hl[0][0], hl[1][0])
        x = rng.normal(0, 1, (F, n)).astype(np.float32)
        x[rng.random((F, n)) < 0.02] = np.float32(-0.0)
        x[rng.random((F, n)) < 0.02] = np.float32(1e-42)
        x[:, 5] = np.float32(np.nan)                                        # one lane's NaN stays in its column
        x[3, 40] = np.float32(np.inf)
        s, v = _forward(MH, layers, head, F, M, x)
        want = T.forward(layers, x)
        assert same_bits(s, want), (hidden, F, special)
        assert same_bits(v, AC.value(layers, head, x)), (hidden, F, special)
        if not special:
            finite += int(np.isfinite(want[:, np.isfinite(x).all(0)]).all())
    assert finite >= 1                                                      # plain weights on finite inputs: finite scores
