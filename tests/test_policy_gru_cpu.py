"""The recurrent policy without a GPU: the ABI of abr_policy_gru, the refusals that come before the handle, the
controller's refusals and blob layout, sig_c / tanh_c and policy_gru_forward of the host build (tests/native/
policy_gru_harness.cpp, the kernel's own header) against the numpy twin (tests/policy_gru_twin.py) bit for bit, the
header's absolute-error bounds against float64, and the twin against torch.nn.GRUCell."""
import ctypes as C

import numpy as np
import pytest

import policy_gru_twin as GT
from helpers import c_abi_output, native_harness

f32 = np.float32
FP = C.POINTER(C.c_float)
E_INVALID = -1            # ABR_E_INVALID


@pytest.fixture(scope="module")
def L():
    from abrsimulator_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def nat():
    return native_harness("policy_gru_harness")


def _fp(a):
    return a.ctypes.data_as(FP) if a is not None else None


def _bits_eq(u, v):
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    return ((u.view(np.uint32) == v.view(np.uint32)) | (np.isnan(u) & np.isnan(v))).all()


# ---------------------------------------------------------------------------------------------------------------------
# the ABI

def test_gru_struct_layout_matches_header(L):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "abr_env.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(abr_policy_gru), offsetof(abr_policy_gru, window),
         offsetof(abr_policy_gru, hidden), offsetof(abr_policy_gru, weights_dev), offsetof(abr_policy_gru, weights_bytes),
         offsetof(abr_policy_gru, norm_dev), offsetof(abr_policy_gru, state_dev), offsetof(abr_policy_gru, state_bytes),
         offsetof(abr_policy_gru, seed), offsetof(abr_policy_gru, explore_threshold), offsetof(abr_policy_gru, reserved_));
  printf("%d %d\n", ABR_POLICY_GRU_MAX_HIDDEN, ABR_ABI_VERSION);
  return 0;
}'''
    out = c_abi_output(prog)
    P = L.PolicyGru
    got = list(map(int, out[0].split()))
    assert got == [C.sizeof(P), P.window.offset, P.hidden.offset, P.weights_dev.offset, P.weights_bytes.offset,
                   P.norm_dev.offset, P.state_dev.offset, P.state_bytes.offset, P.seed.offset,
                   P.explore_threshold.offset, P.reserved_.offset]
    assert got[0] == 80
    assert list(map(int, out[1].split())) == [L.POLICY_GRU_MAX_HIDDEN, L.ABI_VERSION] and L.ABI_VERSION == 4


def test_gru_weights_bytes(L):
    lib = L.lib()
    n = C.c_size_t()
    for W, H, M in ((0, 1, 1), (8, 32, 6), (8, 64, 6), (16, 64, 16), (3, 7, 5), (16, 33, 1)):
        p = L.PolicyGru()
        p.window, p.hidden = W, H
        assert lib.abr_policy_gru_weights_bytes(C.byref(p), M, C.byref(n)) == 0
        F = 4 + W + M
        assert n.value == 4 * (3 * H * F + 3 * H * H + 6 * H + M * H + M), (W, H, M)
    p = L.PolicyGru()
    p.window, p.hidden = 16, 64
    assert lib.abr_policy_gru_weights_bytes(C.byref(p), 16, C.byref(n)) == 0 and n.value == 82496
    for W, H, M in ((-1, 8, 6), (17, 8, 6), (8, 0, 6), (8, 65, 6), (8, 8, 0), (8, 8, 17)):
        p = L.PolicyGru()
        p.window, p.hidden = W, H
        assert lib.abr_policy_gru_weights_bytes(C.byref(p), M, C.byref(n)) == E_INVALID, (W, H, M)
    assert lib.abr_policy_gru_weights_bytes(None, 6, C.byref(n)) == E_INVALID
    assert lib.abr_policy_gru_weights_bytes(C.byref(p), 6, None) == E_INVALID


def _good(L, buf):
    p = L.PolicyGru()
    p.window, p.hidden = 8, 32
    p.weights_dev = p.state_dev = C.addressof(buf)
    p.weights_bytes = p.state_bytes = 4
    return p


def test_refusals_before_the_handle(L):
    """Every check of the structs and of the outputs that need an absent struct fails with ABR_E_INVALID while env is
    still NULL (a call that passed them would fail on the NULL handle with the same code, so each case is paired with
    the message)."""
    lib = L.lib()
    buf = (C.c_double * 4)()
    base = C.addressof(buf)

    def msg():
        return lib.abr_last_error().decode()

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

    def select(p, s=None, v=None, probs=None, value=None):
        return lib.abr_env_policy_select_gru(None, C.byref(p) if p is not None else None,
                                             C.byref(s) if s is not None else None,
                                             C.byref(v) if v is not None else None, 0, base, None, None, probs, value,
                                             None, None)

    def step(p, s=None, v=None, n=1, probs=None, values=None, last=None):
        return lib.abr_env_step_policy_gru(None, C.byref(p) if p is not None else None,
                                           C.byref(s) if s is not None else None,
                                           C.byref(v) if v is not None else None, n, None, None, None, None, None, None,
                                           probs, values, last, None, None)

    # a good call reaches the handle
    assert select(_good(L, buf)) == E_INVALID and "env" in msg()
    assert step(_good(L, buf)) == E_INVALID and "env is NULL" in msg()
    cases = []
    for field, value, word in (("window", -1, "window"), ("window", 17, "window"), ("hidden", 0, "hidden"),
                               ("hidden", 65, "hidden"), ("weights_dev", None, "weights"),
                               ("weights_dev", base + 2, "weights"), ("norm_dev", base + 4, "norm"),
                               ("state_dev", None, "state"), ("state_dev", base + 1, "state"),
                               ("explore_threshold", (1 << 32) + 1, "explore_threshold")):
        p = _good(L, buf)
        setattr(p, field, value)
        cases.append((p, word))
    p = _good(L, buf)
    p.reserved_[3] = 1
    cases.append((p, "reserved_"))
    for p, word in cases:
        for call in (select, step):
            assert call(p) == E_INVALID and word in msg(), (word, msg())
    for call in (select, step):
        assert call(None) == E_INVALID and "policy is NULL" in msg()
        for s, word in ((smp(mode=2), "mode"), (smp(it=0.0), "inv_temperature"), (smp(it=float("inf")), "inv_temperature"),
                        (smp(it=float("nan")), "inv_temperature"), (smp(r=1), "reserved_")):
            assert call(_good(L, buf), s=s) == E_INVALID and word in msg(), (word, msg())
        for v, word in ((val(head=None), "head"), (val(head=base + 2), "head"), (val(r=1), "reserved_")):
            assert call(_good(L, buf), v=v) == E_INVALID and word in msg(), (word, msg())
        assert call(_good(L, buf), probs=base) == E_INVALID and "probs need" in msg()
    assert select(_good(L, buf), value=base) == E_INVALID and "values need" in msg()
    assert step(_good(L, buf), values=base) == E_INVALID and "values need" in msg()
    assert step(_good(L, buf), last=base) == E_INVALID and "values need" in msg()
    for n in (0, -3):
        assert step(_good(L, buf), n=n) == E_INVALID and "n_steps" in msg()
    # with the structs in place the same outputs pass on to the handle
    assert select(_good(L, buf), s=smp(1, 0.5), v=val(), probs=base, value=base) == E_INVALID and "env" in msg()
    assert step(_good(L, buf), s=smp(), v=val(), probs=base, values=base, last=base) == E_INVALID and "env is NULL" in msg()


# ---------------------------------------------------------------------------------------------------------------------
# the controller

class _Player:
    env = None

    def get_mpd(self):
        from abrsimulator_amd.datamodel import MPD, Chunk
        return MPD(10, 4.0, 20.0, 4.0, Chunk([0.3, 0.75, 1.2, 1.85, 2.85, 4.3]))


def test_controller_refusals():
    torch = pytest.importorskip("torch")
    import abrsimulator_amd as A
    nn = torch.nn
    F, M, H = 4 + 8 + 6, 6, 16
    good_cell, good_head = nn.GRUCell(F, H), nn.Linear(H, M)
    z = np.zeros
    bad = [(nn.LSTMCell(F, H), good_head), (nn.GRU(F, H), good_head), (nn.RNNCell(F, H), good_head),
           (nn.GRUCell(F, H, bias=False), good_head), (nn.GRUCell(F + 1, H), good_head), (nn.GRUCell(F, 65), nn.Linear(65, M)),
           (good_cell, nn.Linear(H, M + 1)), (good_cell, nn.Linear(H + 1, M)), (good_cell, nn.Linear(H, M, bias=False)),
           (good_cell, nn.Sequential(nn.Linear(H, M))), (nn.Linear(F, H), good_head), (good_cell, None), (None, good_head),
           ((z((3 * H, F)), z((3 * H, H)), z(3 * H)), good_head),                    # three tensors
           ((z((3 * H, F)), z((3 * H, H)), z(3 * H), z(2 * H)), good_head),          # a short bias
           ((z((2 * H, F)), z((3 * H, H)), z(3 * H), z(3 * H)), good_head),          # two gates
           ((z((0, F)), z((0, 0)), z(0), z(0)), (z((M, 0)), z(M))),                  # H = 0
           (good_cell, (z((H, M)), z(M)))]                                           # a transposed head
    for cell, head in bad:
        with pytest.raises(ValueError):
            A.RecurrentPolicyController(_Player(), cell, head, window=8, device="cpu")
    for w in (-1, 17, 2.5, True):
        with pytest.raises(ValueError):
            A.RecurrentPolicyController(_Player(), nn.GRUCell(4 + 6, H), good_head, window=w, device="cpu")
    for kw in (dict(explore=1.5), dict(sample="greedy"), dict(temperature=0.0), dict(norm="other"),
               dict(value_head=nn.Linear(H + 1, 1)), dict(value_head=nn.Linear(H, 2))):
        with pytest.raises(ValueError):
            A.RecurrentPolicyController(_Player(), good_cell, good_head, window=8, device="cpu", **kw)
    # the other front ends refuse the recurrent policy by name
    with pytest.raises(ValueError, match="recurrent"):
        A.PolicyPopulation(_Player(), [good_cell], group=256)
    with pytest.raises(ValueError):
        A.PolicyController.from_module(_Player(), good_cell)

    class Sharded:
        pass
    Sharded.__name__ = "ShardedABREnv"
    pl = _Player()
    pl.env = Sharded()
    with pytest.raises(ValueError, match="ShardedABREnv"):
        A.RecurrentPolicyController(pl, good_cell, good_head, window=8, device="cpu")


def test_blob_is_the_cells_parameters_concatenated():
    torch = pytest.importorskip("torch")
    from abrsimulator_amd.policy import pack_gru
    torch.manual_seed(3)
    F, H, M = 18, 7, 6
    cell, head = torch.nn.GRUCell(F, H), torch.nn.Linear(H, M)
    blob = pack_gru((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), (head.weight, head.bias))
    want = np.concatenate([p.detach().numpy().ravel() for p in list(cell.parameters()) + list(head.parameters())])
    assert [n for n, _ in cell.named_parameters()] == ["weight_ih", "weight_hh", "bias_ih", "bias_hh"]
    assert blob.dtype == np.float32 and np.array_equal(blob, want)
    parts = GT.split_blob(blob, F, H, M)
    assert np.array_equal(parts[0], cell.weight_ih.detach().numpy()) and np.array_equal(parts[5], head.bias.detach().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# the activations

def _grid():
    """At least 2^20 float32 over [-90, 90]: a dense linear sweep, every binade boundary and its neighbours, subnormals,
    both zeros, the +-40 and +-80 edges with their neighbours, the infinities and NaNs of both signs."""
    lin = np.linspace(-90.0, 90.0, (1 << 20) + 1).astype(f32)
    e = np.arange(-149, 7)
    b = np.ldexp(1.0, e).astype(f32)
    b = np.concatenate([b, np.nextafter(b, f32(0)), np.nextafter(b, f32(np.inf))])
    edges = np.array([40.0, 80.0, 90.0, 0.5 * np.log(2.0), np.log(2.0), 1.0], f32)
    edges = np.concatenate([edges, np.nextafter(edges, f32(0)), np.nextafter(edges, f32(np.inf))])
    rng = np.random.default_rng(5)
    rnd = (rng.standard_normal(1 << 18) * np.exp(rng.uniform(-12, 4.4, 1 << 18))).astype(f32)
    pos = np.concatenate([b[b <= 90], edges, [f32(0.0), f32(np.inf), f32(np.nan)]]).astype(f32)
    return np.concatenate([lin, rnd[np.abs(rnd) <= 90], pos, -pos]).astype(f32)


def test_activations_host_equals_twin_bit_for_bit(nat):
    x = _grid()
    assert x.size >= 1 << 20
    for fn, twin in ((nat.pg_sig, GT.sig_c), (nat.pg_tanh, GT.tanh_c)):
        got = np.empty_like(x)
        fn(C.c_int64(x.size), _fp(x), _fp(got))
        want = twin(x)
        bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), (x[bad][:8], got[bad][:8], want[bad][:8])
    # the stated special values
    t = GT.tanh_c(np.array([0.0, -0.0, 40.5, -40.5, np.inf, -np.inf, 90.0], f32))
    assert np.array_equal(t.view(np.uint32), np.array([0.0, -0.0, 1, -1, 1, -1, 1], f32).view(np.uint32))
    s = GT.sig_c(np.array([0.0, -0.0, 81.0, -81.0, np.inf, -np.inf], f32))
    assert np.array_equal(s.view(np.uint32), np.array([0.5, 0.5, 1, 0, 1, 0], f32).view(np.uint32))
    nan = np.array([np.nan, -np.nan], f32)
    assert _bits_eq(GT.sig_c(nan), nan) and _bits_eq(GT.tanh_c(nan), nan)


def test_activation_absolute_error_bounds_against_float64(capsys):
    """The bounds derived in include/abr_env.h (abr_policy_gru): |sig_c - sigmoid| <= 2^-23 and |tanh_c - tanh| <=
    3 * 2^-24, each times 1 + 2^-20 for the second-order terms.  Monotonicity is not assumed: the maximum is taken over
    the whole grid."""
    x = _grid()
    x = x[np.isfinite(x)]
    x64 = x.astype(np.float64)
    slack = 1.0 + 2.0 ** -20
    with np.errstate(all="ignore"):
        sig = np.where(x64 >= 0, 1.0 / (1.0 + np.exp(-np.abs(x64))), np.exp(-np.abs(x64)) / (1.0 + np.exp(-np.abs(x64))))
    es = np.abs(GT.sig_c(x).astype(np.float64) - sig).max()
    et = np.abs(GT.tanh_c(x).astype(np.float64) - np.tanh(x64)).max()
    with capsys.disabled():
        print(f"\nsig_c max abs error {es:.4g} ({es / 2.0 ** -23:.3f} * 2^-23); "
              f"tanh_c max abs error {et:.4g} ({et / (3 * 2.0 ** -24):.3f} * 3 * 2^-24) on {x.size} points")
    assert es <= 2.0 ** -23 * slack
    assert et <= 3 * 2.0 ** -24 * slack


# ---------------------------------------------------------------------------------------------------------------------
# the forward pass

def _random_blob(rng, F, H, M, special):
    n = 3 * H * (F + H + 2) + M * (H + 1)
    w = (rng.standard_normal(n) * 0.5).astype(f32)
    if special:
        pool = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -3e-42, 1e30, -1e30, 6e-39], f32)
        k = rng.random(n) < 0.02
        w[k] = rng.choice(pool, int(k.sum()))
    return w


def _host_forward(nat, W, H, M, blob, head, x, h):
    n = x.shape[1]
    xi, hi = np.ascontiguousarray(x.T), np.ascontiguousarray(h.T)
    hp, s = np.empty((n, H), f32), np.empty((n, M), f32)
    g, v = np.empty(n, np.int32), np.empty(n, f32)
    nat.pg_forward(C.c_int64(n), W, H, M, _fp(blob), _fp(head), _fp(xi), _fp(hi), _fp(hp), _fp(s),
                   g.ctypes.data_as(C.POINTER(C.c_int32)), _fp(v))
    return hp.T, s.T, g, v


def test_padded_layout_holds_the_blob_and_signed_pads(nat):
    rng = np.random.default_rng(11)
    for W, H, M in ((8, 5, 6), (16, 64, 16), (0, 1, 1)):
        F = 4 + W + M
        blob = rng.uniform(1.0, 2.0, 3 * H * (F + H + 2) + M * (H + 1)).astype(f32)      # no zero, so pads stand out
        head = rng.uniform(1.0, 2.0, H + 1).astype(f32)
        for hd in (None, head):
            total = nat.pg_layout_total(W, H, M, int(hd is not None))
            assert total == H * 324 + 16 + (68 if hd is not None else 0)
            out = np.empty(total, f32)
            nat.pg_padded(W, H, M, _fp(blob), _fp(hd), _fp(out))
            real = out[out != 0]
            assert real.size == blob.size + (H + 1 if hd is not None else 0)
            assert np.array_equal(np.sort(real), np.sort(np.concatenate([blob, hd if hd is not None else []]).astype(f32)))
            G = out[:H * 300].reshape(H, 3, 100)
            Wih, Whh = GT.split_blob(blob, F, H, M)[:2]
            for g in range(3):
                assert np.array_equal(G[:, g, :F], Wih[g * H:(g + 1) * H]) and np.array_equal(G[:, g, 36:36 + H], Whh[g * H:(g + 1) * H])
            pads = np.concatenate([G[:, :, F:36].ravel(), G[:, :, 36 + H:].ravel()])
            assert (pads.view(np.uint32) == 0x80000000).all()                        # weights pad with -0


@pytest.mark.parametrize("H", [1, 2, 7, 33, 64])
def test_host_forward_equals_twin_bit_for_bit(nat, H):
    rng = np.random.default_rng(100 + H)
    n = 24
    for W in (0, 8, 16):
        for M in (1, 6, 16):
            F = 4 + W + M
            for special in (False, True):
                blob = _random_blob(rng, F, H, M, special)
                head = rng.standard_normal(H + 1).astype(f32)
                if special:
                    head[rng.integers(H + 1)] = rng.choice(np.array([np.nan, np.inf, -0.0, 1e-40], f32))
                x = rng.standard_normal((F, n)).astype(f32)
                h = np.tanh(rng.standard_normal((H, n))).astype(f32)
                if special:
                    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-41, -2e-39, 1e20], f32)
                    h[rng.random(h.shape) < 0.05] = rng.choice(pool)
                    x[rng.random(x.shape) < 0.03] = rng.choice(pool)
                    h[:, 0] = 0.0                                                     # a fresh episode's state
                parts = GT.split_blob(blob, F, H, M)
                s, hp, v = GT.forward(parts, x, h, head)
                for hd in (None, head):
                    ghp, gs, gg, gv = _host_forward(nat, W, H, M, blob, hd, x, h)
                    assert _bits_eq(ghp, hp), (W, H, M, special)
                    assert _bits_eq(gs, s), (W, H, M, special)
                    assert np.array_equal(gg, GT.T.argmax_first(s)), (W, H, M, special)
                    if hd is not None:
                        assert _bits_eq(gv, v), (W, H, M, special)


def test_twin_against_torch_grucell():
    """The twin's h' against torch.nn.GRUCell in float64 on 4 096 random (x, h) at H = 64.  The cell is float32 arithmetic
    in another order and with other activations than torch's float32 kernel, so its bound is a small multiple (4x) of
    the distance float32 GRUCell itself shows from float64 on the same inputs."""
    torch = pytest.importorskip("torch")
    torch.manual_seed(7)
    F, H, M, n = 18, 64, 6, 4096
    cell = torch.nn.GRUCell(F, H)
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, F)).astype(f32)
    h = np.tanh(rng.standard_normal((n, H))).astype(f32)
    with torch.no_grad():
        ref32 = cell(torch.from_numpy(x), torch.from_numpy(h)).numpy().astype(np.float64)
        c64 = torch.nn.GRUCell(F, H).double()
        c64.load_state_dict({k: v.double() for k, v in cell.state_dict().items()})
        ref64 = c64(torch.from_numpy(x).double(), torch.from_numpy(h).double()).numpy()
    parts = [p.detach().numpy() for p in cell.parameters()] + [np.zeros((M, H), f32), np.zeros(M, f32)]
    hp = GT.cell(parts, x.T, h.T).T.astype(np.float64)
    e_torch, e_twin = np.abs(ref32 - ref64).max(), np.abs(hp - ref64).max()
    print(f"float32 GRUCell vs float64: {e_torch:.4g}; twin vs float64: {e_twin:.4g}")
    assert e_torch > 0
    assert e_twin <= 4 * e_torch, (e_twin, e_torch)
