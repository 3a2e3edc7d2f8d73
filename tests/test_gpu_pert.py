"""GPU: the perturbation check - ee_pert_check_f32 through the C ABI against ops._pert_check_host, its numpy
float64 restatement.

Bit-exact: Linf (a maximum of float32 values), the range and the NaN count against the host; the resident path against the streaming one;
a view 4 bytes past a 16-byte boundary (word-by-word loads) against the aligned call.  In tolerance: L2 and L1, whose double sums the
kernel takes in the scaffold's order and numpy pairwise - at most 2^14 non-negative terms in double carry a relative error below 2^-38, far
under half a float32 ulp, so the emitted float is the correctly rounded value or its neighbour: 1 ulp."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
BATCHES = (1, 3)
SIZES = (1, 5, 2048, 12288, 12289)  # 5: every other row misaligned; 2048: one group per thread; 12288: the resident limit; 12289: past it
RESIDENT = 12288
PATHS = {"auto": 0, "resident": 1, "streaming": 2}


@pytest.fixture(scope="module")
def env():
    from eeadv import _native, ops
    return _native, ops


def _paths(D):
    return ("resident", "streaming") if D <= RESIDENT else ("streaming",)


def _points(B, D, seed=0):
    rng = np.random.default_rng(seed + 31 * B + D)
    x0 = rng.random((B, D)).astype(F32)
    return np.clip(x0 + rng.uniform(-0.25, 0.25, (B, D)).astype(F32), -0.5, 1.5).astype(F32), x0


def _call(N, xa, x0, path="auto", odd=False):
    """ee_pert_check_f32 on copies of the two arrays on the device; odd: both at an address 4 bytes past a 16-byte boundary."""
    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        if not odd:
            return t
        pad = torch.zeros(t.numel() + 4, dtype=t.dtype, device=DEV)
        v = pad[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    B, D = xa.shape
    a, o = dev(xa), dev(x0)
    norms = torch.full((B, 3), 7.0, device=DEV)  # garbage: every output must be written
    rng = torch.full((B, 2), 7.0, device=DEV)
    n_nan = torch.full((B,), 7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = N.lib.ee_pert_check_f32(p(a), p(o), B, D, p(norms), p(rng), p(n_nan), PATHS[path], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return norms.cpu().numpy(), rng.cpu().numpy(), n_nan.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _within_one_ulp(got, want):
    """got is want or one of its two float32 neighbours (inf and NaN: themselves)."""
    lo, hi = np.nextafter(want, F32(-np.inf)), np.nextafter(want, F32(np.inf))
    return bool(np.all((got == want) | (got == lo) | (got == hi) | (np.isnan(got) & np.isnan(want))))


def _check_against_host(ops, got, xa, x0):
    norms, rng, n_nan = got
    hn, hr, hc = ops._pert_check_host(xa, x0)
    assert norms.dtype == F32 and rng.dtype == F32 and n_nan.dtype == np.int32
    assert np.array_equal(norms[:, 0], hn[:, 0], equal_nan=True), (norms[:, 0], hn[:, 0])
    assert np.array_equal(rng, hr) and np.array_equal(n_nan, hc)
    for col, name in ((1, "L2"), (2, "L1")):
        print(name, "kernel", norms[:, col], "host", hn[:, col])
        assert _within_one_ulp(norms[:, col], hn[:, col]), (name, norms[:, col], hn[:, col])


@pytest.mark.parametrize("D", SIZES)
@pytest.mark.parametrize("B", BATCHES)
def test_against_the_host_restatement_on_every_path(env, B, D):
    N, ops = env
    xa, x0 = _points(B, D)
    outs = [_call(N, xa, x0, path) for path in ("auto",) + _paths(D)]
    _check_against_host(ops, outs[0], xa, x0)
    for other in outs[1:]:  # resident, streaming and auto: the same bits
        assert all(_same_bits(a, b) for a, b in zip(outs[0], other))
    odd = _call(N, xa, x0, "auto", odd=True)  # word-by-word loads: the same bits again
    assert all(_same_bits(a, b) for a, b in zip(outs[0], odd))


def test_rows_of_d5_start_misaligned_every_other_row(env):
    """D = 5: row b starts 20 b bytes into the tensor, so of three rows only the first is 16-byte aligned; every row is read word by word and
    its neighbours' values do not leak into it - each row equals the same row checked alone."""
    N, ops = env
    xa, x0 = _points(3, 5, seed=9)
    whole = _call(N, xa, x0)
    _check_against_host(ops, whole, xa, x0)
    for b in range(3):
        alone = _call(N, xa[b:b + 1], x0[b:b + 1])
        assert all(_same_bits(w[b:b + 1], a) for w, a in zip(whole, alone))


@pytest.mark.parametrize("D", (5, 2048, 12289))
def test_nan_inf_equal_and_all_nan_rows(env, D):
    """Row 0: one NaN in x_adv (norms NaN, the range skips it, n_nan = 1); row 1: +inf and -inf in x_adv (norms inf, range -inf .. inf);
    row 2: x_adv == x0 (norms 0); row 3: all NaN (norms NaN, range (+inf, -inf), n_nan = D); row 4: a NaN in x0 only (norms NaN, n_nan = 0)."""
    N, ops = env
    xa, x0 = _points(5, D, seed=3)
    xa[0, D // 2] = np.nan
    xa[1, 0], xa[1, D - 1] = np.inf, -np.inf
    xa[2] = x0[2]
    xa[3] = np.nan
    x0[4, D - 1] = np.nan
    for path in _paths(D):
        norms, rng, n_nan = got = _call(N, xa, x0, path)
        _check_against_host(ops, got, xa, x0)
        assert np.isnan(norms[0]).all() and n_nan[0] == 1 and rng[0, 0] == np.delete(xa[0], D // 2).min() and rng[0, 1] == np.delete(xa[0], D // 2).max()
        assert np.isposinf(norms[1]).all() and n_nan[1] == 0 and rng[1, 0] == -np.inf and rng[1, 1] == np.inf
        assert (norms[2] == 0).all() and n_nan[2] == 0
        assert np.isnan(norms[3]).all() and n_nan[3] == D and rng[3, 0] == np.inf and rng[3, 1] == -np.inf
        assert np.isnan(norms[4]).all() and n_nan[4] == 0 and rng[4, 0] == xa[4].min() and rng[4, 1] == xa[4].max()


def test_argument_checks(env):
    """The error codes of ee_apgd_start_f32, the neighbouring entry point: a negative size and an unknown path EE_ERR_SHAPE (-2), the resident
    path past its limit EE_ERR_UNSUPPORTED (-3), B == 0 EE_OK before any pointer is looked at, a null pointer EE_ERR_NULL (-1), a pointer off a
    4-byte boundary EE_ERR_ALIGN (-4).  None of these launches."""
    N, _ = env
    f = N.lib.ee_pert_check_f32
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    assert f(p, p, -1, 8, p, p, p, 0, None) == -2 and f(p, p, 2, 0, p, p, p, 0, None) == -2 and f(p, p, 2, -3, p, p, p, 0, None) == -2
    assert f(p, p, 2, 8, p, p, p, 3, None) == -2 and f(p, p, 2, 8, p, p, p, -1, None) == -2
    assert f(p, p, 2, RESIDENT + 1, p, p, p, 1, None) == -3
    assert f(None, None, 0, 8, None, None, None, 0, None) == 0
    for k in range(5):
        a = [p] * 5
        a[k] = None
        assert f(a[0], a[1], 2, 8, a[2], a[3], a[4], 0, None) == -1
        a[k] = odd
        assert f(a[0], a[1], 2, 8, a[2], a[3], a[4], 0, None) == -4


def test_ops_wrapper(env):
    """ops.pert_check: the ABI call on torch tensors of any [B, ...] shape, shapes and paths checked on the host, an empty batch accepted."""
    N, ops = env
    xa, x0 = _points(3, 192, seed=4)
    a, o = torch.from_numpy(xa).to(DEV).view(3, 3, 8, 8), torch.from_numpy(x0).to(DEV).view(3, 3, 8, 8)
    norms, rng, n_nan = ops.pert_check(a, o)
    want = _call(N, xa, x0)
    assert all(_same_bits(g.cpu().numpy(), w) for g, w in zip((norms, rng, n_nan), want))
    with pytest.raises(ValueError, match="path"):
        ops.pert_check(a, o, path="fast")
    with pytest.raises(ValueError, match="shape"):
        ops.pert_check(a, o[:2])
    with pytest.raises(N.EEError):
        ops.pert_check(a, o.cpu())
    e = torch.zeros(0, 8, device=DEV)
    assert ops.pert_check(e, e)[0].shape == (0, 3)
