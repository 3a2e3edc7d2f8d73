"""CPU: tests/conv_reference.py holds with the reference alone - ref64 against float64 nn.Conv2d autograd, the integer cases exact in float32, the
rounding bounds honest for a plain float32 evaluation, the Winograd restatements equal to the direct convolution, the C-ABI table against _native."""
import pytest
import torch

import conv_reference as R

INT_CASES = R.gpu_integer_cases()
RELU_CASES = R.gpu_relu_cases()


def _id(c):
    return "%s-%s%s" % (c[0], "x".join(str(v) for v in c[1]), "".join("-%s%d" % (k[0], v) for k, v in c[2]))


def _autograd64(kind, case):
    """the same results from float64 nn.Conv2d modules and autograd"""
    k, s, p = R.geometry(kind)
    B, Cin, Cout, H, W = case["shape"]
    OH, OW = R.out_hw(kind, H, W)
    gen = torch.Generator().manual_seed(1)
    t = {n: v.double() for n, v in case.items() if torch.is_tensor(v)}
    x = t.get("x", torch.randn(B, Cin, H, W, generator=gen).double()).clone().requires_grad_(True)
    conv = torch.nn.Conv2d(Cin, Cout, k, s, p, bias=False).double()
    if "w" in t:
        with torch.no_grad():
            conv.weight.copy_(t["w"])
    y = conv(x)
    outs, grads = [y], [t.get("dy", torch.zeros_like(y))]
    if "w1" in t or "dy1" in t:
        sc = torch.nn.Conv2d(Cin, Cout, 1, 2, 0, bias=False).double()
        if "w1" in t:
            with torch.no_grad():
                sc.weight.copy_(t["w1"])
        outs.append(sc(x))
        grads.append(t.get("dy1", torch.zeros_like(y)))
    if kind in R.FWD:
        return tuple(o.detach() for o in outs)
    params = [conv.weight] + ([sc.weight] if len(outs) == 2 else [])
    g = torch.autograd.grad(outs, [x] + params, grads)
    return (g[0],) if kind in R.BWD else tuple(g[1:])


@pytest.mark.parametrize("kind", R.KINDS)
def test_ref64_agrees_with_float64_conv2d_autograd(kind):
    shape = {"c1s2": (3, 6, 34, 10, 6), "stem": (2, 3, 5, 10, 6), "wrw_stem": (2, 3, 64, 6, 32), "wrw1x1": (3, 64, 64, 6, 6)}.get(
        kind if kind in R.WRW else kind.rsplit("_", 1)[0], (3, 32, 48, 8, 8))
    case = R.relu_like_case(kind, shape, 3)
    want = _autograd64(kind, case)
    got = R.ref64(kind, case)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and g.shape == w.shape
        assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())
    if kind in R.WINOGRAD:  # the transforms of the kernel headers are the same operation
        for g, w in zip(R._winograd(kind, case, torch.float64), want):
            assert float((g - w).abs().max()) <= 1e-12 * float(w.abs().max())


@pytest.mark.parametrize("c", INT_CASES, ids=_id)
def test_integer_cases_are_exact_in_float32(c):
    kind, shape, opts = c
    case = R.make_integer(kind, shape, opts)
    assert R.exactness_margin(kind, case) < 2 ** 24
    ref = R.ref64(kind, case)
    for g, r in zip(R._direct(kind, case, torch.float32), ref):
        assert g.dtype == torch.float32 and torch.equal(g.double(), r)
    if kind in R.WINOGRAD and shape[3] != 2:  # so is the transform route, every intermediate a multiple of a quarter
        for g, r in zip(R.fp32_restatement(kind, case), ref):
            assert torch.equal(g.double(), r)
    assert float(ref[0].abs().max()) < 2.0 ** 100
    nz = ref[0][ref[0] != 0].abs()
    assert nz.numel() and float(nz.min()) > 2.0 ** -100  # no denormals, no overflow
    ops = [v for n, v in case.items() if torch.is_tensor(v)]
    assert all(v.dtype == torch.float32 for v in ops)
    if not dict(opts).get("impulse") and max(shape[0] * shape[3] * shape[4], 1) >= 64:
        acts = case.get("x", case.get("dy"))
        assert 0.3 < float((acts == 0).float().mean()) < 0.7


def test_integer_cases_span_forty_binades_and_carry_negative_zeros():
    case = R.integer_case("wino_fwd", (5, 32, 96, 8, 8), 7)
    (ref,) = R.ref64("wino_fwd", case)
    per = ref.abs().amax((2, 3))
    assert float(per.max() / per[per > 0].min()) > 2.0 ** 40
    assert bool(((case["x"] == 0) & torch.signbit(case["x"])).any())


@pytest.mark.parametrize("c", RELU_CASES, ids=_id)
def test_float32_on_the_host_lies_within_the_rounding_bound(c):
    kind, shape, opts = c
    case = R.make_relu(kind, shape, opts)
    ref, bound = R.ref64(kind, case), R.rounding_bound(kind, case)
    for g, r, b in zip(R.fp32_restatement(kind, case), ref, bound):
        assert bool(((g.double() - r).abs() <= b).all()), float(((g.double() - r).abs() / b.clamp_min(1e-300)).max())
    ks = R.roundings(kind, case)
    assert len(ks) == len(ref)
    if kind == "pair_fwd":  # the shortcut's output is held to its own count: Cin products
        assert ks == (9 * shape[1] + 1, shape[1] + 1)
    # the hard inputs are what they claim: channel 1 of the activations nearly constant, result channel 2's filters summing to about 0
    acts = case.get("x", case.get("dy"))
    if acts.shape[1] > 1 and kind not in R.BWD and acts[:, 1].numel() >= 16:
        assert float(acts[:, 1].std()) < 3e-3 * float(acts[:, 1].mean().abs())
    if "w" in case and case["w"].shape[0 if kind in R.FWD else 1] > 2:
        w2 = case["w"][2] if kind in R.FWD else case["w"][:, 2]
        assert abs(float(w2.sum())) < 1e-4 * float(w2.abs().sum())


def test_winograd_filter_sets_are_exact_on_integer_filters():
    w = R.integer_case("wino_fwd", (1, 32, 64, 4, 4), 11)["w"]
    uf, ub = R.wino_filter_sets(w)
    assert torch.equal(uf.float().double(), uf) and torch.equal(ub.float().double(), ub)
    assert uf.shape == (16, 32, 64) and ub.shape == (16, 64, 32)
    g = torch.einsum("ia,jb,rkab->ijkr", R.G.float(), R.G.float(), w).reshape(16, 32, 64)  # functional._rearranged's expression
    assert torch.equal(g.double(), uf)


def test_abi_table_matches_native_signatures():
    from eeadv import _native as N
    for name, roles in R.ABI_ARGS.items():
        sig = N.SIGNATURES[name]
        assert len(roles) == len(sig), name
        for role, ct in zip(roles, sig):
            pointer = role in ("x", "u", "w", "w1", "w2", "w9", "w10", "dy", "dy1", "out", "out1", "ws", "extra", "stream")
            assert (ct is N.c_p) == pointer, (name, role)
