"""GPU: the pre-activation block boundary (ee_bn_sum_act_fwd/bwd_f32, functional.BnSumActFn), the PreActResNets of the AWP sub-project on
the HIP path (eeadv.preact), the AWP step with them and the AWP driver (AWP/Tiny_imagenet/experiments_tiny_awp.py)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")
AWP = os.path.join(PKG, "AWP", "Tiny_imagenet")
if AWP not in sys.path:
    sys.path.insert(0, AWP)
DEV = "cuda:0"
EE_KW = dict(cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0)


def _case(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, C = shape[:2]
    x = torch.randn(shape, generator=g) * 2 + 0.5
    r = torch.randn(shape, generator=g)
    w = torch.rand(C, generator=g) + 0.5
    b = torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    dy, dy2, dsa = (torch.randn(shape, generator=g) for _ in range(3))
    return x, r, w, b, rm, rv, dy, dy2, dsa


def _kernel_run(shape, seed, training, dy2_on, dsa_on, want_sum, want_params):
    from eeadv import ops
    x, r, w, b, rm, rv, dy, dy2, dsa = (t.to(DEV) for t in _case(shape, seed))
    rm_o, rv_o = rm.clone(), rv.clone()
    y, s, sm, si = ops.bn_sum_act_fwd(x, r, w, b, rm, rv, 0.1, 1e-5, training, True, want_sum=True)
    # the same forward with sum_out given or NULL (want_sum): everything else must be the same bits
    y_o, s_opt, sm_o, si_o = ops.bn_sum_act_fwd(x, r, w, b, rm_o, rv_o, 0.1, 1e-5, training, True, want_sum=want_sum)
    ds, dg, db = ops.bn_sum_act_bwd(dy, dy2 if dy2_on else None, None, s, w, b, sm, si, None if training else rm, None if training else rv,
                                    1e-5, training, True, dsa if dsa_on else None, want_params)
    ds_y, _, _ = ops.bn_sum_act_bwd(dy, dy2 if dy2_on else None, y, s, w, b, sm, si, None if training else rm, None if training else rv,
                                    1e-5, training, True, dsa if dsa_on else None, False)
    return dict(y=y, s=s, s_opt=s_opt, sm=sm, si=si, rm=rm, rv=rv, ds=ds, ds_y=ds_y, dg=dg, db=db, y_o=y_o, sm_o=sm_o, si_o=si_o, rm_o=rm_o,
                rv_o=rv_o)


SHAPES = [(100, 64, 16, 16), (100, 128, 8, 8), (100, 256, 4, 4), (100, 512, 2, 2), (37, 64, 16, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("dy2_on,dsa_on,want_sum,want_params", [(False, False, False, False), (True, True, True, True), (False, True, True, False),
                                                                (True, False, False, True)])
def test_bn_sum_act_matches_a_float64_composition(shape, training, dy2_on, dsa_on, want_sum, want_params):
    x, r, w, b, rm0, rv0, dy, dy2, dsa = _case(shape, sum(shape))
    got = _kernel_run(shape, sum(shape), training, dy2_on, dsa_on, want_sum, want_params)
    # float64 reference: s = x + r, relu(bn(s)); ds = d/ds with the same incoming pieces
    xd, rd = x.double().requires_grad_(True), r.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    rm, rv = rm0.double(), rv0.double()
    s = xd + rd
    y = F.relu(F.batch_norm(s, rm, rv, wd, bd, training, 0.1, 1e-5))
    g_in = dy.double() + (dy2.double() if dy2_on else 0)
    gx, gr, gw, gb = torch.autograd.grad(y, [xd, rd, wd, bd], g_in)
    ds_ref = gx + (dsa.double() if dsa_on else 0)
    assert torch.equal(gx, gr)
    n = shape[0] * shape[2] * shape[3]
    torch.testing.assert_close(got["y"].cpu().double(), y.detach(), rtol=1e-5, atol=2e-5)
    assert torch.equal(got["s"].cpu(), x + r)  # one fp32 add per element
    assert (got["s_opt"] is not None) == want_sum and (got["s_opt"] is None or torch.equal(got["s_opt"], got["s"]))
    for k in ("y", "rm", "rv") + (("sm", "si") if training else ()):
        assert torch.equal(got[k + "_o"], got[k]), k
    torch.testing.assert_close(got["rm"].cpu().double(), rm, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got["rv"].cpu().double(), rv, rtol=1e-5, atol=1e-6)
    if training:
        s32 = (x + r).double()
        mean = s32.mean(dim=(0, 2, 3))
        var = s32.var(dim=(0, 2, 3), unbiased=False)
        torch.testing.assert_close(got["sm"].cpu().double(), mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(got["si"].cpu().double(), 1 / torch.sqrt(var + 1e-5), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got["ds"].cpu().double(), ds_ref, rtol=2e-5, atol=4e-5)
    assert torch.equal(got["ds"], got["ds_y"])  # the mask from y or recomputed from s: the same bits
    if want_params:
        tol = 2e-5 * max(1.0, n ** 0.5)
        torch.testing.assert_close(got["dg"].cpu().double(), gw, rtol=2e-5, atol=tol)
        torch.testing.assert_close(got["db"].cpu().double(), gb, rtol=2e-5, atol=tol)
    else:
        assert got["dg"] is None and got["db"] is None


_BITS_CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [%r, %r]
import test_gpu_preact as T
out = {}
for i, shape in enumerate(T.SHAPES):
    for tr in (True, False):
        got = T._kernel_run(shape, 3 + i, tr, True, True, True, True)
        for k, v in got.items():
            if v is not None:
                out["%%d_%%d_%%s" %% (i, tr, k)] = v.cpu().numpy()
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_bn_sum_act_bits_are_reproducible_and_the_same_with_one_part_per_channel(tmp_path):
    """EEADV_BN_PARTS=0 (one workgroup per channel) against the default split: every part forms the whole sums, the same bits"""
    runs = []
    for tag, env in (("a", {}), ("b", {}), ("one", {"EEADV_BN_PARTS": "0"})):
        path = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", _BITS_CHILD % (os.path.dirname(__file__), PKG), path], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        runs.append(np.load(path))
    for other in runs[1:]:
        assert set(other.files) == set(runs[0].files)
        for k in runs[0].files:
            assert np.array_equal(runs[0][k], other[k], equal_nan=True), k


@pytest.mark.gpu
def test_bn_sum_act_refuses_shapes_beyond_the_register_cache():
    from eeadv import _native as N, ops
    x = torch.zeros(100, 64, 32, 32, device=DEV)  # B*HW = 102400 > 28672
    assert not ops.bn_sum_act_supported(x)
    p = ctypes.c_void_p(x.data_ptr())
    w = torch.ones(64, device=DEV)
    pw = ctypes.c_void_p(w.data_ptr())
    assert N.lib.ee_bn_sum_act_fwd_f32(p, p, pw, pw, pw, pw, 0.1, 1e-5, 1, 1, None, p, pw, pw, 100, 64, 1024, None) == -3
    assert N.lib.ee_bn_sum_act_bwd_f32(p, None, None, p, pw, pw, pw, pw, None, None, 1e-5, 1, 1, None, p, None, None, 100, 64, 1024, None) == -3
    assert N.lib.ee_bn_sum_act_fwd_f32(p, p, pw, pw, pw, pw, 0.1, 1e-5, 1, 1, None, p, pw, pw, 100, 64, 30, None) == -3  # H*W % 4
    torch.cuda.synchronize()


# ---- the models ------------------------------------------------------------------------------------------------------------------
_MODEL_CHILD = r"""
import os, sys, numpy as np, torch
sys.path[:0] = [%r, %r, %r]
import models_tiny_awp as Z, utils.attacks as A
from eeadv import engine, models as M, preact as P
assert engine.graphs_enabled() == (os.environ.get("EEADV_GRAPH") == "1")
from tiny_models import Args
torch.manual_seed(5)
out = {}
g = torch.Generator().manual_seed(9)
x = torch.rand(100, 3, 64, 64, generator=g).cuda()
y = torch.randint(0, 200, (100,), generator=g).cuda()
wl = torch.randn(100, 200, generator=g).cuda()
for name, kw in (("plain", {}), ("ee3", %r)):
    f = Z.PreActResNet18 if name == "plain" else Z.PreActResNet18_EE_BPDA_3
    torch.manual_seed(1)
    net = f(dataset="Tiny-ImageNet", **kw).cuda()
    for mode in ("train", "eval"):
        net.train(mode == "train")
        xi = x.clone().requires_grad_(True)
        logits = net(xi)
        net.zero_grad()
        (logits * wl).sum().backward()
        out["%%s_%%s_logits" %% (name, mode)] = logits.detach().cpu().numpy()
        out["%%s_%%s_gx" %% (name, mode)] = xi.grad.cpu().numpy()
        for k, p in net.named_parameters():
            if p.grad is not None:
                out["%%s_%%s_g_%%s" %% (name, mode, k)] = p.grad.cpu().numpy()
        out["%%s_%%s_routes" %% (name, mode)] = np.array(M.fallback_report(net)["layers"] + ["-"])
        out["%%s_%%s_boundaries" %% (name, mode)] = np.array(sorted("%%s:%%s" %% kv for kv in P.boundary_report(net).items()))
        if name == "ee3":
            # the CNN body from the front end's (fp32) output: the float64 host copy runs the same body from the same x_in
            with torch.no_grad():
                x_in = net.front(x)
            for k, v in net.state_dict().items():
                if "running_" in k:
                    out["ee3_%%s_rs_%%s" %% (mode, k)] = v.cpu().numpy()
            xb = x_in.clone().requires_grad_(True)
            lb = net.body(xb)
            net.zero_grad()
            (lb * wl).sum().backward()
            out["ee3_%%s_xin" %% mode] = x_in.cpu().numpy()
            out["ee3_%%s_body_logits" %% mode] = lb.detach().cpu().numpy()
            out["ee3_%%s_body_gx" %% mode] = xb.grad.cpu().numpy()
            for k, p in net.named_parameters():
                if p.grad is not None:
                    out["ee3_%%s_body_g_%%s" %% (mode, k)] = p.grad.cpu().numpy()
    # the attack loop in train mode: graph replay in the fused child (EEADV_GRAPH=1), eager in the stock one
    net.train()
    args = Args(random=False, epsilon=16 / 255)
    xa = A.PGD(net, args, x, y, 3, 2 / 255)
    out[name + "_pgd"] = xa.cpu().numpy()
    sd = net.state_dict()
    for k in sd:
        if "running_" in k:
            out[name + "_stat_" + k] = sd[k].cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def _child(tmp_path, tag, env, code):
    path = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(path)


@pytest.fixture(scope="module")
def model_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("preact")
    code = _MODEL_CHILD % (os.path.dirname(__file__), PKG, AWP, EE_KW)
    return (_child(tmp, "fused", {"EEADV_GRAPH": "1"}, code), _child(tmp, "stock", {"EEADV_STOCK_GLUE": "preact", "EEADV_GRAPH": "0"}, code))


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, np.abs(b).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "ee3"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_fused_boundary_matches_the_stock_add_and_bn_act(model_runs, name, mode):
    """Logits, input and parameter gradients of the fused route against EEADV_STOCK_GLUE=preact (add + bn_act): the same expressions,
    the BatchNorm sums over the sum in one launch instead of two; differences are rounding, propagated through 18 layers."""
    fused, stock = model_runs
    pre = "%s_%s_" % (name, mode)
    assert _rel(fused[pre + "logits"], stock[pre + "logits"]) < 1e-4
    assert _rel(fused[pre + "gx"], stock[pre + "gx"]) < 1e-3
    keys = [k for k in stock.files if k.startswith(pre + "g_")]
    assert len(keys) == len([k for k in fused.files if k.startswith(pre + "g_")]) > 40
    for k in keys:
        assert _rel(fused[k], stock[k]) < 2e-3, k
    # every boundary took the fused launch in the one run and the stock add + bn_act in the other
    for run, how in ((fused, "ee_bn.sum_act"), (stock, "add+bn_act")):
        b = list(run[pre + "boundaries"])
        assert len(b) == 8 and all(t.endswith(":" + how) for t in b), b
    routes = list(fused[pre + "routes"])
    assert not [r for r in routes if r.startswith(("layer1", "layer2", "layer3"))], routes


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "ee3"])
def test_attack_loop_route_matches_eager_stock(model_runs, name):
    """PGD-3 in train mode: graph replay with the fused boundaries against eager EEADV_STOCK_GLUE=preact.  A sign step can flip where
    a gradient entry is within rounding of zero: nearly all pixels agree, none is more than two steps apart."""
    fused, stock = model_runs
    a, b = fused[name + "_pgd"], stock[name + "_pgd"]
    d = np.abs(a - b)
    assert (d > 1e-6).mean() < 2e-3 and d.max() <= 4 / 255 + 1e-6
    for k in [k for k in stock.files if k.startswith(name + "_stat_")]:
        np.testing.assert_allclose(fused[k], stock[k], rtol=1e-3, atol=1e-4, err_msg=k)


def _rel2(a, b):
    return float(np.linalg.norm((a.astype(np.float64) - b).ravel()) / max(1e-30, np.linalg.norm(b.ravel())))


@pytest.mark.gpu
def test_fused_route_matches_a_float64_cpu_copy(model_runs):
    import models_tiny_awp as Z
    from eeadv import runtime
    fused, _ = model_runs
    g = torch.Generator().manual_seed(9)
    x = torch.rand(100, 3, 64, 64, generator=g)
    torch.randint(0, 200, (100,), generator=g)
    wl = torch.randn(100, 200, generator=g).double()
    torch.manual_seed(1)
    net = Z.PreActResNet18(dataset="Tiny-ImageNet").double()
    runtime.allow_cpu_plumbing(True)
    try:
        for mode in ("train", "eval"):
            net.train(mode == "train")
            xi = x.double().requires_grad_(True)
            logits = net(xi)
            net.zero_grad()
            (logits * wl).sum().backward()
            pre = "plain_%s_" % mode
            assert _rel(fused[pre + "logits"], logits.detach().numpy()) < 1e-4
            # gradients: the max-pool's argmax and the ReLU masks are decided in fp32 on the device, in fp64 here - a near-tie decided the
            # other way moves a whole gradient entry (max-norm errors of a few %, seen on the input gradient), so the bound is on the
            # relative 2-norm
            e = _rel2(fused[pre + "gx"], xi.grad.numpy())
            assert e < 1e-2, e
            for k, p in net.named_parameters():
                e = _rel2(fused[pre + "g_" + k], p.grad.numpy())
                assert e < 1e-2, (k, e)
    finally:
        runtime.allow_cpu_plumbing(False)


@pytest.mark.gpu
def test_ee_bpda_3_body_matches_a_float64_cpu_copy(model_runs):
    """PreActResNet18_EE_BPDA_3: its CNN body from the device front end's output x_in (the front end's host plumbing is fp32-only; its
    kernels are pinned to the oracle elsewhere) against a float64 CPU copy with the same weights and, in eval mode, the same running
    statistics.  The full model's logits are that body's logits; the bounds are those of the plain model's test."""
    import models_tiny_awp as Z
    from eeadv import runtime
    fused, _ = model_runs
    g = torch.Generator().manual_seed(9)
    torch.rand(100, 3, 64, 64, generator=g)
    torch.randint(0, 200, (100,), generator=g)
    wl = torch.randn(100, 200, generator=g).double()
    torch.manual_seed(1)
    net = Z.PreActResNet18_EE_BPDA_3(dataset="Tiny-ImageNet", **EE_KW).double()
    runtime.allow_cpu_plumbing(True)
    try:
        for mode in ("train", "eval"):
            pre = "ee3_%s_" % mode
            with torch.no_grad():
                for k, v in net.state_dict().items():
                    if pre + "rs_" + k in fused.files:
                        v.copy_(torch.from_numpy(fused[pre + "rs_" + k]).double())
            net.train(mode == "train")
            xi = torch.from_numpy(fused[pre + "xin"]).double().requires_grad_(True)
            logits = net.body(xi)
            net.zero_grad()
            (logits * wl).sum().backward()
            assert _rel(fused[pre + "body_logits"], logits.detach().numpy()) < 1e-4
            assert _rel(fused[pre + "logits"], logits.detach().numpy()) < 1e-4  # the whole model: front end + this body
            e = _rel2(fused[pre + "body_gx"], xi.grad.numpy())
            assert e < 1e-2, e
            n = 0
            for k, p in net.named_parameters():
                if p.grad is not None:
                    e = _rel2(fused[pre + "body_g_" + k], p.grad.numpy())
                    assert e < 1e-2, (k, e)
                    n += 1
            assert n > 40
    finally:
        runtime.allow_cpu_plumbing(False)


@pytest.mark.gpu
def test_seeded_model_on_the_device_matches_the_reference_fixture(golden):
    import models_tiny_awp as Z
    G = golden("preact")
    torch.manual_seed(int(G["seed"]))
    net = Z.PreActResNet18(dataset="Tiny-ImageNet").to(DEV).train()
    x = torch.from_numpy(G["x"]).to(DEV)
    np.testing.assert_allclose(net(x).detach().cpu().numpy(), G["logits_train"], rtol=0, atol=1e-4)
    net.eval()
    with torch.no_grad():
        np.testing.assert_allclose(net(x).cpu().numpy(), G["logits_eval"], rtol=0, atol=1e-4)


# ---- AWP -------------------------------------------------------------------------------------------------------------------------
_AWP_CHILD = r"""
import os, sys, numpy as np, torch
sys.path[:0] = [%r, %r, %r]
import models_tiny_awp as Z
from eeadv import engine, trainer
assert engine.graphs_enabled() == (os.environ.get("EEADV_GRAPH") == "1")
from tiny_models import Args
kw = %r
torch.manual_seed(3)
net, proxy, fresh = (Z.PreActResNet18_EE_BPDA_3(dataset="Tiny-ImageNet", **kw).cuda() for _ in range(3))
opt = trainer.make_sgd(net.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-4)
adv = Z.AdvWeightPerturb(model=net, proxy=proxy, proxy_optim=trainer.make_sgd(proxy.parameters(), lr=0.01), gamma=0.005)
args = Args(method_name="EE_AT_AWP", random=True, epsilon=16 / 255, num_steps_1=10, step_size_1=2 / 255, awp_warmup=0)
g = torch.Generator().manual_seed(4)
x = torch.rand(100, 3, 64, 64, generator=g).cuda()
y = torch.randint(0, 200, (100,), generator=g).cuda()
out, checks = {}, []
perturb, restore = adv.perturb, adv.restore
def against_fresh_copy():
    # eval mode, the body only: running statistics, no draws - equal weights must give equal logits
    fresh.load_state_dict(net.state_dict())
    was = net.training
    net.eval(), fresh.eval()
    with torch.no_grad():
        a, b = net.body(x[:50]), fresh.body(x[:50])
    net.train(was)
    return float((a - b).abs().max())
def checked_perturb(diff):
    perturb(diff)
    checks.append(against_fresh_copy())
def checked_restore(diff):
    stepped = {k: p.detach().clone() for k, p in net.named_parameters()}
    restore(diff)
    checks.append(max(float((p.detach() - (stepped[k] - 0.005 * diff[k] if k in diff else stepped[k])).abs().max())
                      for k, p in net.named_parameters()))
    checks.append(against_fresh_copy())
adv.perturb, adv.restore = checked_perturb, checked_restore
for step in range(3):
    torch.manual_seed(100 + step)
    loss, logits = trainer.awp_train_batch(net, adv, trainer.Criterion(), opt, args, x, y, 0, x.device)
    out["loss_%%d" %% step] = loss.cpu().numpy()
out["w"] = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu().numpy()
out["checks"] = np.array(checks)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_three_awp_steps_match_the_eager_stock_route(tmp_path):
    """Three AWP steps (PGD-10, proxy step, perturb, robust step, restore) with PreActResNet18_EE_BPDA_3: fused + graphs against
    EEADV_GRAPH=0 EEADV_STOCK_GLUE=preact.  Right after perturb and after restore the model's body equals a freshly loaded copy of its
    weights (no stale re-arranged filter buffers); restore leaves the optimiser's result minus gamma * diff."""
    code = _AWP_CHILD % (os.path.dirname(__file__), PKG, AWP, EE_KW)
    fused = _child(tmp_path, "fused", {"EEADV_GRAPH": "1"}, code)
    stock = _child(tmp_path, "stock", {"EEADV_GRAPH": "0", "EEADV_STOCK_GLUE": "preact"}, code)
    for run in (fused, stock):
        assert len(run["checks"]) == 9 and float(run["checks"].max()) < 1e-5, run["checks"]
    for s in range(3):
        np.testing.assert_allclose(fused["loss_%d" % s], stock["loss_%d" % s], rtol=2e-3)
    assert _rel(fused["w"], stock["w"]) < 2e-3


# ---- the driver ------------------------------------------------------------------------------------------------------------------
_LOG = re.compile(r"Epoch: \[0\]\[0/2\]\tTime [\d.]+ \([\d.]+\)\tData [\d.]+ \([\d.]+\)\tRobust Loss ([\d.]+) \(([\d.]+)\)\t"
                  r"Prec@1 [\d.]+ \([\d.]+\)\tPrec@5 [\d.]+ \([\d.]+\)\t")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["at_awp", "ee_at_awp", "ee_bpda_at_awp", "ee_bpda_3_at_awp"])
def test_awp_driver_runs_every_config(tmp_path, cfg):
    script = os.path.join(AWP, "experiments_tiny_awp.py")
    base = [sys.executable, script, "-c", os.path.join(AWP, "configs_tiny_awp", cfg + ".yml"), "--data", "synthetic:2:1",
            "--output-root", str(tmp_path)]
    r = subprocess.run(base + ["--max-epochs", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    m = _LOG.search(r.stdout)
    assert m, r.stdout[-3000:]
    assert 0.5 < float(m.group(1)) < 40
    assert re.search(r"Test_adv: \[0/1\]\tTime [\d.]+ \([\d.]+\)\tLoss [\d.]+ \([\d.]+\)\tPrec@1 [\d.]+ \([\d.]+\)", r.stdout)
    assert re.search(r" \* Adv Prec@1 [\d.]+ Prec@5 [\d.]+", r.stdout)
    root = [l for l in r.stdout.splitlines() if l.startswith("Output dir:")][0][len("Output dir:"):]
    assert os.path.isfile(root + "log/log.txt") and os.path.isfile(root + "log/log_pgd.txt")
    ckpts = os.listdir(root + "model_pth")
    assert len(ckpts) == 1 and ckpts[0].endswith("_0.pth")
    ck = torch.load(root + "model_pth/" + ckpts[0], map_location="cpu", weights_only=True)
    assert ck["epoch"] == 1 and set(ck) == {"epoch", "arch", "state_dict", "best_prec1", "optimizer"}
    if cfg == "ee_bpda_3_at_awp":
        r2 = subprocess.run(base + ["--resume", root + "model_pth/" + ckpts[0], "-e"], capture_output=True, text=True, timeout=600)
        assert r2.returncode == 0, r2.stderr[-3000:]
        assert "=> loaded checkpoint" in r2.stdout and "(epoch 1)" in r2.stdout
        assert "=> PGD: num_step:10," in r2.stdout and "AutoAttack skipped" in r2.stdout
        assert len(re.findall(r" \* Adv Prec@1", r2.stdout)) == 2
