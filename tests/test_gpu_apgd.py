"""GPU: the APGD kernels (ee_apgd.hip) and engine.apgd_loop against tests/apgd_reference.py.

Bit-exact: the momentum step, the bookkeeping and the copies (fp32 on both sides, the same operations in the same order), eager against
graph replay.  In tolerance: the row losses and their gradients against the float64 reference on the same fp32 logits."""
import os
import re
import subprocess
import sys

import pytest
import torch

import apgd_reference as R
from tiny_models import Args, TinyNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "edge-enhancement_amd")


@pytest.fixture(scope="module")
def ops():
    from eeadv import ops
    return ops


def _counter(i):
    return torch.tensor([i], dtype=torch.int32, device=DEV)


# ---- step ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B", [(P, B) for P in (1, 3, 5, 75, 1023, 3 * 8 * 8) for B in (1, 3)] + [(1, 9), (2, 7), (3, 6)])
def test_step_kernel_bit_exact(ops, B, P):
    """The last three shapes put up to four samples into one 16-byte access (B * P >= 4 with P < 4)."""
    eps = 8 / 255
    g = torch.Generator().manual_seed(100 * B + P)
    x0 = torch.rand(B, P, generator=g)
    x0[:, ::7] = 0.0  # on the lower and upper end of [0, 1]: the clamp cuts the box
    x0[:, 3::7] = 1.0
    x0[:, 5::7] = eps / 2
    d = (torch.rand(B, P, generator=g) * 2 - 1) * eps
    d[:, 1::5] = eps  # on both faces of the box: the step leaves it and is projected back
    d[:, 2::5] = -eps
    x = torch.clamp(x0 + d, 0, 1)
    x_old = torch.clamp(x0 + (torch.rand(B, P, generator=g) * 2 - 1) * eps, 0, 1)
    grad = torch.randn(B, P, generator=g)
    special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf")])
    grad.view(-1)[:: 3] = special[torch.arange(grad.view(-1)[::3].numel()) % 5]
    step = torch.tensor([2 * eps / 2 ** b for b in range(B)], dtype=torch.float32)  # per-sample steps apart by factors of 2
    for it, a in ((0, 1.0), (3, 0.75)):
        want_x, want_old = R.step(x, x_old, grad, x0, step, eps, a)
        xd, od = x.to(DEV), x_old.to(DEV)
        ops.apgd_step_(xd, od, grad.to(DEV), x0.to(DEV), step.to(DEV), _counter(it), eps)
        assert torch.equal(xd.cpu(), want_x) and torch.equal(od.cpu(), want_old), (it, B, P)
    # a view at an odd offset: the 16-byte path is not taken, the result is the same
    pad = torch.zeros(4, B * P + 1, device=DEV)
    views = [pad[i, 1:].view(B, P) for i in range(4)]
    for v, src in zip(views, (x, x_old, grad, x0)):
        v.copy_(src)
    want_x, want_old = R.step(x, x_old, grad, x0, step, eps, 0.75)
    from eeadv import _native as N
    import ctypes
    step_d, counter_d = step.to(DEV), _counter(1)
    rc = N.lib.ee_apgd_step_f32(*[ctypes.c_void_p(v.data_ptr()) for v in views], ctypes.c_void_p(step_d.data_ptr()),
                                ctypes.c_void_p(counter_d.data_ptr()), B, P, eps, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(views[0].cpu(), want_x) and torch.equal(views[1].cpu(), want_old)


def test_step_kernel_empty(ops):
    e = torch.empty(0, 12, device=DEV)
    ops.apgd_step_(e, e.clone(), e.clone(), e.clone(), torch.empty(0, device=DEV), _counter(0), 0.1)
    e = torch.empty(3, 0, device=DEV)
    ops.apgd_step_(e, e.clone(), e.clone(), e.clone(), torch.ones(3, device=DEV), _counter(0), 0.1)
    torch.cuda.synchronize()


# ---- losses --------------------------------------------------------------------------------------------------------------------------
_LOSS_REF = {}


def _loss_case(B, K):
    """Logits, labels, targets and the float64 reference of every kind, computed once per shape."""
    if (B, K) not in _LOSS_REF:
        g = torch.Generator().manual_seed(1000 * B + K)
        z = 3 * torch.randn(B, K, generator=g)
        y = torch.randint(0, K, (B,), generator=g)
        t = torch.fmod(y + torch.randint(1, K, (B,), generator=g), K)
        ref = {}
        for kind in ("ce", "dlr", "dlr_t"):
            if K < {"ce": 1, "dlr": 3, "dlr_t": 4}[kind]:
                continue
            rows = [R.row_loss_grad(z[b].double(), y[b], kind, t[b]) for b in range(B)]
            ref[kind] = (torch.stack([r[0] for r in rows]), torch.stack([r[1] for r in rows]))
        pred = torch.tensor([R.pred_row(z[b], y[b]) for b in range(B)])
        _LOSS_REF[(B, K)] = (z, y, t, ref, pred)
    return _LOSS_REF[(B, K)]


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("K", [3, 4, 10, 200, 1000])
@pytest.mark.parametrize("kind", ["ce", "dlr", "dlr_t"])
def test_loss_kernel(ops, B, K, kind):
    from eeadv import _native as N
    z, y, t, ref, pred = _loss_case(B, K)
    if kind not in ref:
        with pytest.raises(N.EEError, match="not supported"):
            ops.apgd_loss(z.to(DEV), y.to(DEV), kind, t.to(DEV))
        return
    loss, d, p = ops.apgd_loss(z.to(DEV), y.to(DEV), kind, t.to(DEV))
    want_l, want_d = ref[kind]
    loss, d = loss.cpu().double(), d.cpu().double()
    assert p.dtype == torch.int32
    if kind == "ce":
        assert torch.allclose(loss, want_l, rtol=2e-6, atol=1e-6)
        assert torch.allclose(d, want_d, rtol=1e-5, atol=1e-7)
    else:
        rel = ((loss - want_l).abs() / want_l.abs()).max()
        print("%s B=%d K=%d: max relative loss error %.3g" % (kind, B, K, float(rel)))
        assert torch.allclose(loss, want_l, rtol=1e-6, atol=0)
        assert torch.equal(d != 0, want_d != 0)
        assert torch.allclose(d, want_d, rtol=1e-5, atol=0)
    assert torch.equal(p.cpu().bool(), pred)


@pytest.mark.parametrize("kind", ["ce", "dlr", "dlr_t"])
def test_loss_kernel_tie_row(ops, kind):
    """[2, 5, 5, 5, 1]: the order is 1, 2, 3, 0, 4, so only label 1 is the prediction."""
    z = torch.tensor([[2.0, 5.0, 5.0, 5.0, 1.0]] * 4)
    y = torch.tensor([1, 2, 3, 0])
    t = torch.tensor([4, 4, 4, 4])
    loss, d, p = ops.apgd_loss(z.to(DEV), y.to(DEV), kind, t.to(DEV))
    assert p.cpu().tolist() == [1, 0, 0, 0]
    for b in range(4):
        wl, wd = R.row_loss_grad(z[b].double(), y[b], kind, t[b])
        assert torch.allclose(loss[b].cpu().double(), wl, rtol=2e-6, atol=1e-6)
        assert torch.allclose(d[b].cpu().double(), wd, rtol=1e-5, atol=1e-7) and torch.equal(d[b].cpu() != 0, wd != 0)


# ---- bookkeeping and copies, model-free ----------------------------------------------------------------------------------------------
class _DeviceState:
    """The device buffers of one run, initialised the way engine._ApgdRun.start does, and read back like a reference trace entry."""

    def __init__(self, ops, x, x_old, g, l0, pred0, eps, n_iter):
        from eeadv import engine
        B = x.shape[0]
        self.ops = ops
        self.x, self.x_old, self.g = x.to(DEV), x_old.to(DEV), g.to(DEV)
        self.x_best, self.g_best, self.x_best_adv = self.x.clone(), self.g.clone(), self.x.clone()
        self.fstate = torch.empty(4, B, device=DEV)
        self.fstate[0] = 2.0 * eps
        self.fstate[1:] = l0.to(DEV)
        self.istate = torch.zeros(4, B, dtype=torch.int32, device=DEV)
        self.istate[ops.APGD_I_REDUCED_LAST] = 1
        self.istate[ops.APGD_I_ROBUST] = pred0.to(DEV).int()
        self.counter = _counter(0)
        self.sched = torch.tensor(engine.apgd_schedule(n_iter), dtype=torch.int32, device=DEV)

    def check(self, want, where, flags=True):
        o = self.ops
        for name, got in (("x", self.x), ("x_old", self.x_old), ("g", self.g), ("x_best", self.x_best), ("g_best", self.g_best),
                          ("x_best_adv", self.x_best_adv), ("step", self.fstate[o.APGD_F_STEP]), ("loss_best", self.fstate[o.APGD_F_LOSS_BEST]),
                          ("f_prev", self.fstate[o.APGD_F_PREV]), ("loss_best_last", self.fstate[o.APGD_F_LOSS_BEST_LAST])):
            assert torch.equal(got.cpu(), want[name]), (where, name)
        assert self.istate[o.APGD_I_INC].cpu().tolist() == want["inc"].tolist(), (where, "inc")
        assert self.istate[o.APGD_I_REDUCED_LAST].cpu().bool().tolist() == want["reduced_last"].tolist(), (where, "reduced_last")
        assert self.istate[o.APGD_I_ROBUST].cpu().bool().tolist() == want["robust"].tolist(), (where, "robust")
        if flags:
            f = self.istate[o.APGD_I_FLAGS].cpu()
            assert (f & o.APGD_IMPROVED).bool().tolist() == want["improved"], (where, "improved")
            assert (f & o.APGD_FOOLED).bool().tolist() == want["fooled"], (where, "fooled")
            assert (f & o.APGD_REDUCED).bool().tolist() == want["reduced"], (where, "reduced")


@pytest.mark.parametrize("P", [75, 192])
def test_bookkeeping_on_synthetic_losses(ops, P):
    """B = 7, n_iter = 10 (windows 2, 1, 1, ...), start loss 0, distinct values throughout:
       0 rises every iteration: never reduced;         1 rises then falls: `osc` alone at the first checkpoint;
       2 1, 2, 3, .5, .7, .9, ...: both at iteration 4, neither at 5, `noimp` alone at 6;  3 fooled at iteration 0 (the first iteration);
       4 never fooled;  5, 6 shuffled values and coin-flip predictions."""
    B, n_iter, eps = 7, 10, 4 / 255
    gen = torch.Generator().manual_seed(P)
    seq = torch.empty(n_iter, B)
    seq[:, 0] = torch.arange(1, n_iter + 1) * 1.0
    seq[:, 1] = torch.tensor([1.0, 0.5, 0.25, 2.0, 3.0, 2.5, 2.75, 4.0, 3.5, 3.75]) + 0.01
    seq[:, 2] = torch.tensor([1.0, 2.0, 3.0, 0.5, 0.7, 0.9, 0.8, 0.85, 5.0, 4.0]) + 0.02
    seq[:, 3] = torch.arange(n_iter, 0, -1) * -1.0 + 0.03
    seq[:, 4] = torch.arange(1, n_iter + 1) * 0.5 + 0.04
    seq[:, 5] = torch.randperm(n_iter, generator=gen) * 1.0 - 3.05
    seq[:, 6] = torch.randperm(n_iter, generator=gen) * 0.3 - 1.06
    preds = torch.ones(n_iter, B, dtype=torch.bool)
    preds[0, 3] = False
    preds[:, 5:] = torch.rand(n_iter, 2, generator=gen) < 0.5
    l0, pred0 = torch.zeros(B), torch.ones(B, dtype=torch.bool)
    x0 = torch.rand(B, P, generator=gen)
    x = torch.clamp(x0 + (torch.rand(B, P, generator=gen) * 2 - 1) * eps, 0, 1)
    g = torch.randn(B, P, generator=gen)
    st = _DeviceState(ops, x, x, g, l0, pred0, eps, n_iter)
    book = R.Book(l0, pred0, eps)
    sched = R.schedule(n_iter)
    x_old, x_best, g_best, x_best_adv = x.clone(), x.clone(), g.clone(), x.clone()
    x0d = x0.to(DEV)
    seen, restored = set(), 0
    for i in range(n_iter):
        x, x_old = R.step(x, x_old, g, x0, torch.stack(book.step), eps, 1.0 if i == 0 else 0.75)
        g = torch.randn(B, P, generator=gen)  # stands for the classifier's gradient at the new iterate
        g_before = g.clone()
        imp, foo, red, osc, noimp = book.update(seq[i], preds[i], sched.get(i, 0))
        x_before = x.clone()
        x, g, x_best, g_best, x_best_adv = R.apply_flags(x, g, x_best, g_best, x_best_adv, imp, foo, red)
        for b in range(B):
            if sched.get(i, 0):
                seen.add(("osc" if osc[b] else "") + ("noimp" if noimp[b] else "") or "neither")
            if red[b] and not imp[b]:
                assert not torch.equal(x[b], x_before[b])  # a restore that moves the iterate
        # the device: step, then the bookkeeping from the synthetic loss, then the copies on the gradient as it was BEFORE them
        ops.apgd_step_(st.x, st.x_old, st.g, x0d, st.fstate[ops.APGD_F_STEP], st.counter, eps)
        st.g = g_before.to(DEV)
        ops.apgd_book_(seq[i].to(DEV), preds[i].to(DEV).int(), st.fstate, st.istate, st.counter, st.sched)
        ops.apgd_select_(st.x, st.g, st.x_best, st.g_best, st.x_best_adv, st.istate[ops.APGD_I_FLAGS], st.counter)
        want = dict(x=x, x_old=x_old, g=g, x_best=x_best, g_best=g_best, x_best_adv=x_best_adv, improved=imp, fooled=foo, reduced=red,
                    **book.snapshot())
        st.check(want, i)
        assert int(st.counter.item()) == i + 1
        restored += sum(1 for b in range(B) if red[b] and not imp[b])
    assert seen == {"osc", "noimp", "oscnoimp", "neither"}, seen
    assert restored >= 3 and not book.robust[3] and book.robust[4] and book.robust[0]


# ---- teacher-forced trajectory -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ce", "dlr_t"])
def test_teacher_forced_trajectory(ops, kind):
    """The reference's fp32 run on TinyNet (CPU): from its recorded x, x_old, g of iteration i the step kernel must give its next iterate,
    and from its recorded loss, pred and gradient there the bookkeeping and the copies must give its next state - bit for bit."""
    B, hw, ncls, eps, n_iter = 6, 8, 10, 0.03, 10
    torch.manual_seed(0)
    model = TinyNet(3, hw, ncls, seed=0).eval()
    x0 = torch.rand(B, 3, hw, hw)
    with torch.no_grad():
        y = model(x0).argmax(1)
    y[0] = (y[0] + 1) % ncls
    t = torch.fmod(y + 3, ncls) if kind == "dlr_t" else None
    x_init = torch.clamp(x0 + torch.zeros_like(x0).uniform_(-eps, eps), 0, 1)
    _, want_robust, _, trace = R.run(model, x0, x_init, y, n_iter, eps, kind, t)
    s = trace[0]
    st = _DeviceState(ops, s["x"], s["x_old"], s["g"], s["loss"], s["pred"], eps, n_iter)
    st.check(s, "start", flags=False)
    x0d = x0.to(DEV)
    for i in range(n_iter):
        prev, nxt = trace[i], trace[i + 1]
        st.x.copy_(prev["x"])
        st.x_old.copy_(prev["x_old"])
        st.g.copy_(prev["g"])
        ops.apgd_step_(st.x, st.x_old, st.g, x0d, st.fstate[ops.APGD_F_STEP], st.counter, eps)
        assert torch.equal(st.x.cpu(), nxt["x_new"]) and torch.equal(st.x_old.cpu(), nxt["x_old"]), i
        st.g.copy_(nxt["g_new"])
        ops.apgd_book_(nxt["loss"].to(DEV), nxt["pred"].to(DEV).int(), st.fstate, st.istate, st.counter, st.sched)
        ops.apgd_select_(st.x, st.g, st.x_best, st.g_best, st.x_best_adv, st.istate[ops.APGD_I_FLAGS], st.counter)
        st.check(nxt, i)
    assert any(any(e["reduced"]) for e in trace[1:]) and any(not all(e["reduced"]) for e in trace[1:] if e["k"])
    assert st.istate[ops.APGD_I_ROBUST].cpu().bool().tolist() == want_robust.tolist()


def _valid(xa, x0, eps):
    e = torch.tensor(eps, dtype=torch.float32)
    assert bool((xa >= x0 - e).all()) and bool((xa <= x0 + e).all()) and bool((xa >= 0).all()) and bool((xa <= 1).all())


# ---- free-running on the ResNets -----------------------------------------------------------------------------------------------------
def _resnet(ee):
    from eeadv import models
    torch.manual_seed(5)
    if ee:
        m = models.make_resnet_ee(18, "tiny", True, cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0,
                                  type_canny="CannyFilter_step125_1", epsilon=16 / 255, n_queries=1)
    else:
        m = models.make_resnet(18, "tiny")
    return m.to(DEV).eval()


def _batch(m, seed, B=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, 64, 64, generator=g).to(DEV)
    with torch.no_grad():
        y = m(x).argmax(1)
    y[0] = (y[0] + 1) % 200  # one sample starts misclassified (for the edge-enhanced model the labels are one draw's predictions)
    noise = (torch.rand(B, 3, 64, 64, generator=g) * 2 - 1) * (16 / 255)
    return x, y, noise.to(DEV)


@pytest.mark.parametrize("ee", [False, True], ids=["resnet18", "resnet18_EE_square"])
def test_free_running_eager_equals_graph(ops, ee, monkeypatch):
    """APGD-CE and APGD-T (3 targets), 64 x 64, B = 4, eval mode, 10 iterations: eager and graph replay give the same bits, a second
    replay with new inputs equals a fresh eager run, and the results are valid.  The Add_Square draws of the edge-enhanced model are
    pinned by rewinding the device draw state before every run.  `robust == (argmax model(x_adv) == y)` is checked with a second forward
    for the plain model only: with n_queries = 1 every forward of the edge-enhanced model draws a new square per sample, the point kept
    for a fooled sample was fooled under the draw of ITS iteration (which one is not recorded, and the draw state only moves forward by
    whole batches), so no single pinned forward reproduces the verdicts of all rows."""
    import utils.attacks as A
    from eeadv import engine, runtime
    m = _resnet(ee)
    eps, n_iter = 16 / 255, 10
    args = Args(epsilon=eps)
    runtime.reseed()
    torch.manual_seed(9)
    state = runtime.draw_state(torch.device(DEV))
    batches = [_batch(m, 1), _batch(m, 2)]

    def attack(which, batch, graph):
        monkeypatch.setenv("EEADV_GRAPH", "1" if graph else "0")
        x, y, noise = batch
        state.copy_(state0)
        if which == "ce":
            return A.APGD(m, args, x, y, n_iter, "ce", noise=noise)
        return A.APGD_T(m, args, x, y, n_iter, 200, n_target_classes=3, noise=noise)

    state0 = state.clone()
    for which in ("ce", "t"):
        attack(which, batches[0], True)  # builds the graphs (the warm-up passes draw too)
    state0 = state.clone()
    for which in ("ce", "t"):
        eager = [attack(which, b, False) for b in batches]
        graph = [attack(which, b, True) for b in batches]
        for (xe, re_), (xg, rg), (x, y, _) in zip(eager, graph, batches):
            assert torch.equal(xe, xg) and torch.equal(re_, rg), which
            _valid(xe.cpu(), x.cpu(), eps)
            assert not bool(re_[0])
            assert torch.equal(xe[re_], x[re_])  # robust rows are the clean inputs
            assert bool((xe[~re_] != x[~re_]).flatten(1).any(1).all())
            if not ee:
                with torch.no_grad():
                    still = m(xe).argmax(1) == y
                assert torch.equal(still[~re_], re_[~re_]), which  # every changed row is misclassified
        assert not torch.equal(eager[0][0], eager[1][0])
    engine.clear_graphs()


@pytest.mark.parametrize("ee", [False, True], ids=["resnet18", "resnet18_EE_square"])
def test_loss_best_never_falls_below_the_start(ops, ee):
    """loss_best starts at the start point's loss and only ever takes larger values - under whatever Add_Square draws the run saw."""
    from eeadv import engine
    m = _resnet(ee)
    x, y, noise = _batch(m, 3)
    eps = 16 / 255
    x_init = ops.pgd_init(x, noise)
    from eeadv import runtime
    state = runtime.draw_state(torch.device(DEV))
    state0 = state.clone()
    for kind, t in (("ce", None), ("dlr", None), ("dlr_t", torch.fmod(y + 7, 200))):
        state.copy_(state0)
        run = engine._ApgdRun(x, y, 10, eps, kind)
        run.load(x_init, x, y, t)
        run.start(m)
        l0 = run.loss0.clone()
        g = run.g
        for _ in range(10):
            g = run.iteration(m, g)
        xa, robust, best = run.result()
        assert bool((best >= l0).all()) and bool((best > l0).any()), kind
        state.copy_(state0)  # the same Add_Square draws
        xb, rb, bb = engine.apgd_loop(m, x, x_init, y, 10, eps, kind, t, use_graph=False)
        assert torch.equal(xa, xb) and torch.equal(robust, rb) and torch.equal(best, bb)
        assert int(run.counter.item()) == 10


# ---- driver --------------------------------------------------------------------------------------------------------------------------
def test_tiny_imagenet_driver_evaluates_with_apgd(tmp_path):
    cfg = open(os.path.join(PKG, "Tiny_ImageNet", "configs_tinyimagenet", "adversarial_training.yml")).read()
    cfg = re.sub(r"num_steps_(\d): \d+", r"num_steps_\1: 2", cfg).replace("batch_size: 100", "batch_size: 8").replace("print_freq: 50", "print_freq: 1")
    path = tmp_path / "apgd.yml"
    path.write_text(cfg)
    r = subprocess.run([sys.executable, "experiments_tinyimagenet.py", "-c", str(path), "--output-root", str(tmp_path), "--data", "synthetic:1:1",
                        "-e", "--attack_method", "APGD"], cwd=os.path.join(PKG, "Tiny_ImageNet"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    logs = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("log")]
    text = r.stdout + "".join(open(f).read() for f in logs)
    clean = re.findall(r"^ \* Clean Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    adv = re.findall(r"^ \* Adv Prec@1 ([\d.]+) Prec@5 ([\d.]+)$", text, flags=re.M)
    assert len(clean) >= 3 and len(clean) == len(adv)
    assert re.search(r"^Test_adv: \[0/1\]\tTime [\d.]+ \([\d.]+\)\tLoss [\d.]+ \([\d.]+\)\tPrec@1 [\d.]+ \([\d.]+\)\tPrec@5 [\d.]+ \([\d.]+\)$", text, flags=re.M)
    for (c1, _), (a1, _) in zip(clean, adv):
        assert float(a1) <= float(c1)
