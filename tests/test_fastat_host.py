"""CPU: fast adversarial training - the host fallbacks of the three ee_fastat ops against the torch restatement
(tests/fastat_reference.py) bit for bit, the config parsing and scalings of the driver, the interpolated learning rate, the center-crop
padding rule, and the driver end to end on the host plumbing with a small classifier."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import fastat_reference as FR
from tiny_models import TinyModuleNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_DIR = os.path.join(ROOT, "edge-enhancement_amd", "ImageNet", "fgsm_imagenet")


@pytest.fixture(scope="module")
def drv():
    spec = importlib.util.spec_from_file_location("main_fast", os.path.join(DRIVER_DIR, "main_fast.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def plumbing():
    from eeadv import runtime
    runtime.allow_cpu_plumbing(True)
    yield
    runtime.allow_cpu_plumbing(False)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the three ops on the host -------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_without_the_opt_in():
    from eeadv import ops
    x = torch.rand(2, 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fastat_start_(torch.zeros(6), torch.empty_like(x), x, 0.1, noise=torch.zeros_like(x))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_host_start_and_ascend_match_the_restatement(plumbing, n):
    from eeadv import ops
    g0 = torch.Generator().manual_seed(n)
    eps, alpha = 4 / 255, 5 / 255
    x = torch.rand(n, generator=g0)
    x[::7] = 0.0
    x[3::7] = 1.0
    inj = (torch.rand(n, generator=g0) * 2 - 1) * eps
    inj[::5] = eps
    inj[1::5] = -eps
    g = torch.randn(n, generator=g0)
    special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-45, -1e-45])
    g[:min(n, 7)] = special[:min(n, 7)]
    delta, in1, ctr = torch.zeros(n + 8), torch.empty(n), torch.zeros(1, dtype=torch.int64)
    ops.fastat_start_(delta, in1, x, eps, noise=inj)
    assert torch.equal(bits(delta[:n]), bits(inj)) and torch.equal(delta[n:], torch.zeros(8))
    assert torch.equal(bits(in1), bits((x + inj).clamp(0, 1.0)))  # main_fast.py:234-235
    # :246-253 through autograd: the gradient of the clamp masks g
    nb = inj.clone().requires_grad_(True)
    (x + nb).clamp(0, 1.0).backward(torch.nan_to_num(g, nan=0.0, posinf=1.0, neginf=-1.0))
    want = (inj + FR.fgsm(nb.grad, alpha)).clamp(-eps, eps)
    ops.fastat_ascend_(delta, in1, g, x, alpha, eps, ctr)
    assert torch.equal(bits(delta[:n]), bits(want)) and torch.equal(bits(in1), bits((x + want).clamp(0, 1.0)))
    assert int(ctr) == 1
    ops.fastat_ascend_(delta, in1, g, x, alpha, eps, None)  # no counter


def test_host_draw_is_the_rng_kernels_formula(plumbing):
    """fastat_draw_host restates ee_pgd_init_rng_f32 (dist 0) at offset step << 32: Philox words -> 24-bit uniforms -> u * 2 eps - eps"""
    from eeadv import ops
    from eeadv.sqatk import philox4x32
    eps, n = 4 / 255, 4099
    a, b = ops.fastat_draw_host(n, eps, 1234, 0), ops.fastat_draw_host(n, eps, 1234, 1)
    assert a.dtype == np.float32 and a.shape == (n,) and not np.array_equal(a, b)
    assert np.abs(a).max() <= np.float32(eps) and np.abs(b).max() <= np.float32(eps)
    r = philox4x32(1234, np.uint64(1 << 32) + np.arange(2, dtype=np.uint64), 0)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    e = np.float32(eps)
    assert np.array_equal(b[:8], (u * (e - (-e)) + (-e)).reshape(-1))
    delta, in1, x, ctr = torch.zeros(n), torch.empty(n), torch.rand(n), torch.ones(1, dtype=torch.int64)
    ops.fastat_start_(delta, in1, x, eps, seed=1234, step=ctr)
    assert np.array_equal(delta.numpy(), b) and int(ctr) == 1
    assert torch.equal(in1, (x + delta).clamp(0, 1))


@pytest.mark.parametrize("first", [True, False])
def test_host_keep_matches_the_restatement(plumbing, first):
    from eeadv import ops
    torch.manual_seed(3)
    B, K, per = 6, 5, 7
    x, final = torch.rand(B, per), torch.rand(B, per)
    logits = torch.randn(B, K)
    logits[1, 2] = logits[1, 4] = 9.0  # a tie: index 2
    logits[2, 1] = logits[2, 3] = float("nan")  # the first NaN: index 1
    labels = torch.tensor([int(logits[0].argmax()), 2, 1, 4, -1, K])
    want = FR.keep(final.clone(), x, logits, labels, first)
    got = ops.fastat_keep_(final.clone(), x, None if first else logits, None if first else labels, first=first)
    assert torch.equal(bits(got), bits(want))
    if not first:  # rows 0, 1, 2 are "still correct" by torch.max's tie and NaN rules and keep what they held
        assert torch.equal(got[:3], final[:3]) and torch.equal(got[4:], x[4:])
    with pytest.raises(ValueError):
        ops.fastat_keep_(x, x, first=True)


# ---- the driver's host-side pieces ----------------------------------------------------------------------------------------------------
_REF_STYLE = """
TRAIN:
    arch: 'resnet50'
    lr: 0.1
    momentum: 0.9
    weight_decay: 0.0001
    print_freq: 10
    start_epoch: 0
    epochs: 6
    lr_epochs: !!python/tuple [0,1,6]
    lr_values: !!python/tuple [0,0.4,0.04]
    half: true
    random_init: true
ADV:
    clip_eps: 4.0
    fgsm_step: 5.0
    n_repeats: 1
    pgd_attack:
    - !!python/tuple [10, 0.00392156862]
    - !!python/tuple [50, 0.00392156862]
DATA:
    workers: 16
    max_color_value: 255.0
    img_size: 0
    batch_size: 512
    crop_size: 128
"""


def test_config_parsing_both_tuple_forms_output_name_and_scaling(drv, tmp_path):
    ref = tmp_path / "ref.yml"
    ref.write_text(_REF_STYLE)
    ours = os.path.join(DRIVER_DIR, "configs", "configs_fast_4px_phase1.yml")
    a = drv.parse_config_file(drv.parse_args(["synthetic", "-c", str(ref), "--output_prefix", "p1"]))
    b = drv.parse_config_file(drv.parse_args(["synthetic", "-c", ours, "--output_prefix", "p1"]))
    assert a.TRAIN.lr_epochs == (0, 1, 6) and list(b.TRAIN.lr_epochs) == [0, 1, 6]
    assert [tuple(p) for p in a.ADV.pgd_attack] == [tuple(p) for p in b.ADV.pgd_attack] == [(10, 0.00392156862), (50, 0.00392156862)]
    for c in (a, b):
        assert c.output_name == "p1_step5_eps4_repeat1"  # before the scaling (utils.py:89-91)
        assert c.restarts == 1 and c.evaluate is False and c.data == "synthetic"
        drv.scale_config(c)
        assert c.TRAIN.epochs == 6 and c.ADV.fgsm_step == 5.0 / 255.0 and c.ADV.clip_eps == 4.0 / 255.0
        # the corner points of phase 1's schedule
        assert drv.lr_at(c, 0) == 0 and drv.lr_at(c, 1) == 0.4 and drv.lr_at(c, 6) == 0.04
        assert drv.lr_at(c, 0.5) == pytest.approx(0.2) and drv.lr_at(c, 3.5) == pytest.approx(0.22)
    c = drv.parse_config_file(drv.parse_args(["synthetic", "-c", ours]))
    c.ADV.n_repeats = 4
    assert drv.scale_config(c).TRAIN.epochs == 2  # ceil(6 / 4)


def test_the_sixteen_configs_exist_and_name_models_the_driver_builds(drv):
    names = []
    for d, tail in (("configs", ""), ("configs_ee", "_ee")):
        for eps in ("2px", "4px"):
            for phase in ("phase1", "phase2", "phase3", "evaluate"):
                names.append(os.path.join(DRIVER_DIR, d, "configs_fast_%s_%s%s.yml" % (eps, phase, tail)))
    for p in names:
        c = drv.parse_config_file(drv.parse_args(["synthetic", "-c", p]))
        assert c.TRAIN.arch == ("resnet50_EE" if p.endswith("_ee.yml") else "resnet50")
        assert c.DATA.crop_size in (128, 224, 288) and c.TRAIN.half is True and ("r" in c.DATA) == p.endswith("_ee.yml")
    assert drv.pad_str(" ARGUMENTS ") == "*" * 29 + " ARGUMENTS " + "*" * 29 and len(drv.pad_str("")) == 70


def test_unknown_arch_and_pretrained_stop(drv, tmp_path, monkeypatch, plumbing):
    monkeypatch.chdir(tmp_path)
    cfg = tmp_path / "c.yml"
    cfg.write_text(_REF_STYLE.replace("'resnet50'", "'resnet50_hfs_canny_unify'"))
    with pytest.raises(NotImplementedError):
        drv.main(["synthetic:1:1", "-c", str(cfg), "--no-cuda"])
    with pytest.raises(SystemExit, match="nothing is downloaded"):
        drv.main(["synthetic:1:1", "-c", str(cfg), "--no-cuda", "--pretrained"])


def _tv_center_crop_window(h, w, S):
    """torchvision.transforms.functional.center_crop (v0.15 - v0.20; torchvision is not installed here, so its rule is restated from
    the source): padding_ltrb = [(S - w) // 2 if S > w else 0, (S - h) // 2 if S > h else 0, (S - w + 1) // 2 if S > w else 0,
    (S - h + 1) // 2 if S > h else 0], fill 0; then crop_top = int(round((h' - S) / 2.0)), crop_left = int(round((w' - S) / 2.0))."""
    out = np.zeros((S, S), dtype=np.int64) - 1  # -1: padding; otherwise the flat index of the source pixel
    pl, pt = ((S - w) // 2 if S > w else 0), ((S - h) // 2 if S > h else 0)
    pr, pb = ((S - w + 1) // 2 if S > w else 0), ((S - h + 1) // 2 if S > h else 0)
    H2, W2 = h + pt + pb, w + pl + pr
    top, left = int(round((H2 - S) / 2.0)), int(round((W2 - S) / 2.0))
    for i in range(S):
        for j in range(S):
            si, sj = i + top - pt, j + left - pl
            if 0 <= si < h and 0 <= sj < w:
                out[i, j] = si * w + sj
    return out


@pytest.mark.parametrize("h,w,S", [(5, 8, 6), (8, 5, 6), (3, 4, 6), (9, 9, 6), (10, 7, 6), (6, 6, 6), (7, 12, 6), (1, 1, 4)])
def test_center_crop_pads_like_torchvision(h, w, S):
    from eeadv.data import center_crop_u8
    a = (np.arange(h * w * 3) % 251 + 1).astype(np.uint8).reshape(h, w, 3)
    got = center_crop_u8(a, S)
    idx = _tv_center_crop_window(h, w, S)
    want = np.where(idx[..., None] >= 0, a.reshape(-1, 3)[np.maximum(idx, 0)], 0).astype(np.uint8)
    assert got.shape == (S, S, 3) and np.array_equal(got, want)


# ---- DATA.img_size at decode -----------------------------------------------------------------------------------------------------------
def test_img_size_resizes_at_decode_and_is_part_of_the_cache_key(tmp_path):
    """main_fast.py:136-160 on a small ImageFolder tree of PNG and JPEG files (tests/fake_imagenet.py): img_size = 30 is Resize(30) in both
    splits - smaller AND larger files, PIL BILINEAR, the shorter side to 30 -, val is CenterCrop(24) of that; img_size = 0 is
    CenterCrop(24) of the file as it is, zero-padded where it is smaller; each setting has cache files of its own."""
    from PIL import Image
    import fake_imagenet as FI
    from eeadv import data as D
    root = str(tmp_path / "inet")
    items = FI.tree(root)
    S = 24

    def resized(a, short):
        img = Image.fromarray(a)
        if min(img.size) == short:
            return a
        return np.asarray(img.resize(D.resized_size(img.size[0], img.size[1], short), Image.BILINEAR))

    pixels, offsets, sizes, labels = D.load_imagenet(root, "train", (3, S, S), 3, img_size=30)
    assert sizes.min(axis=1).tolist() == [30] * len(items["train"]) and labels.tolist() == [lab for _, lab, _ in items["train"]]
    assert any(min(a.shape[:2]) < 30 for _, _, a in items["train"]) and any(min(a.shape[:2]) > 30 for _, _, a in items["train"])
    for i, (_, _, a) in enumerate(items["train"]):
        want = resized(a, 30)
        h, w = sizes[i]
        assert (h, w) == want.shape[:2] and np.array_equal(pixels[offsets[i]:offsets[i] + h * w * 3].reshape(h, w, 3), want)
    val30, vlab = D.load_imagenet(root, "val", (3, S, S), 3, img_size=30)
    val0, _ = D.load_imagenet(root, "val", (3, S, S), 3, img_size=0)
    assert val30.shape == val0.shape == (len(items["val"]), S, S, 3) and vlab.tolist() == [lab for _, lab, _ in items["val"]]
    for i, (_, _, a) in enumerate(items["val"]):
        assert np.array_equal(val30[i], D.center_crop_u8(resized(a, 30), S)) and np.array_equal(val0[i], D.center_crop_u8(a, S))
    assert not np.array_equal(val30, val0)
    small, _ = D.load_imagenet(root, "val", (3, 60, 60), 3, img_size=0)  # every val file is smaller than 60 along one side: padded
    assert small.shape[1:] == (60, 60, 3) and all((small[i] == 0).any() for i in range(len(small)))
    train0 = D.load_imagenet(root, "train", (3, S, S), 3, img_size=0)
    assert train0[2].tolist() == [list(a.shape[:2]) for _, _, a in items["train"]]  # img_size = 0: the files as they are
    names = sorted(os.listdir(D.cache_dir(root)))
    assert len([n for n in names if n.startswith("imagenet-train-")]) == 2 and len([n for n in names if n.startswith("imagenet-val-")]) == 3
    with pytest.raises(D.DataError):
        D.load_imagenet(root, "val", (3, S, S), 3, img_size=-1)


# ---- the driver end to end on the host -------------------------------------------------------------------------------------------------
_TINY = """
TRAIN: {arch: 'resnet50', lr: 0.1, momentum: 0.9, weight_decay: 0.0001, print_freq: 1, start_epoch: 0, epochs: 2,
        lr_epochs: [0, 1, 2], lr_values: [0, 0.4, 0.04], half: true, random_init: true}
ADV: {clip_eps: 4.0, fgsm_step: 5.0, n_repeats: 1, pgd_attack: [[2, 0.00392156862], [3, 0.00392156862]]}
DATA: {workers: 1, max_color_value: 255.0, img_size: 0, batch_size: 4, crop_size: 32, num_classes: 10}
"""
_TRAIN_LINE = re.compile(r"^Train Epoch: \[(\d+)\]\[(\d+)/(\d+)\]\tTime [\d.]+ \([\d.]+\)\tData [\d.]+ \([\d.]+\)\tLoss [\d.]+ \([\d.]+\)\t"
                         r"Prec@1 [\d.]+ \([\d.]+\)\tPrec@5 [\d.]+ \([\d.]+\)\tLR (\d\.\d{3})$")
_TEST_LINE = re.compile(r"^(PGD Test|Test): \[(\d+)/(\d+)\]\tTime [\d.]+ \([\d.]+\)\tLoss [\d.]+ \([\d.]+\)\tPrec@1 [\d.]+ \([\d.]+\)\t"
                        r"Prec@5 [\d.]+ \([\d.]+\)$")


def _tiny(configs):
    return TinyModuleNet(3, 32, 10, seed=5)


@pytest.fixture(scope="module")
def trained(drv, tmp_path_factory):
    """two epochs of the driver on the host plumbing, in a directory of its own"""
    from eeadv import runtime
    d = tmp_path_factory.mktemp("fastat")
    (d / "tiny.yml").write_text(_TINY)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        best = drv.main(["synthetic:3:2", "-c", "tiny.yml", "--output_prefix", "t", "--no-cuda"], build=_tiny)
    finally:
        os.chdir(cwd)
        runtime.allow_cpu_plumbing(False)
    return d, best


def test_no_cuda_run_writes_the_reference_layout(trained):
    d, best = trained
    name = "t_step5_eps4_repeat1"
    for f in ("checkpoint_epoch1.pth.tar", "checkpoint_epoch2.pth.tar", "model_best.pth.tar"):
        assert (d / "trained_models" / name / f).is_file(), f
    lines = (d / "output" / name / "log.txt").read_text().splitlines()
    assert lines[0] == "*" * 29 + " LOGISTICS " + "*" * 30 or lines[0] == "*" * 29 + " LOGISTICS " + "*" * 29
    assert any("TRAIN.half is set: this run is fp32" in ln for ln in lines)
    train = [m for m in map(_TRAIN_LINE.match, lines) if m]
    assert [(m.group(1), m.group(2), m.group(3)) for m in train] == [(str(e), str(i), "3") for e in range(2) for i in range(3)]
    # lr = interp(epoch + (i + 1) / 3): 0.133, 0.267, 0.400, 0.280, 0.160, 0.040
    assert [m.group(4) for m in train] == ["0.133", "0.267", "0.400", "0.280", "0.160", "0.040"]
    assert sum(1 for ln in lines if _TEST_LINE.match(ln)) == 4 and sum(1 for ln in lines if re.match(r"^ Final Prec@1 [\d.]+ Prec@5 [\d.]+$", ln)) == 2
    ck = torch.load(d / "trained_models" / name / "checkpoint_epoch2.pth.tar", weights_only=True)
    assert ck["epoch"] == 2 and ck["arch"] == "resnet50" and ck["best_prec1"] == best
    assert all(k.startswith("module.") for k in ck["state_dict"])  # the DataParallel-era names
    groups = ck["optimizer"]["param_groups"]
    assert len(groups) == 2 and groups[0]["weight_decay"] == 0.0001 and groups[1]["weight_decay"] == 0 and len(groups[1]["params"]) == 2
    assert isinstance(groups[0]["lr"], float) and groups[0]["lr"] == pytest.approx(0.04)
    assert ck["noise_step"] == 6  # the counter of the drawn starts: two epochs of three steps


@pytest.mark.parametrize("prefixed", [True, False])
def test_resume_reads_either_key_form_and_evaluates_with_restarts(drv, trained, prefixed):
    from eeadv import runtime
    d, _ = trained
    name = "t_step5_eps4_repeat1"
    ck = torch.load(d / "trained_models" / name / "checkpoint_epoch2.pth.tar", weights_only=True)
    if not prefixed:
        ck["state_dict"] = {k[len("module."):]: v for k, v in ck["state_dict"].items()}
    path = d / ("resume_%d.pth.tar" % prefixed)
    torch.save(ck, path)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        drv.main(["synthetic:3:2", "-c", "tiny.yml", "--output_prefix", "t", "--no-cuda", "--resume", str(path), "--evaluate", "--restarts", "2"],
                 build=_tiny)
    finally:
        os.chdir(cwd)
        runtime.allow_cpu_plumbing(False)
    lines = (d / "output" / name / "eval.txt").read_text().splitlines()
    assert any(ln == "=> loaded checkpoint '%s' (epoch 2)" % path for ln in lines)
    heads = [ln for ln in lines if " PGD eps: " in ln]
    assert len(heads) == 2 and "K: 2, step: 0.00392156862, restarts: 2 " in heads[0] and "K: 3," in heads[1]
    finals = [ln for ln in lines if re.match(r"^ (PGD )?Final Prec@1 [\d.]+ Prec@5 [\d.]+$", ln)]
    assert [ln.startswith(" PGD") for ln in finals] == [True, True, False]  # every pgd_attack pair, then the clean pass
    assert not any("TRAIN.half" in ln for ln in lines)  # main_fast.py:114: not with --evaluate


def test_pgd_restarts_on_the_host_matches_the_restatement(plumbing):
    from eeadv import trainer
    torch.manual_seed(0)
    m = TinyModuleNet(3, 8, 5, seed=2).eval()
    x, y = torch.rand(6, 3, 8, 8), torch.randint(0, 5, (6,))
    eps = 8 / 255
    noises = [(torch.rand_like(x) * 2 - 1) * eps for _ in range(3)]
    final, out = trainer.pgd_restarts(m, x, y, eps, 3, 2 / 255, 3, seed=0, noises=noises)
    want, wout = FR.validate_pgd_batch(m, x, y, eps, 3, 2 / 255, noises)
    assert torch.equal(final, want) and torch.equal(out, wout)
    assert float((final - x).abs().max()) <= eps + 1e-7 and float(final.min()) >= 0 and float(final.max()) <= 1
