"""Host: the PreActResNets of the AWP sub-project (eeadv.preact, AWP/Tiny_imagenet/models_tiny_awp/preactresnet*.py) against
tests/golden/preact.npz, which the reference's own preactresnet.py wrote (tests/golden/make_preact_golden.py), and the AWP driver's
command line, directory and checkpoint names (AWP/Tiny_imagenet/experiments_tiny_awp.py) - on CPU, without a launch."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AWP = os.path.join(ROOT, "edge-enhancement_amd", "AWP", "Tiny_imagenet")
if AWP not in sys.path:
    sys.path.insert(0, AWP)

EE_KW = dict(cize=64, r=8, w=1.0, with_gf=False, low=38.0, high=76.0, alpha=0.0, sigma=1.0)


def _seeded(golden, factory=None, **kw):
    import models_tiny_awp as Z
    torch.manual_seed(int(golden("preact")["seed"]))
    return (factory or Z.PreActResNet18)(dataset="Tiny-ImageNet", **kw)


def test_state_dict_names_shapes_and_seeded_weights_match_the_reference(golden):
    G = golden("preact")
    sd = _seeded(golden).state_dict()
    assert list(sd.keys()) == list(G["names"])
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(G["shapes"])
    assert np.array_equal(np.array([v.numpy().astype(np.float64).sum() for v in sd.values()]), G["checksum"])  # numpy: a fixed summation order


def test_cpu_logits_statistics_and_input_gradient_are_the_reference_bits(golden):
    """One CPU thread, the same torch ops in the same order as preactresnet.py: bit-identical."""
    from eeadv import runtime
    G = golden("preact")
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    runtime.allow_cpu_plumbing(True)
    try:
        net = _seeded(golden).train()
        x = torch.from_numpy(G["x"]).requires_grad_(True)
        logits = net(x)
        logits.sum().backward()
        assert np.array_equal(logits.detach().numpy(), G["logits_train"])
        assert np.array_equal(x.grad.numpy(), G["grad_x"])
        sd = net.state_dict()
        stats = np.concatenate([sd[k].numpy().reshape(-1) for k in G["stat_names"]])
        assert np.array_equal(stats, G["stats"])
        assert all(int(v) == 1 for k, v in sd.items() if k.endswith("num_batches_tracked"))
        from eeadv.preact import boundary_report
        b = boundary_report(net)  # on the host every boundary is the stock add + bn_act
        assert sorted(b) == ["bn"] + ["layer%d.%d.bn1" % (i, j) for i in range(1, 5) for j in range(2) if (i, j) != (1, 0)]
        assert set(b.values()) == {"add+bn_act"}
        net.eval()
        with torch.no_grad():
            assert np.array_equal(net(torch.from_numpy(G["x"])).numpy(), G["logits_eval"])
    finally:
        runtime.allow_cpu_plumbing(False)
        torch.set_num_threads(prev)


def test_ee_variants_keys_are_the_plain_keys_plus_the_front_end(golden):
    import models_tiny_awp as Z
    from utils.core import CannyFilter, CannyFilter_BPDA, CannyFilter_step125_1
    plain = list(_seeded(golden).state_dict().keys())
    for factory, canny in ((Z.PreActResNet18_EE, CannyFilter), (Z.PreActResNet18_EE_BPDA, CannyFilter_BPDA),
                           (Z.PreActResNet18_EE_BPDA_3, CannyFilter_step125_1)):
        m = _seeded(golden, factory, **EE_KW)
        assert type(m.canny) is canny
        front = ["weight_gaussian"] + ["hfs." + k for k in m.hfs.state_dict()] + ["canny." + k for k in m.canny.state_dict()]
        keys = list(m.state_dict().keys())
        assert sorted(keys) == sorted(plain + front)
        assert [k for k in keys if k in plain] == plain  # the CNN's keys in the reference's order
    # the EE models build the front end before the CNN (preactresnet_EE.py:79-88), as the reference: the CNN weights then differ from
    # the plain model's only by the RNG the front end consumed - none here
    e = _seeded(golden, Z.PreActResNet18_EE_BPDA_3, **EE_KW).state_dict()
    p = _seeded(golden).state_dict()
    assert all(torch.equal(e[k], p[k]) for k in p)


def test_other_datasets_and_factories_keep_the_reference_names():
    import models_tiny_awp as Z
    for name in ("PreActResNet18", "PreActResNet34", "PreActResNet50", "PreActResNet101", "PreActResNet152", "PreActResNet18_EE",
                 "PreActResNet152_EE", "PreActResNet18_EE_BPDA", "PreActResNet152_EE_BPDA", "PreActResNet18_EE_BPDA_3", "AdvWeightPerturb"):
        assert callable(getattr(Z, name))
    import models_tiny_awp.preactresnet_EE as E1
    import models_tiny_awp.preactresnet_EE_BPDA as E2
    import models_tiny_awp.preactresnet_EE_BPDA_3 as E3
    for mod, cls in ((E1, "PreActResNet_EE"), (E2, "PreActResNet_EE_BPDA"), (E3, "PreActResNet_EE_BPDA_3")):
        suffix = cls[len("PreActResNet"):]
        for depth in (18, 34, 50, 101, 152):
            assert callable(getattr(mod, "PreActResNet%d%s" % (depth, suffix)))
        assert type(getattr(mod, "PreActResNet50" + suffix)(dataset="Tiny-ImageNet", **EE_KW)) is getattr(mod, cls)
    with pytest.raises(NotImplementedError):
        Z.PreActResNet18(dataset="CIFAR100")
    m = Z.PreActResNet50(dataset="Tiny-ImageNet")
    assert m.fc.in_features == 2048 and "layer1.0.shortcut.0.weight" in m.state_dict() and "layer1.1.shortcut.0.weight" not in m.state_dict()


def test_awp_driver_keeps_the_reference_command_line_and_names(tmp_path):
    """experiments_tiny_awp.py:37-54 (every flag, its default), the output directory (:147-160) and checkpoint names (:200-222)."""
    from utils.helper import parse_config_file
    drv = importlib.import_module("experiments_tiny_awp")
    a = drv.make_parser().parse_args([])
    assert (a.config, a.pretrained, a.resume, a.evaluate, a.attack_method, a.no_cuda) == ("configs.yml", False, "", False, "PGD", False)
    a = drv.make_parser().parse_args(["-c", os.path.join(AWP, "configs_tiny_awp", "ee_bpda_3_at_awp.yml"), "--output-root", str(tmp_path),
                                      "--pretrained", "-e", "--resume", "x.pth", "--attack_method", "PGD", "--no-cuda", "--data", "synthetic:1:1"])
    assert (a.pretrained, a.evaluate, a.resume, a.no_cuda, a.data) == (True, True, "x.pth", True, "synthetic:1:1")
    args = parse_config_file(a)
    assert (args.method_name, args.arch, args.awp_gamma, args.awp_warmup, args.num_steps_2, args.l1, args.l2) == (
        "EE_AT_AWP", "PreActResNet18_EE_BPDA_3", 0.005, 0, 20, 0, 0)
    d = drv.output_dirs(args)
    assert d["root"] == (str(tmp_path) + "/checkpoint_Tiny/EE_AT_AWP/PreActResNet18_EE_BPDA_3-bs100-lr0.1-momentum0.9-wd0.0005-seed0-awp_gamma0.005"
                         "epoch200/")
    assert all(os.path.isdir(d[k]) for k in ("model", "best", "log"))
    f, best = drv.driver.checkpoint_names(args, d, 3)
    assert f == d["model"] + "at_numstep10_epsilon16_r8_canny_sigma1.0_alpha0-bs100-lr_0.1-w1.0-gfFalse-l38.0-h76.0_3.pth"
    assert best == d["best"] + "at_numstep10_epsilon16r8_canny_sigma1.0_alpha0-bs100-lr_0.1-w1.0-gfFalse-l38.0-h76.0.pth"
    with pytest.raises(SystemExit, match="autoattack"):
        drv.main(["-c", os.path.join(AWP, "configs_tiny_awp", "at_awp.yml"), "--attack_method", "AA", "--output-root", str(tmp_path)])


def test_awp_driver_l2_groups_follow_the_parameter_names():
    from utils.helper import EasyDict
    drv = importlib.import_module("experiments_tiny_awp")
    import models_tiny_awp as Z
    m = Z.PreActResNet18(dataset="Tiny-ImageNet")
    opt = drv.make_optimizer(m, EasyDict(l2=0.01, lr=0.1, momentum=0.9, weight_decay=5e-4))
    decay, no_decay = opt.param_groups
    names = {id(p): n for n, p in m.named_parameters()}
    assert decay["weight_decay"] == 0.01 and no_decay["weight_decay"] == 0
    assert all("bn" not in names[id(p)] and "bias" not in names[id(p)] for p in decay["params"])
    assert {names[id(p)] for p in no_decay["params"]} == {n for n in names.values() if "bn" in n or "bias" in n}
