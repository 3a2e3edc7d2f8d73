"""A torch restatement of the reference's fast adversarial training step (ImageNet/fgsm_imagenet/main_fast.py:224-266) and of its PGD with
restarts (lib/validation.py:29-57), with the noise injected instead of drawn, in whatever dtype the model and the inputs carry (fp32 and
float64 in the tests).  Stock torch ops only - nothing of eeadv is used - line numbers cited.

The reference's own modules cannot be imported here: main_fast.py pulls in apex and managpu at import time, runs its training at module
level and calls .cuda() throughout.  This restatement is therefore checked by READING it against those files, not by running them."""
import torch
import torch.nn.functional as F


def fgsm(gradz, step_size):
    """lib/utils.py:36-37"""
    return step_size * torch.sign(gradz)


def fast_step(model, optimizer, input, target, global_noise, fgsm_step, clip_eps, random_init, injected_noise=None):
    """One j of main_fast.py:224-266 with n_repeats = 1, in place on global_noise [N, ...]; `injected_noise` [n, ...] stands in for the
    uniform_ of :225 on the live rows (the rows beyond n are redrawn by the reference and never read before the next draw).  Returns
    (loss, output, g): the descend pass's, and the ascend pass's gradient with respect to the noise (the clamp's mask applied by autograd).
    The model is in train mode: both forwards advance BatchNorm's running statistics."""
    n = input.size(0)
    if random_init:  # :224-225
        global_noise[0:n] = injected_noise
    # :233-243 ascend on the global noise
    noise_batch = global_noise[0:n].clone().requires_grad_(True)
    in1 = input + noise_batch
    in1 = in1.clamp(0, 1.0)  # (clamp_ in the reference: the same value and the same gradient mask)
    output = model(in1)
    loss = F.cross_entropy(output, target)
    optimizer.zero_grad()  # the reference lets these weight gradients accumulate and discards them at :259; discarded here, earlier
    loss.backward()
    g = noise_batch.grad.detach().clone()
    # :246-248
    pert = fgsm(noise_batch.grad, fgsm_step)
    global_noise[0:n] += pert.data
    global_noise.clamp_(-clip_eps, clip_eps)
    # :251-266 descend
    noise_batch = global_noise[0:n].clone()
    in1 = input + noise_batch
    in1 = in1.clamp(0, 1.0)
    output = model(in1)
    loss = F.cross_entropy(output, target)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach(), output.detach(), g


def make_sgd(model, lr, momentum, weight_decay):
    """main_fast.py:99-112"""
    names = {}
    for m in model.modules():
        for p in m.parameters(recurse=False):
            names[p] = str(type(m).__name__)
    decay = [p for p in model.parameters() if 'BatchNorm' not in names[p]]
    no_decay = [p for p in model.parameters() if 'BatchNorm' in names[p]]
    return torch.optim.SGD([dict(params=decay), dict(params=no_decay, weight_decay=0)], lr, momentum=momentum, weight_decay=weight_decay)


def set_lr(optimizer, lr):
    """main_fast.py:229-230"""
    for g in optimizer.param_groups:
        g['lr'] = lr


def keep(final_input, input, output, target, first):
    """lib/validation.py:51-57"""
    if first:
        return input.clone()
    I = output.max(1)[1] != target
    final_input[I] = input[I]
    return final_input


def validate_pgd_batch(model, input, target, eps, K, step, noises):
    """lib/validation.py:29-63 on one batch, the model in eval mode; noises[r] stands in for the uniform_ of :32.  Returns
    (final_input, output)."""
    orig_input = input.clone()
    final_input = None
    for r, randn in enumerate(noises):
        input = orig_input + randn
        input = input.clamp(0, 1.0)
        for _ in range(K):
            invar = input.clone().requires_grad_(True)
            output = model(invar)
            ascend_loss = F.cross_entropy(output, target)
            ascend_grad = torch.autograd.grad(ascend_loss, invar)[0]
            pert = fgsm(ascend_grad, step)
            input = input + pert.data
            input = torch.max(orig_input - eps, input)
            input = torch.min(orig_input + eps, input)
            input = input.clamp(0, 1.0)
        with torch.no_grad():
            final_input = keep(final_input, input, None if r == 0 else model(input), target, r == 0)
    with torch.no_grad():
        output = model(final_input)
    return final_input, output
