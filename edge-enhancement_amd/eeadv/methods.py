"""The evaluation methods behind --attack_method as one table.

A member is one attack call on one batch, fn(model, args, x, y, ctx) -> (x_adv, robust), through a door of utils.attacks that is looked up
when the member runs.  A plan names the members of a method in the order they run - a seed=None run takes its Philox ticket from torch's
generator in call order - and says what else the dispatch has to know about the method.  trainer.attack_for_validation, the method tuples
and the option checks of trainer.py, the stage lists of cascade.py and the drivers' pre-run log lines are all read off PLANS.

A keyword reaches a door only where it says something: no norm= for Linf, no n_restarts= for one restart, no eot_iter= from a plan without
EOT, and the target count and class order of the cascade only from the cascade - each call is the call made before its option existed.
"""
import collections
import types

import utils.attacks as A


def context(args, num_steps, n_class, eot_iter=None, nkw=None, akw=None, rkw=None, n_target_classes=9):
    """What the members of one run share: APGD's iterations, the class count, E (None: the calls carry no eot_iter=), the keyword dicts of
    the norm (A._norm_kw), the APGD restarts and the FAB restarts (restarts_kw), and args.fab_iters / args.square_queries read once.  The
    cascade adds `order`, the class order of the clean logits, per batch; n_target_classes is handed on next to it only."""
    return types.SimpleNamespace(num_steps=num_steps, n_class=n_class, n_target_classes=n_target_classes, eot_iter=eot_iter, nkw=nkw or {},
                                 akw=akw or {}, rkw=rkw or {}, fab_iters=int(getattr(args, 'fab_iters', 100)),
                                 queries=int(getattr(args, 'square_queries', 5000)))


def restarts_kw(args, key, flag):
    """{} or {'n_restarts': N} from args.<key> (None / absent: 1): one restart adds nothing to a call.  `flag` is how the caller's message names
    the option."""
    n = getattr(args, key, None)
    n = 1 if n is None else int(n)
    if n < 1:
        raise ValueError("%s must be at least 1, got %d" % (flag, n))
    return {} if n == 1 else {'n_restarts': n}


def _eot(ctx):
    return {} if ctx.eot_iter is None else {'eot_iter': ctx.eot_iter}


def _targets(ctx):
    """What the cascade adds to a targeted call: its target count, positionally, and the class order it took from the clean forward."""
    return ((ctx.n_target_classes,), {'order': ctx.order}) if hasattr(ctx, 'order') else ((), {})


def _apgd_ce(model, args, x, y, ctx):
    return A.APGD(model, args, x, y, ctx.num_steps, 'ce', **_eot(ctx), **ctx.nkw, **ctx.akw)


def _apgd_dlr(model, args, x, y, ctx):
    return A.APGD(model, args, x, y, ctx.num_steps, 'dlr', **_eot(ctx), **ctx.nkw, **ctx.akw)


def _apgd_t(model, args, x, y, ctx):
    t, okw = _targets(ctx)
    return A.APGD_T(model, args, x, y, ctx.num_steps, ctx.n_class, *t, **okw, **ctx.nkw, **ctx.akw)


def _rand(model, args, x, y, ctx):  # APGD-CE then APGD-DLR inside one door, which checks the class count itself
    return A.APGD_Rand(model, args, x, y, ctx.num_steps, ctx.eot_iter, ctx.n_class, **ctx.nkw, **ctx.akw)


def _fab_t(model, args, x, y, ctx):
    t, okw = _targets(ctx)
    return A.FAB_T(model, args, x, y, ctx.n_class, ctx.fab_iters, *t, **okw, **ctx.nkw, **ctx.rkw)[:2]


def _fab_u(model, args, x, y, ctx):
    return A.FAB(model, args, x, y, ctx.fab_iters, **ctx.nkw, **ctx.rkw)[:2]  # the norm reaches it from cascade.aa_stages only (section 26)


def _square(model, args, x, y, ctx):
    return A.Square(model, args, x, y, ctx.queries, **ctx.nkw)[:2]


def _apgd_l1_ce(model, args, x, y, ctx):
    return A.APGD_L1(model, args, x, y, ctx.num_steps, 'ce', **ctx.akw)


def _apgd_t_l1(model, args, x, y, ctx):
    t, okw = _targets(ctx)
    return A.APGD_T_L1(model, args, x, y, ctx.num_steps, ctx.n_class, *t, **okw, **ctx.akw)


def _fab_t_l1(model, args, x, y, ctx):
    t, okw = _targets(ctx)
    return A.FAB_T_L1(model, args, x, y, ctx.n_class, ctx.fab_iters, *t, **okw, **ctx.rkw)[:2]


def _fab_l1_u(model, args, x, y, ctx):
    return A.FAB_L1(model, args, x, y, ctx.fab_iters, **ctx.rkw)[:2]


def _square_l1(model, args, x, y, ctx):
    return A.Square_L1(model, args, x, y, ctx.queries)[:2]


# the L1 members go through doors of their own (DESIGN.md sections 19 to 22): norm="L1" stays refused by the Linf / L2 doors
MEMBERS = {'APGD-CE': _apgd_ce, 'APGD-DLR': _apgd_dlr, 'APGD-T': _apgd_t, 'Rand': _rand, 'FAB-T': _fab_t, 'FAB-U': _fab_u, 'Square': _square,
           'APGD-L1-CE': _apgd_l1_ce, 'APGD-T-L1': _apgd_t_l1, 'FAB-T-L1': _fab_t_l1, 'FAB-L1-U': _fab_l1_u, 'Square-L1': _square_l1}
APGD_MEMBERS = ('APGD-CE', 'APGD-DLR', 'APGD-T', 'Rand', 'APGD-L1-CE', 'APGD-T-L1')  # they take --apgd_restarts (section 24)
FAB_U_MEMBERS = ('FAB-U', 'FAB-L1-U')  # untargeted: one backward pass per class and iteration (section 22)
FAB_MEMBERS = ('FAB-T', 'FAB-T-L1') + FAB_U_MEMBERS  # they take --fab_restarts (section 23)

# members: in the order they run, each on the whole batch, flags ANDed and the first fooling point kept (a cascade: each on the survivors)
# l1:      the threat model is L1, by the method's name: the ' [norm L1]' tag, --norm refused
# l2:      --norm L2 is accepted - every member is an APGD run (section 16)
# eot:     the E of the calls that carry eot_iter= when --eot_iter is absent (section 15); None: no call carries it
# eot_explicit: an --eot_iter above 1 is honoured
# cascade: runs over the whole loader (eeadv.cascade, section 14), not batch by batch
Plan = collections.namedtuple('Plan', 'members l1 l2 eot eot_explicit cascade', defaults=(False, False, None, False, False))
_STANDARD = ('APGD-CE', 'APGD-T', 'FAB-T', 'Square')  # the order of AutoAttack's `standard` version
_STANDARD_L1 = ('APGD-L1-CE', 'APGD-T-L1', 'FAB-T-L1', 'Square-L1')
PLANS = {
    'APGD-CE': Plan(('APGD-CE',), l2=True, eot=1, eot_explicit=True),
    'APGD-T': Plan(('APGD-T',), l2=True),
    'APGD': Plan(_STANDARD[:2], l2=True, eot=1),
    'Square': Plan(('Square',)),
    'APGD+Square': Plan(_STANDARD[:2] + ('Square',)),
    'FAB-T': Plan(('FAB-T',)),
    'APGD+FAB+Square': Plan(_STANDARD),
    'APGD-DLR': Plan(('APGD-DLR',), l2=True, eot=1, eot_explicit=True),
    'Rand': Plan(('Rand',), l2=True, eot=20, eot_explicit=True),  # the `rand` order for randomised defences
    'Cascade': Plan(_STANDARD, cascade=True),
    'Cascade-Rand': Plan(('APGD-CE', 'APGD-DLR'), l2=True, eot=20, eot_explicit=True, cascade=True),
    'APGD-L1-CE': Plan(('APGD-L1-CE',), l1=True),
    'APGD-L1-T': Plan(('APGD-T-L1',), l1=True),
    'APGD-L1': Plan(_STANDARD_L1[:2], l1=True),
    'FAB-L1-T': Plan(('FAB-T-L1',), l1=True),
    'APGD-L1+FAB': Plan(_STANDARD_L1[:3], l1=True),
    'Square-L1': Plan(('Square-L1',), l1=True),
    'APGD-L1+FAB+Square': Plan(_STANDARD_L1, l1=True),
    'FAB-U': Plan(('FAB-U',)),
    'FAB-L1-U': Plan(('FAB-L1-U',), l1=True),
    'Custom': Plan(('APGD-CE', 'FAB-U')),  # the reference's `custom` version (utils/aa.py: attacks_to_run = ['apgd-ce', 'fab']); Linf only
}
NO_PLAN = Plan(())  # PGD, FGSM, CW and whatever is no method at all: no member, no option


def plan_of(method):
    return PLANS.get(method, NO_PLAN)


def runs(method, members):
    """Whether `method` runs one of `members` (APGD_MEMBERS, FAB_MEMBERS, FAB_U_MEMBERS)."""
    return any(m in members for m in plan_of(method).members)


def select(keep):
    """The methods whose plan `keep` accepts, in the table's order."""
    return tuple(method for method, plan in PLANS.items() if keep(plan))
