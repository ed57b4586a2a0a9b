"""Cases, inputs, the float64 restatement and the fixture format of the stack-tail gradient tests (tests/golden/tail_grads_*.npz,
tools/gen_golden_tail_grads.py), after hg_grad_common.py.  Everything on the input side comes from seeds; a fixture holds the seed of ll
the generator's kink search settled on, the achieved kink margin, the reference's float64 gradients of the tail's parameters, of ll
(under "input") and of previous (under "previous") in grad_common.quantities' format, and the distance of its own float32 gradients
from them.

The tail of stack s, written from the state-dict keys (P = "image_filter_lr.", 1 x 1 convolutions with bias, GroupNorm(32), eps 1e-5):
    t = conv_last{s}(ll);  a = relu(bn_end{s}(t));  out = l{s}(a);  next = previous + bl{s}(a) + al{s}(out)    (no next for the last stack)
    L = <G_out, out> + <G_next, next>
The one NORM SITE is the input of the relu, 256 h w elements per image.  A fixture is KINK-SAFE when the float64 pre-activation z64
satisfies |z64| >= 16 max |z32 - z64| over the site (sr_grad_common's rule and factor)."""
import os
from collections import OrderedDict

import numpy as np

import common
import grad_common as gc
import sr_grad_common as sg
from surs_amd import options, prng, weights

FLOOR = sg.FLOOR          # 2^-20
KINK_FACTOR = sg.KINK_FACTOR
MAX_TRIES = sg.MAX_TRIES
P = "image_filter_lr."
_TWO = ["--num_stack_lr", "2", "--hg_depth", "1"]
# name -> (stack, flags beyond common.FLAGS, (h, w) of the map, B)
CASES = OrderedDict([
    ("joint57", (0, _TWO, (5, 7), 2)),
    ("joint88", (0, _TWO, (8, 8), 2)),
    ("last57", (1, _TWO, (5, 7), 2)),
    ("d48", (0, _TWO + ["--hg_dim", "48"], (5, 7), 1)),
])
INPUT_KEY, PREVIOUS_KEY = "input", "previous"


def flags(name):
    return common.FLAGS + CASES[name][1]


def opt(name):
    return options.BaseOptions().parse(flags(name))


def stack(name):
    return CASES[name][0]


def is_last(name):
    return stack(name) == opt(name).num_stack_lr - 1


def fixture_path(golden_dir, name, part=0):
    return os.path.join(golden_dir, "tail_grads_%s%s.npz" % (name, "_p%d" % part if part else ""))


def load_fixture(golden_dir, name):
    """A case's fixture as one dict: tail_grads_<name>.npz joined with _p1, _p2, ... (every file below 1 MiB)."""
    out, part = {}, 0
    while os.path.exists(fixture_path(golden_dir, name, part)):
        out.update(np.load(fixture_path(golden_dir, name, part)))
        part += 1
    if not out:
        raise FileNotFoundError(fixture_path(golden_dir, name))
    return out


_sd_cache = {}


def state_dict(name):
    key = tuple(CASES[name][1])
    if key not in _sd_cache:
        _sd_cache[key] = weights.synthetic_state_dict(opt(name), seed=0)
    return _sd_cache[key]


def tail_names(name):
    s = stack(name)
    return ["conv_last%d" % s, "bn_end%d" % s, "l%d" % s] + ([] if is_last(name) else ["bl%d" % s, "al%d" % s])


def param_keys(name):
    """The keys a gradient exists for, in state_dict() order."""
    want = {P + m + e for m in tail_names(name) for e in (".weight", ".bias")}
    return [k for k in state_dict(name) if k in want]


def shapes(name):
    """(ll / previous / next, out) shapes."""
    _, _, (h, w), B = CASES[name]
    return (B, 256, h, w), (B, opt(name).hg_dim, h, w)


def inputs(name, seed):
    """ll: the map the kink search varies."""
    return prng.uniform("tail_grad_ll_" + name, seed, shapes(name)[0], -1.0, 1.0)


def previous(name):
    return None if is_last(name) else prng.uniform("tail_grad_prev_" + name, 3, shapes(name)[0], -1.0, 1.0)


def upstream(name):
    """(G_out, G_next or None)."""
    g_out = prng.uniform("tail_grad_Gout_" + name, 17, shapes(name)[1], -1.0, 1.0)
    return g_out, (None if is_last(name) else prng.uniform("tail_grad_Gnext_" + name, 19, shapes(name)[0], -1.0, 1.0))


# ------------------------------------------------------------------ the restatement (torch on the CPU, any dtype)
def forward(name, Pm, ll, prev, sites=None):
    """(out, next or None)."""
    import torch.nn.functional as F
    s = stack(name)
    W = lambda m: (Pm[P + m % s + ".weight"], Pm[P + m % s + ".bias"])
    t = F.conv2d(ll, *W("conv_last%d"))
    z = F.group_norm(t, 32, *W("bn_end%d"), 1e-5)
    if sites is not None:
        sites.append(z.detach().clone())
    a = F.relu(z)
    out = F.conv2d(a, *W("l%d"))
    if is_last(name):
        return out, None
    return out, prev + F.conv2d(a, *W("bl%d")) + F.conv2d(out, *W("al%d"))


def grads_of(name, ll, dtype, want_sites=False):
    """(OrderedDict key -> gradient as float64 numpy - the parameters in param_keys order, then INPUT_KEY and, for a stack that is not the
    last, PREVIOUS_KEY -, L, sites)."""
    import torch
    sd = state_dict(name)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    Pm = OrderedDict((k, T(np.array(sd[k])).requires_grad_()) for k in param_keys(name))
    llt = T(ll).requires_grad_()
    prev = None if is_last(name) else T(previous(name)).requires_grad_()
    g_out, g_next = upstream(name)
    sites = [] if want_sites else None
    with torch.enable_grad():
        out, nxt = forward(name, Pm, llt, prev, sites)
        L = (T(g_out) * out).sum()
        if nxt is not None:
            L = L + (T(g_next) * nxt).sum()
        wrt = list(Pm.values()) + [llt] + ([] if prev is None else [prev])
        got = torch.autograd.grad(L, wrt)
    names = list(Pm) + [INPUT_KEY] + ([] if prev is None else [PREVIOUS_KEY])
    return OrderedDict((k, g.detach().double().numpy()) for k, g in zip(names, got)), float(L.detach()), sites


kink_margin = sg.kink_margin


def compare(gold, grads, factor=8.0):
    """sr_grad_common.compare's rule: [(name, max |g - g64| / max |g64|, factor * max(e_ref, 2^-20))] per stored quantity."""
    return sg.compare(gold, grads, factor)


worst = sg.worst
