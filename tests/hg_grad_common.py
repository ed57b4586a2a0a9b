"""Inputs, the float64 restatement and the fixture format of the hourglass gradient tests (tests/golden/hg_grads_*.npz,
tools/gen_golden_hg_grads.py), after sr_grad_common.py.  Everything on the input side comes from seeds; a fixture holds the input seed
the generator's kink search settled on, the achieved kink margin, the reference's float64 gradients of the module's parameters AND of its
input (grad_common.quantities' format) and the distance of its own float32 gradients from them.

The loss of a case, for an input x [B,256,h,w] and a seeded upstream G of the module's output shape:  L = <G, module(x)>.
The modules, written here from the state-dict keys (P = "image_filter_lr."):
    ConvBlock p:   o1 = conv1(relu(bn1(x))), o2 = conv2(relu(bn2(o1))), o3 = conv3(relu(bn3(o2))), out = cat(o1, o2, o3) + x
                   (3 x 3, padding 1, no bias; bn = GroupNorm(32), eps 1e-5)
    HourGlass m{s}, level l:  up1 = b1_l(x); low = b2_l(avg_pool2(x)); low = level l - 1 (l > 1) or b2_plus_1(low); low = b3_l(low);
                   out = up1 + bicubic x2 (align_corners) of low
    stack1:        t = top_m_0(m0(conv2(x)));  out = l0(relu(bn_end0(conv_last0(t))))      (1 x 1 convolutions with bias)
A NORM SITE is the input of any relu above.  A fixture is KINK-SAFE when at every site the float64 pre-activation z64 satisfies
|z64| >= 16 max over that site of |z32 - z64| (sr_grad_common's rule and factor)."""
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
# name -> (module, flags beyond common.FLAGS, (h, w) of the map, B)
CASES = OrderedDict([
    ("cb_tiny", ("conv2", [], (4, 6), 2)),
    ("hg_d1", ("m0", ["--hg_depth", "1"], (4, 6), 2)),
    ("hg_d2", ("m0", ["--hg_depth", "2"], (8, 12), 1)),
    ("stack1", ("stack", ["--num_stack_lr", "1", "--hg_depth", "1"], (8, 8), 1)),
])
INPUT_KEY = "input"       # the name the input gradient's quantities are stored under


def flags(name):
    return common.FLAGS + CASES[name][1]


def opt(name):
    return options.BaseOptions().parse(flags(name))


def fixture_path(golden_dir, name, part=0):
    return os.path.join(golden_dir, "hg_grads_%s%s.npz" % (name, "_p%d" % part if part else ""))


def load_fixture(golden_dir, name):
    """A case's fixture as one dict: hg_grads_<name>.npz joined with _p1, _p2, ... (every file below 1 MiB)."""
    out, part = {}, 0
    while os.path.exists(fixture_path(golden_dir, name, part)):
        out.update(np.load(fixture_path(golden_dir, name, part)))
        part += 1
    if not out:
        raise FileNotFoundError(fixture_path(golden_dir, name))
    return out


_sd_cache = {}


def state_dict(name):
    if name not in _sd_cache:
        _sd_cache[name] = weights.synthetic_state_dict(opt(name), seed=0)
    return _sd_cache[name]


def block_keys(prefix):
    return [prefix + k for k in ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
                                 "bn3.weight", "bn3.bias")]


def hourglass_blocks(stack, depth):
    """The ConvBlock prefixes of m{stack} in module order."""
    out = []

    def gen(level):
        out.append(P + "m%d.b1_%d." % (stack, level))
        out.append(P + "m%d.b2_%d." % (stack, level))
        if level > 1:
            gen(level - 1)
        else:
            out.append(P + "m%d.b2_plus_%d." % (stack, level))
        out.append(P + "m%d.b3_%d." % (stack, level))
    gen(depth)
    return out


def param_keys(name):
    """The keys a gradient exists for, in state_dict() order."""
    module, o = CASES[name][0], opt(name)
    if module == "conv2":
        want = set(block_keys(P + "conv2."))
    elif module == "m0":
        want = {k for p in hourglass_blocks(0, o.hg_depth) for k in block_keys(p)}
    else:
        want = {k for p in [P + "conv2."] + hourglass_blocks(0, o.hg_depth) + [P + "top_m_0."] for k in block_keys(p)}
        want |= {P + m + e for m in ("conv_last0", "bn_end0", "l0") for e in (".weight", ".bias")}
    return [k for k in state_dict(name) if k in want]


def shapes(name):
    """(input, output) shapes."""
    _, _, (h, w), B = CASES[name]
    c_out = opt(name).hg_dim if CASES[name][0] == "stack" else 256
    return (B, 256, h, w), (B, c_out, h, w)


def inputs(name, seed):
    return prng.uniform("hg_grad_x_" + name, seed, shapes(name)[0], -1.0, 1.0)


def upstream(name):
    return prng.uniform("hg_grad_G_" + name, 17, shapes(name)[1], -1.0, 1.0)


# ------------------------------------------------------------------ the restatement (torch on the CPU, any dtype)
def _norm_relu(Pm, key, t, sites):
    import torch.nn.functional as F
    z = F.group_norm(t, 32, Pm[key + ".weight"], Pm[key + ".bias"], 1e-5)
    if sites is not None:
        sites.append(z.detach().clone())
    return F.relu(z)


def conv_block(Pm, p, x, sites=None):
    import torch
    import torch.nn.functional as F
    o1 = F.conv2d(_norm_relu(Pm, p + "bn1", x, sites), Pm[p + "conv1.weight"], padding=1)
    o2 = F.conv2d(_norm_relu(Pm, p + "bn2", o1, sites), Pm[p + "conv2.weight"], padding=1)
    o3 = F.conv2d(_norm_relu(Pm, p + "bn3", o2, sites), Pm[p + "conv3.weight"], padding=1)
    return torch.cat((o1, o2, o3), 1) + x


def hourglass(Pm, stack, depth, x, sites=None):
    import torch.nn.functional as F
    m = P + "m%d." % stack

    def fwd(level, inp):
        up1 = conv_block(Pm, m + "b1_%d." % level, inp, sites)
        low = conv_block(Pm, m + "b2_%d." % level, F.avg_pool2d(inp, 2, stride=2), sites)
        low = fwd(level - 1, low) if level > 1 else conv_block(Pm, m + "b2_plus_%d." % level, low, sites)
        low = conv_block(Pm, m + "b3_%d." % level, low, sites)
        return up1 + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)
    return fwd(depth, x)


def stack_tail(Pm, s, t, sites=None):
    """l{s}(relu(bn_end{s}(conv_last{s}(t))))."""
    import torch.nn.functional as F
    t = F.conv2d(t, Pm[P + "conv_last%d.weight" % s], Pm[P + "conv_last%d.bias" % s])
    return F.conv2d(_norm_relu(Pm, P + "bn_end%d" % s, t, sites), Pm[P + "l%d.weight" % s], Pm[P + "l%d.bias" % s])


def forward(name, Pm, x, sites=None):
    module, o = CASES[name][0], opt(name)
    if module == "conv2":
        return conv_block(Pm, P + "conv2.", x, sites)
    if module == "m0":
        return hourglass(Pm, 0, o.hg_depth, x, sites)
    t = conv_block(Pm, P + "top_m_0.", hourglass(Pm, 0, o.hg_depth, conv_block(Pm, P + "conv2.", x, sites), sites), sites)
    return stack_tail(Pm, 0, t, sites)


def grads_of(name, x, G, dtype, want_sites=False):
    """(OrderedDict key -> gradient as float64 numpy - the parameters in param_keys order, then INPUT_KEY -, L, sites)."""
    import torch
    sd = state_dict(name)
    Pm = OrderedDict((k, torch.from_numpy(np.array(sd[k])).to(dtype).requires_grad_()) for k in param_keys(name))
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_()
    sites = [] if want_sites else None
    with torch.enable_grad():
        out = forward(name, Pm, xt, sites)
        L = (torch.from_numpy(np.ascontiguousarray(G)).to(dtype) * out).sum()
        got = torch.autograd.grad(L, list(Pm.values()) + [xt])
    res = OrderedDict((k, g.detach().double().numpy()) for k, g in zip(list(Pm) + [INPUT_KEY], got))
    return res, float(L.detach()), sites


kink_margin = sg.kink_margin


def input_quantities(g):
    """The input gradient [B,256,h,w] as grad_common.quantities stores it (rows: the images)."""
    return gc.quantities(INPUT_KEY, g)


def compare(gold, grads, factor=8.0):
    """sr_grad_common.compare's rule: [(name, max |g - g64| / max |g64|, factor * max(e_ref, 2^-20))] per stored quantity."""
    return sg.compare(gold, grads, factor)


worst = sg.worst
