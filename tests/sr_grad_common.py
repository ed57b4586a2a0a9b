"""Inputs, the float64 restatement and the fixture format of the super-resolution gradient tests (tests/golden/sr_grads_*.npz,
tools/gen_golden_sr_grads.py).  Everything on the input side comes from seeds; a fixture holds the image seed the generator's kink
search settled on, the achieved kink margin, the reference's float64 gradients (grad_common.quantities' format) and the distance of its
own float32 gradients from them.

The loss, for a batch of images x [B,3,h,w] and seeded upstream gradients G_*:
    img_SR, feature_lr, feature_hr = super_resolution(x);  feat_hr = image_filter_hr.conv5(feature_hr)
    L = <G_img, img_SR> + <G_lr, feature_lr> + <G_hr, feat_hr>
The network, written here from the state-dict keys (scale s, LeakyReLU slope 0.2 unless noted):
    h    = lrelu(head.0(bicubic_s(x)))                                              [32, sh, sw]
    d_i  = lrelu(down{i}.0(previous, stride 2));  d_i = body{i}.{b}(d_i) for every block with --residual:
           t = relu(body.0(d)), d = body.2(t) + d;  d_i_f = lrelu(tail{i}.2(lrelu(tail{i}.0(d_i))))      i = 1, 2, 3
    bo   = lrelu(bottleneck.0(d3_f));             up1 = lrelu(shuffle(lrelu(bott2.0(cat(d3_f, bo)))))
    new2 = cat(d2_f, up1) = feature_lr;           up2 = lrelu(shuffle(lrelu(ups2.0(new2))))
    new3 = cat(d1_f, up2);                        up3 = lrelu(shuffle(lrelu(ups3.0(new3))))
    feature_hr = lrelu(ups4.0(cat(h, up3)));      img_SR = last.2(lrelu(last.0(feature_hr)))
An ACTIVATION SITE is the input of any lrelu / relu above.  A fixture is KINK-SAFE when at every site the float64 pre-activation z64
satisfies |z64| >= 16 max over that site of |z32 - z64| (z32: the float32 run): 4 for the library's 22-bit operands against fp32's
24, times a safety factor of 4."""
import os
from collections import OrderedDict

import numpy as np

import common
import grad_common as gc
from surs_amd import options, prng, weights

FLOOR = 2.0 ** -20        # four times grad_common.FLOOR: the library's forward rounds its operands to 22 bits
KINK_FACTOR = 16.0
MAX_TRIES = 500
_BASE = [f for f in common.FLAGS if f != "--residual"]
# name -> (flags beyond _BASE, (h, w) of the input image, B)
CASES = OrderedDict([
    ("tiny", (["--residual", "--n_block", "1", "1", "1"], (4, 8), 2)),
    ("odd", ([], (8, 12), 1)),
    ("blocks", (["--scale", "4", "--residual", "--n_block", "2", "0", "1"], (4, 8), 1)),
])
S = "super_resolution."


def flags(name):
    return _BASE + CASES[name][0]


def opt(name):
    return options.BaseOptions().parse(flags(name))


def fixture_path(golden_dir, name, part=0):
    return os.path.join(golden_dir, "sr_grads_%s%s.npz" % (name, "_p%d" % part if part else ""))


def load_fixture(golden_dir, name):
    """A case's fixture as one dict: sr_grads_<name>.npz joined with sr_grads_<name>_p1.npz, _p2, ... (the generator cuts a case into
    parts to keep every file below 1 MiB)."""
    out, part = {}, 0
    while os.path.exists(fixture_path(golden_dir, name, part)):
        out.update(np.load(fixture_path(golden_dir, name, part)))
        part += 1
    if not out:
        raise FileNotFoundError(fixture_path(golden_dir, name))
    return out


_sd_cache = {}


def state_dict(name):
    """weights.synthetic_state_dict for the case's flags (float32 numpy, every key)."""
    if name not in _sd_cache:
        _sd_cache[name] = weights.synthetic_state_dict(opt(name), seed=0)
    return _sd_cache[name]


def conv_modules(n_block):
    """The module names of the super-resolution convolutions (a set: the order of the keys is the state dict's)."""
    mods = ["head.0", "bottleneck.0", "bott2.0", "ups2.0", "ups3.0", "ups4.0", "last.0", "last.2"]
    for i, nb in zip((1, 2, 3), n_block):
        mods += ["down%d.0" % i, "tail%d.0" % i, "tail%d.2" % i] + ["body%d.%d.body.%d" % (i, b, p) for b in range(nb) for p in (0, 2)]
    return mods


def param_keys(name):
    """The keys a gradient exists for, in state_dict() order: every super_resolution.* convolution and image_filter_hr.conv5."""
    mods = {S + m for m in conv_modules(opt(name).n_block)} | {"image_filter_hr.conv5"}
    return [k for k in state_dict(name) if k.rsplit(".", 1)[0] in mods]


def shapes(name):
    """(image [B,3,h,w], img_SR, feature_lr, feat_hr) shapes."""
    _, (h, w), B = CASES[name]
    s = opt(name).scale
    c5 = state_dict(name)["image_filter_hr.conv5.weight"].shape[0]
    return (B, 3, h, w), (B, 3, s * h, s * w), (B, 256, s * h // 4, s * w // 4), (B, c5, s * h, s * w)


def images(name, seed):
    return prng.uniform("sr_grad_image_" + name, seed, shapes(name)[0], 0.0, 1.0)


def upstream(name):
    """(G_img, G_lr, G_hr): seeded uniform [-1, 1) tensors of the outputs' shapes."""
    sh = shapes(name)
    return tuple(prng.uniform("sr_grad_G%d_%s" % (i, name), 11 + i, sh[1 + i], -1.0, 1.0) for i in range(3))


# ------------------------------------------------------------------ the restatement (torch on the CPU, any dtype)
def forward(P, x, o, sites=None):
    """(img_SR, feature_lr, feature_hr, feat_hr) of images x [B,3,h,w] under parameters P (key -> tensor) and options o.  sites: a
    list that receives every pre-activation, detached, in execution order."""
    import torch
    import torch.nn.functional as F

    def conv(mod, t, stride=1):
        return F.conv2d(t, P[S + mod + ".weight"], P[S + mod + ".bias"], stride=stride, padding=1)

    def act(z, slope=0.2):
        if sites is not None:
            sites.append(z.detach().clone())
        return torch.where(z > 0, z, slope * z)

    def shuffle(z):   # conv -> lrelu -> PixelShuffle(2) -> lrelu
        return act(F.pixel_shuffle(act(z), 2))

    def stage(i, t):
        d = act(conv("down%d.0" % i, t, 2))
        if o.residual:
            for b in range(o.n_block[i - 1]):
                d = conv("body%d.%d.body.2" % (i, b), act(conv("body%d.%d.body.0" % (i, b), d), 0.0)) + d
        return act(conv("tail%d.2" % i, act(conv("tail%d.0" % i, d))))

    up = F.interpolate(x, scale_factor=o.scale, mode="bicubic", align_corners=False)
    h = act(conv("head.0", up))
    d1_f = stage(1, h)
    d2_f = stage(2, d1_f)
    d3_f = stage(3, d2_f)
    bo = act(conv("bottleneck.0", d3_f))
    new2 = torch.cat((d2_f, shuffle(conv("bott2.0", torch.cat((d3_f, bo), 1)))), 1)
    new3 = torch.cat((d1_f, shuffle(conv("ups2.0", new2))), 1)
    fin = torch.cat((h, shuffle(conv("ups3.0", new3))), 1)
    new_fin = act(conv("ups4.0", fin))
    img = conv("last.2", act(conv("last.0", new_fin)))
    feat_hr = F.conv2d(new_fin, P["image_filter_hr.conv5.weight"], P["image_filter_hr.conv5.bias"])
    return img, new2, new_fin, feat_hr


def grads_of(name, x, G, dtype, want_sites=False, use=(True, True, True)):
    """(OrderedDict key -> gradient as float64 numpy, L, sites) of the loss above in `dtype`; use: which of the three terms enter.
    A parameter the forward does not touch (the blocks without --residual) gets zeros."""
    import torch
    o = opt(name)
    sd = state_dict(name)
    P = OrderedDict((k, torch.from_numpy(np.array(sd[k])).to(dtype).requires_grad_()) for k in param_keys(name))
    sites = [] if want_sites else None
    with torch.enable_grad():
        img, f_lr, _, f_hr = forward(P, torch.from_numpy(np.ascontiguousarray(x)).to(dtype), o, sites)
        L = sum((torch.from_numpy(np.ascontiguousarray(g)).to(dtype) * t).sum() for g, t, u in zip(G, (img, f_lr, f_hr), use) if u)
        got = torch.autograd.grad(L, list(P.values()), allow_unused=True)
    out = OrderedDict((k, (torch.zeros_like(p) if g is None else g).detach().double().numpy()) for (k, p), g in zip(P.items(), got))
    return out, float(L.detach()), sites


def kink_margin(sites64, sites32):
    """min over the activation sites of min |z64| / max |z32 - z64| (inf where the two runs agree exactly), and the site count."""
    m, count = np.inf, 0
    for a, b in zip(sites64, sites32):
        a, b = a.double().numpy(), b.double().numpy()
        d = float(np.abs(a - b).max())
        count += a.size
        if d > 0:
            m = min(m, float(np.abs(a).min()) / d)
    return m, count


# ------------------------------------------------------------------ the fixture format (grad_common.quantities)
def compare(gold, grads, factor=8.0, scale=1.0):
    """[(name, deviation relative to the reference's max-abs, bound)] for every stored quantity t of every gradient:
    max |g / scale - g64| / max |g64| against factor * max(e_ref(t), 2^-20).  A reference gradient that is zero throughout (a block
    the forward does not run) must be met exactly."""
    out = []
    for key, g in grads.items():
        for qname, got in gc.quantities(key, np.asarray(g, np.float64) / scale):
            ref = gold[qname]
            top = float(np.abs(ref).max())
            dev = float(np.abs(got - ref).max()) / top if top > 0 else (0.0 if not np.abs(got).max() else np.inf)
            out.append((qname, dev, factor * max(float(gold[qname + "|e_ref"]), FLOOR)))
    return out


def worst(rows):
    """(name, deviation / bound) of the row closest to (or furthest beyond) its bound."""
    name, dev, bound = max(rows, key=lambda r: r[1] / r[2])
    return name, dev / bound
