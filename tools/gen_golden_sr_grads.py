"""Generate tests/golden/sr_grads_<case>.npz: the reference's own gradients of
    L = <G_img, img_SR> + <G_lr, feature_lr> + <G_hr, image_filter_hr(feature_hr)>
with respect to every super_resolution.* convolution and image_filter_hr.conv5, on the CPU.

Build container only, through tools/ref_harness.py.  Per case of tests/sr_grad_common.py (weights, upstream gradients and images from
seeds):
  1. the image seed is searched, 0, 1, 2, ... (at most sr_grad_common.MAX_TRIES): the reference runs in float64 and in float32 with a
     forward hook on every convolution that feeds an activation and on the PixelShuffle (the input of the LeakyReLU behind it); a
     seed is kept when at every such site  min |z64| >= 16 max |z32 - z64|  (sr_grad_common.kink_margin);
  2. on that image: L.backward() in float64 and again in float32;
  3. stored (in parts of at most 900 000 bytes of data per file): the seed, the achieved margin, the number of sites, L, and per parameter the float64 gradient in
     grad_common.quantities' format with e_ref = max |fp32 - fp64| / max |fp64| per stored quantity.  A parameter autograd leaves
     without a gradient (the blocks without --residual) is stored as zeros.
The margin is asserted before anything is written.

    python tools/gen_golden_sr_grads.py [case ...]
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_harness as rh  # noqa: E402
import grad_common as gc  # noqa: E402
import sr_grad_common as sg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900000


def make_net(name, dtype):
    net = rh.build_net(rh.parse_opt(sg.flags(name)))
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sg.state_dict(name).items()}, strict=True)
    return net.to(dtype)


def hook_sites(net, sites):
    """Forward hooks that append every pre-activation of the super-resolution network to `sites`; returns the handles."""
    sr = net.super_resolution
    skip = {"last.2"} | {n for n, _ in sr.named_modules() if n.endswith(".body.2")}
    keep = lambda mod, inp, out: sites.append(out.detach().clone())
    hs = [m.register_forward_hook(keep) for n, m in sr.named_modules() if isinstance(m, torch.nn.Conv2d) and n not in skip]
    hs.append(sr.pixel_shuffle[0].register_forward_hook(keep))
    return hs


def run(net, name, x, dtype, want_grads):
    """(grads or None, L, sites) of the reference on images x."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    sites = []
    hs = hook_sites(net, sites)
    net.zero_grad()
    try:
        with torch.enable_grad(), rh.quiet():
            img, f_lr, f_hr = net.super_res(T(x))
            net.filter_hr(f_hr)
            L = sum((T(g) * t).sum() for g, t in zip(sg.upstream(name), (img, f_lr, net.im_feat_list_hr[0])))
            if want_grads:
                L.backward()
    finally:
        for h in hs:
            h.remove()
    if not want_grads:
        return None, float(L.detach()), sites
    named = dict(net.named_parameters())
    grads = OrderedDict()
    for k in sg.param_keys(name):
        g = named[k].grad
        grads[k] = (torch.zeros_like(named[k]) if g is None else g).detach().double().numpy().copy()
    return grads, float(L.detach()), sites


def gen(name):
    net64, net32 = make_net(name, torch.float64), make_net(name, torch.float32)
    seed, margin, count = None, 0.0, 0
    for s in range(sg.MAX_TRIES):
        x = sg.images(name, s)
        _, _, z64 = run(net64, name, x, torch.float64, False)
        _, _, z32 = run(net32, name, x, torch.float32, False)
        margin, count = sg.kink_margin(z64, z32)
        if margin >= sg.KINK_FACTOR:
            seed = s
            break
    if seed is None:
        raise SystemExit("%s: no kink-safe image among %d seeds; shrink the image, not the factor" % (name, sg.MAX_TRIES))
    x = sg.images(name, seed)
    g64, L64, z64 = run(net64, name, x, torch.float64, True)
    g32, L32, z32 = run(net32, name, x, torch.float32, True)
    margin, count = sg.kink_margin(z64, z32)
    assert margin >= sg.KINK_FACTOR, (name, seed, margin)
    out = {"seed": np.int64(seed), "margin": np.float64(margin), "sites": np.int64(count), "L": np.float64(L64)}
    worst = 0.0
    for k in g64:
        for (qn, q64), (_, q32) in zip(gc.quantities(k, g64[k]), gc.quantities(k, g32[k])):
            out[qn] = q64
            top = float(np.abs(q64).max())
            out[qn + "|e_ref"] = np.float64(np.abs(q32 - q64).max() / top if top > 0 else 0.0)
            worst = max(worst, float(out[qn + "|e_ref"]))
    # parts of at most PART_BYTES of raw data each: random float64 values do not compress, and no committed file may exceed 1 MiB
    parts, room = [{}], PART_BYTES
    for k, v in out.items():
        n = np.asarray(v).nbytes
        if n > room and parts[-1]:
            parts.append({})
            room = PART_BYTES
        parts[-1][k] = v
        room -= n
    sizes = []
    for i, part in enumerate(parts):
        path = sg.fixture_path(GOLD, name, i)
        np.savez_compressed(path, **part)
        sizes.append(os.path.getsize(path))
        assert sizes[-1] < 1000000, (path, sizes[-1])
    assert not os.path.exists(sg.fixture_path(GOLD, name, len(parts))), "a stale part of an earlier run lies behind the last one"
    print(name, "seed %d, margin %.1f over %d sites, L f64 %.9g f32 %.9g, worst e_ref %.3g, bytes %s" % (seed, margin, count, L64, L32, worst, sizes),
          file=sys.__stdout__)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in sys.argv[1:] or list(sg.CASES):
        gen(case)
