"""Generate tests/golden/hg_grads_<case>.npz: the reference's own gradients of L = <G, module(x)> with respect to the module's
parameters and its input, on the CPU, for the cases of tests/hg_grad_common.py (a ConvBlock, the HourGlass m0 at depth 1 and 2, and
a one-stack HGFilter).

Build container only, through tools/ref_harness.py.  Per case (weights and the upstream G from seeds):
  1. the input seed is searched, 0, 1, 2, ... (at most hg_grad_common.MAX_TRIES): the reference's ConvBlock / HourGlass / HGFilter
     run in float64 and in float32 with a forward hook on every GroupNorm that feeds a ReLU (bn1 - bn3 of each block, bn_end); a
     seed is kept when at every such site  min |z64| >= 16 max |z32 - z64|  (sr_grad_common.kink_margin);
  2. on that input: L.backward() in float64 and again in float32;
  3. stored (in parts of at most 900 000 bytes of data per file): the seed, the achieved margin, the number of site elements, L, and per
     parameter - and for the input, under "input" - the float64 gradient in grad_common.quantities' format with
     e_ref = max |fp32 - fp64| / max |fp64| per stored quantity.
The margin is asserted before anything is written.

    python tools/gen_golden_hg_grads.py [case ...]
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
import hg_grad_common as hg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900000


def make_filter(name, dtype):
    """The reference's image_filter_lr (an HGFilter) with the case's weights."""
    net = rh.build_net(rh.parse_opt(hg.flags(name)))
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in hg.state_dict(name).items()}, strict=True)
    return net.image_filter_lr.to(dtype)


def module_of(name, flt):
    kind = hg.CASES[name][0]
    if kind == "conv2":
        return flt.conv2, flt.conv2
    if kind == "m0":
        return flt.m0, flt.m0
    return (lambda x: flt(x)[0]), flt


def run(flt, name, x, dtype, want_grads):
    """(grads or None, L, sites) of the reference's module on x."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    fn, root = module_of(name, flt)
    sites = []
    keep = lambda mod, inp, out: sites.append(out.detach().clone())
    live = ("bn1", "bn2", "bn3")   # (bn4 belongs to the downsample path these blocks do not have)
    hs = [m.register_forward_hook(keep) for n, m in root.named_modules()
          if isinstance(m, torch.nn.GroupNorm) and (n.rsplit(".", 1)[-1] in live or n.startswith("bn_end"))]
    flt.zero_grad()
    xt = T(x).requires_grad_()
    try:
        with torch.enable_grad():
            L = (T(hg.upstream(name)) * fn(xt)).sum()
            if want_grads:
                L.backward()
    finally:
        for h in hs:
            h.remove()
    if not want_grads:
        return None, float(L.detach()), sites
    named = dict(flt.named_parameters())
    grads = OrderedDict()
    for k in hg.param_keys(name):
        grads[k] = named[k[len(hg.P):]].grad.detach().double().numpy().copy()
    grads[hg.INPUT_KEY] = xt.grad.detach().double().numpy().copy()
    return grads, float(L.detach()), sites


def gen(name):
    f64, f32 = make_filter(name, torch.float64), make_filter(name, torch.float32)
    seed, margin, count = None, 0.0, 0
    for s in range(hg.MAX_TRIES):
        x = hg.inputs(name, s)
        _, _, z64 = run(f64, name, x, torch.float64, False)
        _, _, z32 = run(f32, name, x, torch.float32, False)
        margin, count = hg.kink_margin(z64, z32)
        if margin >= hg.KINK_FACTOR:
            seed = s
            break
    if seed is None:
        raise SystemExit("%s: no kink-safe input among %d seeds; shrink the map, not the factor" % (name, hg.MAX_TRIES))
    x = hg.inputs(name, seed)
    g64, L64, z64 = run(f64, name, x, torch.float64, True)
    g32, L32, z32 = run(f32, name, x, torch.float32, True)
    margin, count = hg.kink_margin(z64, z32)
    assert margin >= hg.KINK_FACTOR, (name, seed, margin)
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
        path = hg.fixture_path(GOLD, name, i)
        np.savez_compressed(path, **part)
        sizes.append(os.path.getsize(path))
        assert sizes[-1] < 1000000, (path, sizes[-1])
    assert not os.path.exists(hg.fixture_path(GOLD, name, len(parts))), "a stale part of an earlier run lies behind the last one"
    print(name, "seed %d, margin %.1f over %d sites, L f64 %.9g f32 %.9g, worst e_ref %.3g, bytes %s" % (seed, margin, count, L64, L32, worst, sizes),
          file=sys.__stdout__)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in sys.argv[1:] or list(hg.CASES):
        gen(case)
