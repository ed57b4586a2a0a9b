"""Generate tests/golden/tail_grads_<case>.npz: the reference's own gradients of L = <G_out, out> + <G_next, next> of a stack's tail
with respect to the tail's parameters, its input ll and previous, on the CPU, for the cases of tests/tail_grad_common.py.

Build container only, through tools/ref_harness.py, after gen_golden_hg_grads.py.  The module under test is built from the
reference's own conv_last{s}, bn_end{s}, l{s}, bl{s}, al{s} of a two-stack HGFilter, in the order HGFilter.forward applies them.
Per case (weights, previous and the upstream gradients from seeds):
  1. the seed of ll is searched, 0, 1, 2, ... (at most tail_grad_common.MAX_TRIES): the modules run in float64 and in float32 with a
     forward hook on bn_end{s}; a seed is kept when  min |z64| >= 16 max |z32 - z64|  over the site (sr_grad_common.kink_margin);
  2. on that input: L.backward() in float64 and again in float32;
  3. stored (in parts of at most 900 000 bytes of data per file): the seed, the achieved margin, the number of site elements, L, and
     per parameter - and for ll under "input", for previous under "previous" - the float64 gradient in grad_common.quantities' format
     with e_ref = max |fp32 - fp64| / max |fp64| per stored quantity.
The margin is asserted before anything is written.

    python tools/gen_golden_tail_grads.py [case ...]
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
import tail_grad_common as tg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900000


def make_filter(name, dtype):
    """The reference's image_filter_lr (an HGFilter) with the case's weights."""
    net = rh.build_net(rh.parse_opt(tg.flags(name)))
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in tg.state_dict(name).items()}, strict=True)
    return net.image_filter_lr.to(dtype)


def run(flt, name, ll, dtype, want_grads):
    """(grads or None, L, sites) of the reference's tail modules on ll."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    s, last = tg.stack(name), tg.is_last(name)
    M = lambda n: flt._modules[n + str(s)]
    sites = []
    hook = M("bn_end").register_forward_hook(lambda mod, inp, out: sites.append(out.detach().clone()))
    flt.zero_grad()
    llt = T(ll).requires_grad_()
    prev = None if last else T(tg.previous(name)).requires_grad_()
    g_out, g_next = tg.upstream(name)
    try:
        with torch.enable_grad():
            a = torch.nn.functional.relu(M("bn_end")(M("conv_last")(llt)), True)
            out = M("l")(a)
            L = (T(g_out) * out).sum()
            if not last:
                L = L + (T(g_next) * (prev + M("bl")(a) + M("al")(out))).sum()
            if want_grads:
                L.backward()
    finally:
        hook.remove()
    if not want_grads:
        return None, float(L.detach()), sites
    named = dict(flt.named_parameters())
    grads = OrderedDict()
    for k in tg.param_keys(name):
        grads[k] = named[k[len(tg.P):]].grad.detach().double().numpy().copy()
    grads[tg.INPUT_KEY] = llt.grad.detach().double().numpy().copy()
    if not last:
        grads[tg.PREVIOUS_KEY] = prev.grad.detach().double().numpy().copy()
    return grads, float(L.detach()), sites


def gen(name):
    f64, f32 = make_filter(name, torch.float64), make_filter(name, torch.float32)
    seed, margin, count = None, 0.0, 0
    for s in range(tg.MAX_TRIES):
        ll = tg.inputs(name, s)
        _, _, z64 = run(f64, name, ll, torch.float64, False)
        _, _, z32 = run(f32, name, ll, torch.float32, False)
        margin, count = tg.kink_margin(z64, z32)
        if margin >= tg.KINK_FACTOR:
            seed = s
            break
    if seed is None:
        raise SystemExit("%s: no kink-safe input among %d seeds; shrink the map, not the factor" % (name, tg.MAX_TRIES))
    ll = tg.inputs(name, seed)
    g64, L64, z64 = run(f64, name, ll, torch.float64, True)
    g32, L32, z32 = run(f32, name, ll, torch.float32, True)
    margin, count = tg.kink_margin(z64, z32)
    assert margin >= tg.KINK_FACTOR, (name, seed, margin)
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
        path = tg.fixture_path(GOLD, name, i)
        np.savez_compressed(path, **part)
        sizes.append(os.path.getsize(path))
        assert sizes[-1] < 1000000, (path, sizes[-1])
    assert not os.path.exists(tg.fixture_path(GOLD, name, len(parts))), "a stale part of an earlier run lies behind the last one"
    print(name, "seed %d, margin %.1f over %d sites, L f64 %.9g f32 %.9g, worst e_ref %.3g, bytes %s" % (seed, margin, count, L64, L32, worst, sizes),
          file=sys.__stdout__)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in sys.argv[1:] or list(tg.CASES):
        gen(case)
