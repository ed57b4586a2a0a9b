"""Generate tests/golden/mlp_grads_<case>.npz (and <case>_hr.npz where one file would pass 1 MiB): the reference's own gradients of the classifier loss terms, on the CPU.

Build container only, through tools/ref_harness.py.  Per case of tests/grad_common.py (inputs from seeds, feature maps set by hand,
no encoder):
  1. the reference in float64 (net.double()) evaluates query_mr / query_sr on the 16 000 candidate points of every image; forward
     hooks on every hidden convolution give the pre-activations, from which the kink-safe indices follow (grad_common's definition,
     layer maxima over all candidates); the first N of them per image are kept;
  2. on the kept points: query_mr(labels) + query_sr(labels), error = mlp1 get_error_lr() + mlp2 get_error_hr() + dispweight
     get_error_disp_1(), error.backward() - in float64, and again in float32;
  3. stored: the kept indices, and per quantity of grad_common.quantities (a tensor below 65 536 elements whole, else its row sums,
     column sums and 2 048 seeded elements) the float64 value and e_ref = max |fp32 - fp64| / max |fp64|.
The kept set is checked again for kink-safety (on the kept points' own layer maxima, through the hooks) before anything is written.

    python tools/gen_golden_grads.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_harness as rh  # noqa: E402
import grad_common as gc  # noqa: E402
from surs_amd import weights  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def make_net(name, dtype):
    net = rh.build_net(rh.parse_opt(gc.flags(name)))
    sd = weights.synthetic_state_dict(gc.opt(name), seed=0)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return net.to(dtype)


def run(net, x, dtype, want_grads):
    """query_mr + query_sr on inputs x; (margin [B,N], edge [B,N]) from hooks, or the gradients of the three terms."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    B, S = len(x["feat_hr"]), len(x["feat_lr"][0])
    net.im_feat_list_lr = [T(np.stack([x["feat_lr"][b][s] for b in range(B)])) for s in range(S)]
    net.im_feat_list_hr = [T(np.stack(x["feat_hr"]))]
    stats = {}
    hooks = []
    for m in ("mlp_lr", "mlp_hr"):
        L = len(getattr(net, m).filters)
        for l in range(L - 1):
            def hook(mod, i, o, key=(m, l)):
                a = o.detach().abs()                        # [B, units, N]
                low, top = stats.get(key, (None, 0.0))
                cur = a.min(1).values
                stats[key] = (cur if low is None else torch.minimum(low, cur), max(top, float(a.max())))
            hooks.append(getattr(net, m)._modules["conv%d" % l].register_forward_hook(hook))
    net.zero_grad()
    with torch.set_grad_enabled(want_grads), rh.quiet():
        net.query_mr(T(x["points_mr"]), T(x["calib_mr"]), labels=T(x["lab_lr"][:, None]))
        net.query_sr(T(x["points_sr"]), T(x["calib_sr"]), labels=T(x["lab_hr"][:, None]))
        w1, w2, wd = gc.LOSS_WEIGHTS
        error = w1 * net.get_error_lr() + w2 * net.get_error_hr() + wd * net.get_error_disp_1()
        if want_grads:
            error.backward()
    for h in hooks:
        h.remove()
    N = x["points_mr"].shape[2]
    margin = np.full((B, N), np.inf)
    for low, top in stats.values():
        margin = np.minimum(margin, low.double().numpy() / max(1.0, top))
    edge = np.full((B, N), np.inf)
    for pts, cal in ((x["points_mr"], x["calib_mr"]), (x["points_sr"], x["calib_sr"])):
        for b in range(B):
            xyz = gc.project(pts[b], cal[b])
            edge[b] = np.minimum(edge[b], np.min(np.abs(np.abs(xyz[:2]) - 1.0), 0))
    grads = None
    if want_grads:
        grads = {k: p.grad.detach().double().numpy().copy() for k, p in net.named_parameters() if k.startswith("mlp_")}
    return margin, edge, grads, float(error.detach())


def gen(name):
    _, S, B, N = gc.CASES[name]
    x = gc.inputs(name)
    net64 = make_net(name, torch.float64)
    margin, edge, _, _ = run(net64, x, torch.float64, False)
    safe = (margin >= gc.KINK_REL) & (edge >= gc.EDGE)
    print(name, "kink-safe fraction", float(safe.mean()), file=sys.__stdout__)
    keep = []
    for b in range(B):
        idx = np.nonzero(safe[b])[0]
        assert idx.size >= N, (name, b, idx.size)
        keep.append(idx[:N])
    keep = np.stack(keep).astype(np.int32)
    xk = gc.kept(x, keep)
    margin, edge, g64, e64 = run(net64, xk, torch.float64, True)
    if not ((margin >= gc.KINK_REL).all() and (edge >= gc.EDGE).all()):
        raise SystemExit("%s: the kept points are not kink-safe; nothing written" % name)
    _, _, g32, e32 = run(make_net(name, torch.float32), xk, torch.float32, True)
    out = {"keep": keep, "error": np.float64(e64)}
    worst = 0.0
    for key in g64:
        for (qn, q64), (_, q32) in zip(gc.quantities(key, g64[key]), gc.quantities(key, g32[key])):
            out[qn] = q64
            out[qn + "|e_ref"] = np.float64(np.abs(q32 - q64).max() / np.abs(q64).max())
            worst = max(worst, float(out[qn + "|e_ref"]))
    outside = float(np.mean([gc.point_rows(xk["feat_lr"][b][0], xk["feat_hr"][b], xk["points_mr"][b], xk["calib_mr"][b])[1] == 0
                             for b in range(B)]))
    path, path_hr = gc.fixture_path(GOLD, name), gc.fixture_path(GOLD, name, "_hr")
    np.savez_compressed(path, **out)
    sizes = [os.path.getsize(path)]
    if os.path.exists(path_hr):
        os.remove(path_hr)
    if sizes[0] >= 1000000:   # every committed file below 1 MiB: mlp_hr's quantities in a file of their own
        np.savez_compressed(path, **{k: v for k, v in out.items() if not k.startswith("mlp_hr.")})
        np.savez_compressed(path_hr, **{k: v for k, v in out.items() if k.startswith("mlp_hr.")})
        sizes = [os.path.getsize(path), os.path.getsize(path_hr)]
    print(name, "error f64 %.9g f32 %.9g, worst e_ref %.3g, min margin %.3g, outside %.3f, %s bytes" % (
        e64, e32, worst, float(margin.min()), outside, sizes), file=sys.__stdout__)
    assert max(sizes) < 1000000, (path, sizes)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in sys.argv[1:] or list(gc.CASES):
        gen(case)
