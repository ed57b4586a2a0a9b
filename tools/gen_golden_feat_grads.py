"""Generate tests/golden/feat_grads_<case>.npz: the reference's own gradients of the classifier loss terms with respect to the feature
maps, on the CPU.

Build container only, through tools/ref_harness.py.  Per case of tests/feat_grad_common.py (inputs from seeds, no encoder):
  1. the kink-safe selection of tools/gen_golden_grads.py (its make_net and run: the reference in float64 on the 16 000 candidates,
     hooks on every hidden convolution, grad_common's KINK_REL and EDGE); the first N safe indices per image are kept;
  2. on the kept points: im_feat_list_lr / im_feat_list_hr set by hand as LEAF tensors with requires_grad_(), query_mr(labels) +
     query_sr(labels), error = mlp1 get_error_lr() + mlp2 get_error_hr() + dispweight get_error_disp_1(), error.backward() - in
     float64, and again in float32;
  3. stored: the kept indices, the float64 error, per tensor (lr0 .. lr{S-1} [B,D,hl,wl], hr [B,64,hh,wh]) the float64 gradient,
     whole, and e_ref = max |fp32 - fp64| / max |fp64|.
Before anything is written the kept set is checked again for kink-safety and feat_grad_common.check_coverage must hold (d48: an hr
pixel that receives nothing, an lr pixel with 8 or more taps within one chunk, a pixel fed from both chunks); the counts are printed.

    python tools/gen_golden_feat_grads.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_harness as rh  # noqa: E402
import gen_golden_grads as gg  # noqa: E402
import grad_common as gc  # noqa: E402
import feat_grad_common as fg  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def run(net, x, dtype):
    """(OrderedDict tensor name -> d error / d map as float64 numpy, error) on inputs x."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    B, S = len(x["feat_hr"]), len(x["feat_lr"][0])
    maps_lr = [T(np.stack([x["feat_lr"][b][s] for b in range(B)])).requires_grad_() for s in range(S)]
    map_hr = T(np.stack(x["feat_hr"])).requires_grad_()
    net.im_feat_list_lr, net.im_feat_list_hr = maps_lr, [map_hr]
    net.zero_grad()
    with torch.enable_grad(), rh.quiet():
        net.query_mr(T(x["points_mr"]), T(x["calib_mr"]), labels=T(x["lab_lr"][:, None]))
        net.query_sr(T(x["points_sr"]), T(x["calib_sr"]), labels=T(x["lab_hr"][:, None]))
        w1, w2, wd = gc.LOSS_WEIGHTS
        error = w1 * net.get_error_lr() + w2 * net.get_error_hr() + wd * net.get_error_disp_1()
        error.backward()
    return fg.named([m.grad.detach().double().numpy().copy() for m in maps_lr], map_hr.grad.detach().double().numpy().copy()), \
        float(error.detach())


def gen(name):
    S, B, N, _, _ = fg.CASES[name]
    x = fg.inputs(name)
    net64 = gg.make_net(name, torch.float64)
    margin, edge, _, _ = gg.run(net64, x, torch.float64, False)
    safe = (margin >= gc.KINK_REL) & (edge >= gc.EDGE)
    print(name, "kink-safe fraction", float(safe.mean()), file=sys.__stdout__)
    keep = []
    for b in range(B):
        idx = np.nonzero(safe[b])[0]
        assert idx.size >= N, (name, b, idx.size)
        keep.append(idx[:N])
    keep = np.stack(keep).astype(np.int32)
    xk = gc.kept(x, keep)
    margin, edge, _, _ = gg.run(net64, xk, torch.float64, False)
    if not ((margin >= gc.KINK_REL).all() and (edge >= gc.EDGE).all()):
        raise SystemExit("%s: the kept points are not kink-safe; nothing written" % name)
    cov = fg.coverage(name, xk)
    print(name, "coverage", cov, file=sys.__stdout__)
    fg.check_coverage(name, cov)
    g64, e64 = run(net64, xk, torch.float64)
    g32, e32 = run(gg.make_net(name, torch.float32), xk, torch.float32)
    out = {"keep": keep, "error": np.float64(e64)}
    worst = 0.0
    for k in fg.tensor_names(name):
        assert g64[k][0].size < gc.WHOLE, (k, g64[k].shape)          # stored whole
        out[k] = g64[k]
        out[k + "|e_ref"] = np.float64(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max())
        worst = max(worst, float(out[k + "|e_ref"]))
    path = fg.fixture_path(GOLD, name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(name, "error f64 %.9g f32 %.9g, worst e_ref %.3g, min margin %.3g, %d bytes" % (e64, e32, worst, float(margin.min()), size),
          file=sys.__stdout__)
    assert size < 1000000, (path, size)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in sys.argv[1:] or list(fg.CASES):
        gen(case)
