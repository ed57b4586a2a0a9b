"""Generate tests/golden/train_step_<case>.npz and tests/golden/samples_prob.ply from the reference on the CPU.

Build container only, through tools/ref_harness.py.  For the cases, loss-weight variants and parameter sets of
tests/train_step_common.py: the reference's SuRSNet.forward error (train mode) in float64 and in float32, before and after one plain
SGD step (momentum 0) on the set's parameters alone, p -= lr * d error / d p from error.backward(), with the smallest learning rate of
the ladder that moves the float64 error by at least STEP_RATIO resolutions - asserted before anything is written.  A set the variant's
error does not depend on must have no (or an all-zero) gradient in the reference: asserted, stored with equal error values.

samples_prob.ply is lib/sample_util.py's save_samples_truncted_prob on seeded points and probabilities.

    python tools/gen_golden_train_step.py [case ...]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_harness as rh  # noqa: E402
import train_step_common as ts  # noqa: E402
import sample_ply_common as sp  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def make_net(case, variant, dtype):
    net = rh.build_net(rh.parse_opt(ts.flags(case, variant)))
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in ts.state_dict(case).items()}, strict=True)
    net.train()
    return net.to(dtype)


def error_of(net, x, dtype):
    T = lambda k: torch.from_numpy(x[k].copy()).to(dtype)
    with rh.quiet():
        _, err, _ = net.forward(T("images_lr"), T("images_hr"), T("points_lr"), T("points_hr"), T("calibs"),
                                labels_lr=T("labels_lr"), labels_hr=T("labels_hr"))
    return err


def gradients(net, x, dtype):
    """(error before, {parameter name: gradient}) of one backward."""
    net.zero_grad()
    with torch.enable_grad():
        err = error_of(net, x, dtype)
        err.backward()
    return float(err.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def stepped_error(net, x, dtype, grads, keys, lr):
    """The error after p -= lr g on `keys`; the parameters are put back."""
    named = dict(net.named_parameters())
    todo = [(named[k], grads[k]) for k in keys if k in named and k in grads]
    with torch.no_grad():
        saved = [p.detach().clone() for p, _ in todo]
        for p, g in todo:
            p.add_(g, alpha=-lr)
        e = float(error_of(net, x, dtype))
        for (p, _), s in zip(todo, saved):
            p.copy_(s)
    return e


def gen(case):
    x = ts.inputs(case)
    rows = []
    for variant in ts.VARIANTS:
        n64, n32 = make_net(case, variant, torch.float64), make_net(case, variant, torch.float32)
        b64, g64 = gradients(n64, x, torch.float64)
        b32, g32 = gradients(n32, x, torch.float32)
        for which in ts.SETS:
            keys = ts.set_keys(case, which)
            if not ts.live(variant, which):
                assert all(k not in g64 or not g64[k].abs().max() > 0 for k in keys), (case, variant, which)
                rows.append(dict(variant=variant, set=which, lr=1.0, e64=[b64, b64], e32=[b32, b32], ratio=0.0, live=False))
                continue
            assert any(k in g64 and g64[k].abs().max() > 0 for k in keys), (case, variant, which)
            row = None
            for lr in ts.LADDER:
                a64, a32 = stepped_error(n64, x, torch.float64, g64, keys, lr), stepped_error(n32, x, torch.float32, g32, keys, lr)
                row = dict(variant=variant, set=which, lr=lr, e64=[b64, a64], e32=[b32, a32], live=True)
                row["ratio"] = abs(a64 - b64) / ts.resolution(row)
                print(case, variant, which, "lr %g: e64 %.9g -> %.9g, e32 - e64 %.3g / %.3g, |d64| / r = %.1f" % (
                    lr, b64, a64, b32 - b64, a32 - a64, row["ratio"]), file=sys.__stdout__)
                if np.isfinite(a64) and row["ratio"] >= ts.STEP_RATIO:
                    break
            assert np.isfinite(row["e64"][1]) and row["ratio"] >= ts.STEP_RATIO, (case, variant, which, row)
            rows.append(row)
    path = ts.fixture_path(GOLD, case)
    np.savez_compressed(path, rows=np.array(json.dumps(rows)))
    print("wrote", path, os.path.getsize(path), "bytes", file=sys.__stdout__)


def gen_ply():
    ns = rh.load_reference()
    with rh.quiet():
        from lib import sample_util
    pts, prob = sp.samples()
    sample_util.save_samples_truncted_prob(os.path.join(GOLD, "samples_prob.ply"), pts, prob)
    print("wrote samples_prob.ply", os.path.getsize(os.path.join(GOLD, "samples_prob.ply")), "bytes", file=sys.__stdout__)
    del ns


if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_ply()
    for case in sys.argv[1:] or list(ts.CASES):
        gen(case)
