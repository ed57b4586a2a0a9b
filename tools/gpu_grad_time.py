"""Times the classifier gradients at a training-sized call: S = 3 maps, B = 2 images, N = 6000 points per
image (the reference's --batch_size and --num_sample_inout), full-size feature maps (256 x 256^2, 64 x 1024^2), for the released
shape and s1 (the 512-wide pair of tests/test_gpu_mlp_shapes.py).

  grads     (a) forward_backward's gradient part: native.mlp_grads, one call per image, the second accumulating
  features      the same calls with feat_grads: the parameter gradients and d error / d (the S lr maps and the hr map), every image
                into maps of its own (--features; full-size maps: 3 x 64 MiB + 256 MiB per image, zeroed by each call)
  grads_parent  (a) on another build of the library (--parent-lib FILE: the parent commit's libsurs_hip.so) - the parameter-only call
                launches the same kernels in both, so the two must agree within the spread the rounds show for either
  query     (b) the stacks query of forward() alone: an lr-only pass on one point set, an hr-only pass on another, per image
  autograd  (c) torch autograd, fp32, on the same GPU: this tool's own torch.nn.functional restatement of the two classifiers
                (conv1d, leaky_relu, sigmoid, the three loss terms) on PRE-GATHERED inputs [B S, c0, N] - forward, backward to
                the classifier parameters.  What a user would otherwise reach for; it does not pay for the gather.

Every measurement runs in a process of its own, ROUNDS times, the variants alternating, each child under a time limit; a host clock
around work that ends in a device synchronise.  Prints one JSON line per child and a summary (min / median / max ms over the rounds).

    python tools/gpu_grad_time.py [--rounds 3] [--out FILE] [--features] [--parent-lib FILE] [--kinds grads features ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
S1 = ["--mlp_dim_lr", "321", "512", "256", "128", "1", "--mlp_dim_hr", "322", "512", "256", "128", "1",
      "--mlp_res_layers_lr", "1", "2", "3", "--mlp_res_layers_hr", "1", "2", "3"]
B, N, S = 2, 6000, 3


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.nn.functional as F
    if args.child == "grads_parent":
        # an older build lacks the entries added since: the binding checks every declared symbol on load, so drop what is not there
        import ctypes
        from surs_amd import _lib
        _lib.LIB_PATH = os.path.abspath(args.parent_lib)
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib._SIGS if not hasattr(old, k)]:
            del _lib._SIGS[name]
    import common
    import gpu_common as g
    from surs_amd import native, options, prng, weights
    dev = g.dev()
    cal = common.CALIB.reshape(-1)[:12]
    opt = options.BaseOptions().parse(common.FLAGS + (S1 if args.shape == "s1" else []))
    sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
    shapes = native.mlp_shapes(sd, opt)
    pa = [torch.from_numpy(weights.synthetic_points(N, seed=30 + b)).to(dev) for b in range(B)]
    pb = [torch.from_numpy(weights.synthetic_points(N, seed=40 + b)).to(dev) for b in range(B)]
    gen = torch.Generator().manual_seed(1)
    lab = [(torch.rand((B, N), generator=gen) > 0.5).float().to(dev) for _ in range(2)]
    w = (0.5, 2.0, 1.5)

    def timed(f, reps):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    out = dict(child=args.child, shape=args.shape)
    if args.child in ("grads", "grads_parent", "features", "query"):
        fh = g.upload_nhwc(prng.uniform("feat_hr", 3, (64, 1024, 1024), -1.0, 1.0))
        maps = [g.upload_nhwc(prng.uniform("feat_lr", 3 + s, (256, 256, 256), -1.0, 1.0)) for s in range(S)]
    if args.child in ("grads", "grads_parent"):
        params = native.MlpParams(sd, dev, shapes)
        ws = torch.empty(native.mlp_grad_workspace_bytes(shapes) // 4, dtype=torch.float32, device=dev)
        grads = native.mlp_grads(pa[0], pb[0], cal, cal, 512, 200.0, maps, fh, params, lab[0][0], lab[1][0], w, B * N, workspace=ws)

        def f():
            for b in range(B):
                native.mlp_grads(pa[b], pb[b], cal, cal, 512, 200.0, maps, fh, params, lab[0][b], lab[1][b], w, B * N, grads=grads,
                                 accumulate=b > 0, workspace=ws)
        out["ms"] = timed(f, 20)
        out["workspace_mb"] = ws.numel() * 4 / 2 ** 20
    elif args.child == "features":
        params = native.MlpParams(sd, dev, shapes)
        ws = torch.empty(native.mlp_grad_features_workspace_bytes(shapes) // 4, dtype=torch.float32, device=dev)
        fgs = [native.FeatGrads.like(maps, fh, dev) for _ in range(B)]
        grads = native.mlp_grads(pa[0], pb[0], cal, cal, 512, 200.0, maps, fh, params, lab[0][0], lab[1][0], w, B * N, workspace=ws)

        def f():
            for b in range(B):
                native.mlp_grads(pa[b], pb[b], cal, cal, 512, 200.0, maps, fh, params, lab[0][b], lab[1][b], w, B * N, grads=grads,
                                 accumulate=b > 0, workspace=ws, feat_grads=fgs[b])
        out["ms"] = timed(f, 20)
        out["workspace_mb"] = ws.numel() * 4 / 2 ** 20
    elif args.child == "query":
        given = torch.rand((S, N)).to(dev)
        if native.is_default_mlp(shapes):
            blob, ws = g.blob("bf16"), native.Workspace(dev)
            st = lambda p, **k: native.query_points_stacks(p, cal, 512, 200.0, maps, fh, blob, ws, **k)
        else:
            gm = native.pack_mlp_generic(sd, dev, shapes)
            st = lambda p, **k: native.query_points_generic_stacks(p, cal, 512, 200.0, maps, fh, gm, **k)
        out["ms"] = timed(lambda: [(st(p, lr_only=True), st(q, p_lr=given)) for p, q in zip(pa, pb)], 50)
    else:
        P = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}
        xl = torch.rand((B * S, shapes[0][0][0], N), generator=gen).to(dev) * 2 - 1          # pre-gathered rows of both point sets
        xh = torch.rand((B * S, shapes[0][0][0], N), generator=gen).to(dev) * 2 - 1
        mask = [(torch.rand((B * S, 1, N), generator=gen) > 0.17).float().to(dev) for _ in range(2)]
        ll, lh = (l.repeat_interleave(S, 0)[:, None] for l in lab)                             # row b S + s

        def mlp(prefix, dims, res, x):
            y = x
            for l in range(len(dims) - 1):
                y = F.conv1d(torch.cat([y, x], 1) if l in res else y, P[prefix + "conv%d.weight" % l], P[prefix + "conv%d.bias" % l])
                if l != len(dims) - 2:
                    y = F.leaky_relu(y)
            return torch.sigmoid(y)

        def f():
            for p in P.values():
                p.grad = None
            q = mask[0] * mlp("mlp_lr.", *shapes[0], xl)
            r = mask[1] * mlp("mlp_hr.", *shapes[1], torch.cat([xh, q], 1))
            last = slice(S - 1, None, S)
            err = w[0] * F.mse_loss(q, ll) + w[1] * F.mse_loss(r, lh) + w[2] * F.mse_loss(lh[last] - ll[last], r[last] - q[last])
            err.backward()
        out["ms"] = timed(f, 20)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["grads", "grads_parent", "features", "query", "autograd"])
    ap.add_argument("--features", action="store_true", help="also time the call that returns the feature-map gradients")
    ap.add_argument("--parent-lib", help="also time the parameter-only call on this build of libsurs_hip.so")
    ap.add_argument("--kinds", nargs="+", help="the measurements to run (default: grads query autograd, + what the flags add)")
    ap.add_argument("--shape", choices=["released", "s1"], default="released")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    kinds = args.kinds or (["grads"] + (["grads_parent"] if args.parent_lib else []) + (["features"] if args.features else [])
                           + ["query", "autograd"])
    if "grads_parent" in kinds and not args.parent_lib:
        raise SystemExit("grads_parent needs --parent-lib")
    results = []
    for r in range(args.rounds):
        for shape in ("released", "s1"):
            for kind in kinds:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", shape]
                if kind == "grads_parent":
                    cmd += ["--parent-lib", args.parent_lib]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:   # nothing more is started on the device after a failure
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
                line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
                print(line, flush=True)
                results.append(json.loads(line))
    summary = {}
    for d in results:
        summary.setdefault("%s %s" % (d["shape"], d["child"]), []).append(d["ms"])
    summary = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), runs=v) for k, v in summary.items()}
    for shape in ("released", "s1"):
        for a, b in (("grads", "autograd"), ("grads", "query"), ("grads", "grads_parent"), ("features", "grads")):
            if shape + " " + a in summary and shape + " " + b in summary:
                summary["%s %s / %s (medians)" % (shape, a, b)] = summary["%s %s" % (shape, a)]["median"] / summary["%s %s" % (shape, b)]["median"]
    text = json.dumps(dict(rounds=args.rounds, B=B, N=N, S=S, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
