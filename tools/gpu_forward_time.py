"""Times what the validation forward added to the point path.

1. stacks:  the stacks entry at a training-sized call - S = 3 maps, B = 2 images, N = 6000 points per image (the reference's
            --batch_size and --num_sample_inout), full-size feature maps (256 x 256^2, 64 x 1024^2) - against S separate calls of the
            single-map entry on the same maps, for the released shape (surs_query_points_stacks: the layer kernels sequenced in the
            library) and s1 (surs_query_points_generic_stacks: one launch): the both-classifier form and forward()'s pair (lr only on
            one point set, hr only on another).
2. single:  the single-map 50 000-point query (tools/gpu_points_time.py's call; s1: the fused evaluator) on this tree's library and,
            with --parent-lib, on another build of it (the parent commit's), to hold the existing kernels' time to the parent's spread.

Every measurement runs in a process of its own, ROUNDS times, the variants alternating; a host clock around work that ends in a device
synchronise.  Prints one JSON line per child and a summary (min / median / max ms over the rounds).

    python tools/gpu_forward_time.py [--parent-lib PATH] [--rounds 3] [--out FILE]
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
NEW_ENTRIES = ("surs_query_points_generic_stacks", "surs_query_points_stacks", "surs_forward_losses", "surs_forward_losses_workspace_bytes")


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.lib:
        from surs_amd import _lib
        _lib.LIB_PATH = args.lib
        for k in NEW_ENTRIES:      # (a build from before these entries)
            _lib._SIGS.pop(k, None)
    import numpy as np
    import torch
    import common
    import gpu_common as g
    from surs_amd import native, options, prng, weights
    dev = g.dev()
    cal = common.CALIB.reshape(-1)[:12]
    fh = g.upload_nhwc(prng.uniform("feat_hr", 3, (64, 1024, 1024), -1.0, 1.0))
    maps = [g.upload_nhwc(prng.uniform("feat_lr", 3 + s, (256, 256, 256), -1.0, 1.0)) for s in range(3 if args.child == "stacks" else 1)]
    gm = None
    if args.shape == "s1":
        opt = options.BaseOptions().parse(common.FLAGS + S1)
        sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
        gm = native.pack_mlp_generic(sd, dev, native.mlp_shapes(sd, opt))
    else:
        blob, ws = g.blob("bf16"), native.Workspace(dev)

    def timed(f, reps):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    out = dict(child=args.child, shape=args.shape, lib=args.lib or "tree")
    if args.child == "single":
        pts = torch.from_numpy(weights.synthetic_points(50000, seed=2)).to(dev)
        if gm is None:
            f = lambda: native.query_points(pts, cal, 512, 200.0, maps[0], fh, blob, ws)
        else:
            f = lambda: native.query_points_generic(pts, cal, 512, 200.0, maps[0], fh, gm)
        out["ms"] = timed(f, 100)
    else:
        B, N, S = 2, 6000, 3
        pa = [torch.from_numpy(weights.synthetic_points(N, seed=30 + b)).to(dev) for b in range(B)]
        pb = [torch.from_numpy(weights.synthetic_points(N, seed=40 + b)).to(dev) for b in range(B)]
        given = torch.rand((S, N)).to(dev)
        if gm is None:
            st = lambda p, **k: native.query_points_stacks(p, cal, 512, 200.0, maps, fh, blob, ws, **k)
            one = lambda p, m: native.query_points(p, cal, 512, 200.0, m, fh, blob, ws)
            one_hr = lambda p, m, pl: native.query_points_hr(p, cal, 512, 200.0, m, fh, blob, ws, pl)
        else:
            st = lambda p, **k: native.query_points_generic_stacks(p, cal, 512, 200.0, maps, fh, gm, **k)
            one = lambda p, m: native.query_points_generic(p, cal, 512, 200.0, m, fh, gm)
            one_hr = lambda p, m, pl: native.query_points_generic(p, cal, 512, 200.0, m, fh, gm, p_lr=pl)
        rows = [given[s].contiguous() for s in range(S)]
        # ms per batch of B images
        out["both_stacks_ms"] = timed(lambda: [st(p) for p in pa], 50)
        out["both_separate_ms"] = timed(lambda: [one(p, m) for p in pa for m in maps], 50)
        out["forward_pair_stacks_ms"] = timed(lambda: [(st(p, lr_only=True), st(q, p_lr=given)) for p, q in zip(pa, pb)], 50)
        out["forward_pair_separate_ms"] = timed(lambda: [(one(p, m), one_hr(q, m, r)) for p, q in zip(pa, pb) for m, r in zip(maps, rows)], 50)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["stacks", "single"])
    ap.add_argument("--shape", choices=["released", "s1"], default="released")
    ap.add_argument("--lib")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = [("stacks", s, None) for s in ("released", "s1")]
    for s in ("released", "s1"):
        if args.parent_lib:
            variants.append(("single", s, os.path.abspath(args.parent_lib)))
        variants.append(("single", s, None))
    results = []
    for r in range(args.rounds):
        for kind, shape, lib in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--shape", shape] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
            line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
            print(line, flush=True)
            results.append(json.loads(line))
    summary = {}
    for d in results:
        for k, v in d.items():
            if k.endswith("ms"):
                summary.setdefault("%s %s %s %s" % (d["child"], d["shape"], "tree" if d["lib"] == "tree" else "parent", k), []).append(v)
    summary = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), runs=v) for k, v in summary.items()}
    text = json.dumps(dict(rounds=args.rounds, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
