"""Times the hourglass gradients at the released size: image_filter_lr.m0, --hg_depth 2, a 128 x 128 x 256 map.

  plain       encoder.hourglass() - the host mirror's launches, side streams as the inference forward uses them
  train       SuRSNet.hourglass_train(): one stream, every map kept, one surs_groupnorm_fold per norm site
  backward    SuRSNet.hourglass_backward() after one hourglass_train()
  autograd    torch autograd, fp32, on the same GPU: L.backward() (retain_graph) of <G, out> on this project's torch.nn.functional
              restatement of the module (tests/hg_grad_common.hourglass) - what a user would otherwise reach for
  gn          the GroupNorm + ReLU gradient alone on the 128 x 128 x 256 map: ms and the fraction of the 8 TB/s HBM peak, the bytes
              counted as two reads of g and of x and one write of dx
  bench       bench.py --gpus 1 on this tree;  bench_parent: on another build of the library (--parent-lib FILE: the parent commit's
              libsurs_hip.so) - only kernels were added, so the two must agree within the run-to-run spread

Every measurement runs in a process of its own, ROUNDS times (bench: 4), the variants alternating, each child under a time limit; a
host clock around work that ends in a device synchronise.  Prints one JSON line per child and a summary (min / median / max).

    python tools/gpu_hg_grad_time.py [--rounds 3] [--out FILE] [--parent-lib FILE] [--kinds plain train ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
H = 128
HBM_PEAK = 8.0e12


def _use_parent_lib(path):
    # an older build lacks the entries added since: the binding checks every declared symbol on load, so drop what is not there
    import ctypes
    import torch  # noqa: F401  (first: the library must bind to the HIP runtime torch carries - _lib.lib())
    from surs_amd import _lib
    _lib.LIB_PATH = os.path.abspath(path)
    old = ctypes.CDLL(_lib.LIB_PATH)
    for name in [k for k in _lib._SIGS if not hasattr(old, k)]:
        del _lib._SIGS[name]
    _lib.EXPORTS[:] = sorted(_lib._SIGS)


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.child in ("bench", "bench_parent"):
        if args.child == "bench_parent":
            _use_parent_lib(args.parent_lib)
        import runpy
        sys.argv = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", "1"]
        return runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
    import numpy as np
    import torch
    import common
    import gpu_common as g
    import hg_grad_common as hg
    from surs_amd import encoder, model, native, options, prng, weights
    from surs_amd.model import _as_img
    dev = g.dev()

    def timed(f, reps):
        for _ in range(2):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    out = dict(child=args.child)
    opt = options.BaseOptions().parse(common.FLAGS)
    sd = weights.synthetic_state_dict(opt, seed=0)
    x = torch.from_numpy(prng.uniform("t_hg_x", 1, (1, 256, H, H), -1.0, 1.0)).to(dev)
    if args.child == "gn":
        xi = g.upload_nhwc(prng.uniform("t_gn_x", 1, (256, H, H), -2.0, 2.0))
        gi = g.upload_nhwc(prng.uniform("t_gn_g", 2, (256, H, H), -1.0, 1.0))
        gamma, beta = (torch.from_numpy(np.array(sd[hg.P + "conv2.bn1." + k])).to(dev) for k in ("weight", "bias"))
        coeffs = native.groupnorm_fold(xi, gamma, beta)
        ws = torch.empty(native.lib().surs_groupnorm_relu_grad_workspace_bytes(H * H, 256), dtype=torch.uint8, device=dev)
        dx, dga, dbe = native.groupnorm_relu_grad(gi, xi, coeffs, gamma, workspace=ws)
        ms = timed(lambda: native.groupnorm_relu_grad(gi, xi, coeffs, gamma, dx=dx, dgamma=dga, dbeta=dbe, workspace=ws), 20)
        nbytes = 5.0 * H * H * 256 * 4
        out.update(ms=ms, gbytes_per_s=nbytes / (ms * 1e-3) / 1e9, of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK)
    elif args.child in ("plain", "train", "backward"):
        net = model.SuRSNet(opt).to(device=dev)
        net.load_state_dict(sd)
        if args.child == "plain":
            W, xi = net._encoder_weights(), _as_img(x)
            out["ms"] = timed(lambda: encoder.hourglass(W, hg.P + "m0.", opt.hg_depth, xi), 10)
        elif args.child == "train":
            out["ms"] = timed(lambda: net.hourglass_train(0, x), 10)
        else:
            y = net.hourglass_train(0, x)
            G = torch.rand_like(y) * 2 - 1
            out["ms"] = timed(lambda: net.hourglass_backward(0, G), 5)
            n = net._hg_native()
            out["tape_mb"] = native.hg_tape_bytes(n, H, H, True) / 2 ** 20
            out["workspace_mb"] = native.hg_backward_workspace_bytes(n, H, H, True) / 2 ** 20
    else:
        keys = [k for p in hg.hourglass_blocks(0, opt.hg_depth) for k in hg.block_keys(p)]
        P = {k: torch.from_numpy(np.array(sd[k])).to(dev).requires_grad_(True) for k in keys}
        xt = x.clone().requires_grad_()
        y = hg.hourglass(P, 0, opt.hg_depth, xt)
        G = torch.rand_like(y) * 2 - 1
        L = (G * y).sum()

        def f():
            xt.grad = None
            for p in P.values():
                p.grad = None
            L.backward(retain_graph=True)
        out["ms"] = timed(f, 5)
        out["forward_ms"] = timed(lambda: hg.hourglass(P, 0, opt.hg_depth, xt), 5)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["plain", "train", "backward", "autograd", "gn", "bench", "bench_parent"])
    ap.add_argument("--parent-lib", help="also run bench.py on this build of libsurs_hip.so")
    ap.add_argument("--kinds", nargs="+", help="the measurements to run (default: plain train backward autograd gn, + bench with --parent-lib)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="bench.py --steps")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    kinds = args.kinds or (["plain", "train", "backward", "autograd", "gn"] + (["bench", "bench_parent"] if args.parent_lib else []))
    if "bench_parent" in kinds and not args.parent_lib:
        raise SystemExit("bench_parent needs --parent-lib")
    results = []

    def run(kind):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(args.steps)]
        if kind == "bench_parent":
            cmd += ["--parent-lib", args.parent_lib]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
        d = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
        if kind.startswith("bench"):
            d = dict(child=kind, bench=d)
        print(json.dumps(d), flush=True)
        results.append(d)

    for r in range(args.rounds):
        for kind in [k for k in kinds if not k.startswith("bench")]:
            run(kind)
    for r in range(4 if any(k.startswith("bench") for k in kinds) else 0):
        for kind in [k for k in kinds if k.startswith("bench")]:
            run(kind)
    summary = {}
    for d in results:
        if "ms" in d:
            summary.setdefault(d["child"], []).append(d["ms"])
    summary = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), runs=v) for k, v in summary.items()}
    text = json.dumps(dict(rounds=args.rounds, summary=summary, all=results), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
