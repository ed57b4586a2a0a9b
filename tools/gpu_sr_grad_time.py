"""Times the super-resolution gradients at the released size: a 256 x 256 image, 512 x 512 enlarged, default
--n_block, with and without --residual.

  plain       super_res() + filter_hr(feature_hr): what the tape forward is held against
  train       super_res_train(): the same kernels with one buffer per layer; train - plain is the cost of the tape
  backward    super_res_backward() with all three upstream gradients, after one super_res_train()
  autograd    torch autograd, fp32, on the same GPU: loss.backward() (retain_graph) of <G, outputs> on this tool's own
              torch.nn.functional restatement of the network (tests/sr_grad_common.forward) - what a user would otherwise reach for
  layers      the weight-gradient kernel alone on bott2 (512 -> 512 at 64 x 64), ups4 (64 -> 64 at 512 x 512) and head (3 -> 32 at
              512 x 512): ms, TFLOP/s and the fraction of the 157 TFLOP/s fp32 matrix peak, next to torch.nn.grad.conv2d_weight
  bench       bench.py --gpus 1 on this tree;  bench_parent: on another build of the library (--parent-lib FILE: the parent commit's
              libsurs_hip.so) - no forward kernel changed, so the two must agree within the run-to-run spread

Every measurement runs in a process of its own, ROUNDS times (bench: 4), the variants alternating, each child under a time limit; a
host clock around work that ends in a device synchronise.  Prints one JSON line per child and a summary (min / median / max).

    python tools/gpu_sr_grad_time.py [--rounds 3] [--out FILE] [--parent-lib FILE] [--kinds plain train ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
H = 256
LAYERS = [("bott2", 512, 512, 64), ("ups4", 64, 64, 512), ("head", 3, 32, 512)]
PEAK_TFLOPS = 157.0


def _use_parent_lib(path):
    # an older build lacks the entries added since: the binding checks every declared symbol on load, so drop what is not there
    import ctypes
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
    from surs_amd import model, native, options, prng, weights
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

    out = dict(child=args.child, residual=args.residual)
    if args.child == "layers":
        rows = []
        for name, cin, cout, size in LAYERS:
            x = g.upload_nhwc(prng.uniform("t_x", 1, (cin, size, size), -1.0, 1.0))
            gz = g.upload_nhwc(prng.uniform("t_g", 2, (cout, size, size), -1.0, 1.0))
            ws = torch.empty(native.conv_grad_weight_workspace_bytes(size, size, cin, cout, 3) // 4, dtype=torch.float32, device=dev)
            dw, db = native.conv_grad_weight(gz, x, 3, 1, workspace=ws)
            ms = timed(lambda: native.conv_grad_weight(gz, x, 3, 1, dw=dw, db=db, workspace=ws), 10)
            xt = x.buf.view(1, size, size, cin).permute(0, 3, 1, 2)
            gt = gz.buf.view(1, size, size, cout).permute(0, 3, 1, 2)
            ms_t = timed(lambda: torch.nn.grad.conv2d_weight(xt, (cout, cin, 3, 3), gt, padding=1), 10)
            tf = 2.0 * cout * 9 * cin * size * size / (ms * 1e-3) / 1e12
            rows.append(dict(layer=name, ms=ms, tflops=tf, of_peak=tf / PEAK_TFLOPS, torch_ms=ms_t))
        out["layers"] = rows
        print(json.dumps(out), flush=True)
        return
    flags = [f for f in common.FLAGS if f != "--residual"] + (["--residual"] if args.residual else [])
    opt = options.BaseOptions().parse(flags)
    sd = weights.synthetic_state_dict(opt, seed=0)
    img = torch.from_numpy(weights.synthetic_image(H, seed=1)).to(dev)
    if args.child in ("plain", "train", "backward"):
        net = model.SuRSNet(opt).to(device=dev)
        net.load_state_dict(sd)
        if args.child == "plain":
            def f():
                _, _, f_hr = net.super_res(img)
                net.filter_hr(f_hr)
            out["ms"] = timed(f, 10)
        elif args.child == "train":
            out["ms"] = timed(lambda: net.super_res_train(img), 10)
        else:
            i, l, _ = net.super_res_train(img)
            G = [torch.rand_like(t) * 2 - 1 for t in (i, l, net.im_feat_list_hr[0])]
            out["ms"] = timed(lambda: net.super_res_backward(*G), 5)
            n = net._sr_native()[0]
            out["tape_mb"] = native.sr_tape_bytes(n, H, H) / 2 ** 20
            out["workspace_mb"] = native.sr_backward_workspace_bytes(n, H, H) / 2 ** 20
    else:
        import sr_grad_common as sg
        keys = native.sr_param_keys(sd, opt.n_block)
        P = {k: torch.from_numpy(np.array(sd[k])).to(dev).requires_grad_(True) for k in keys}
        outs = sg.forward(P, img, opt)
        outs = (outs[0], outs[1], outs[3])
        G = [torch.rand_like(t) * 2 - 1 for t in outs]
        L = sum((a * b).sum() for a, b in zip(G, outs))

        def f():
            for p in P.values():
                p.grad = None
            L.backward(retain_graph=True)
        out["ms"] = timed(f, 5)
        out["forward_ms"] = timed(lambda: sg.forward(P, img, opt), 5)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["plain", "train", "backward", "autograd", "layers", "bench", "bench_parent"])
    ap.add_argument("--residual", type=int, default=1)
    ap.add_argument("--parent-lib", help="also run bench.py on this build of libsurs_hip.so")
    ap.add_argument("--kinds", nargs="+", help="the measurements to run (default: plain train backward autograd layers, + bench with --parent-lib)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="bench.py --steps")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    kinds = args.kinds or (["plain", "train", "backward", "autograd", "layers"] + (["bench", "bench_parent"] if args.parent_lib else []))
    if "bench_parent" in kinds and not args.parent_lib:
        raise SystemExit("bench_parent needs --parent-lib")
    results = []

    def run(kind, residual):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--residual", str(residual), "--steps", str(args.steps)]
        if kind == "bench_parent":
            cmd += ["--parent-lib", args.parent_lib]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
        d = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
        if kind.startswith("bench"):
            d = dict(child=kind, residual=1, bench=d)
        print(json.dumps(d), flush=True)
        results.append(d)

    for r in range(args.rounds):
        for kind in [k for k in kinds if not k.startswith("bench")]:
            for residual in ((1,) if kind == "layers" else (1, 0)):
                run(kind, residual)
    for r in range(4 if any(k.startswith("bench") for k in kinds) else 0):
        for kind in [k for k in kinds if k.startswith("bench")]:
            run(kind, 1)
    summary = {}
    for d in results:
        if "ms" in d:
            summary.setdefault("%s residual=%d" % (d["child"], d["residual"]), []).append(d["ms"])
    summary = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v), runs=v) for k, v in summary.items()}
    text = json.dumps(dict(rounds=args.rounds, summary=summary, all=results), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
