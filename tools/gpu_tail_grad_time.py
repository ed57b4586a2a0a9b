"""Times the stack-tail and whole-filter gradients at the released size: a 128 x 128 x 256 map, D = 256.

  joint        surs_tail_joint_grad alone (G_out, G_next -> dOut, dA in one launch): ms, and the bytes it has to move - four maps: two
               read, two written - per second as a fraction of the 8 TB/s HBM peak
  chain        the three-call chain of surs_conv_grad_input (k = 1) it replaces, the second and third adding into their target: ms,
               and ITS bytes - eight map passes: G_next twice, dOut read, written and read, dA written, read and written - likewise
  filter       SuRSNet.filter_lr_train() + filter_lr_backward() at the released options (every stack's G given)
  composition  the Python composition of a trainable filter_lr that INTEGRATION.md gave before these entries existed: autograd.conv_block
               / autograd.hourglass plus the stacks' 1 x 1 tails in torch.nn.functional; forward + L.backward()
  bench        bench.py --gpus 1 on this tree;  bench_parent: on another build of the library (--parent-lib FILE: the parent commit's
               libsurs_hip.so) - the inference path keeps its launches, so the two must agree within the run-to-run spread

Every measurement runs in a process of its own, ROUNDS times (bench: 4), the variants alternating, each child under a time limit; a
host clock around work that ends in a device synchronise.  Prints one JSON line per child and a summary (min / median / max).

    python tools/gpu_tail_grad_time.py [--rounds 3] [--out FILE] [--parent-lib FILE] [--kinds joint chain ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
H = 128
D = 256
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
    import torch
    import torch.nn.functional as F
    import common
    import gpu_common as g
    from surs_amd import autograd, model, native, options, prng, weights
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
    p = H * H
    if args.child in ("joint", "chain"):
        U = lambda tag, shape, a=1.0: torch.from_numpy(prng.uniform("t_tail_" + tag, 1, shape, -a, a)).to(dev)
        go, gn = native.Img(H, H, D, D, U("go", (p * D,))), native.Img(H, H, 256, 256, U("gn", (p * 256,)))
        w_al, w_l, w_bl = U("al", (256, D, 1, 1), 0.1), U("l", (D, 256, 1, 1), 0.1), U("bl", (256, 256, 1, 1), 0.1)
        d_out, d_a = native.Img(H, H, D, device=dev), native.Img(H, H, 256, device=dev)
        d_out.buf.zero_()
        if args.child == "joint":
            ms = timed(lambda: native.tail_joint_grad(go, gn, w_al, w_l, w_bl, d_out=d_out, d_a=d_a), 20)
            passes = 4
        else:
            def chain():   # (d_out keeps adding up: the timing does not care)
                native.conv_grad_input(gn, w_al, H, H, dx=d_out, add=True)
                native.conv_grad_input(d_out, w_l, H, H, dx=d_a)
                native.conv_grad_input(gn, w_bl, H, H, dx=d_a, add=True)
            ms = timed(chain, 20)
            passes = 8
        nbytes = passes * p * 256 * 4.0
        flop = 2.0 * p * (256 * D + D * 256 + 256 * 256)
        out.update(ms=ms, map_passes=passes, gbytes_per_s=nbytes / (ms * 1e-3) / 1e9, of_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK,
                   tflops=flop / (ms * 1e-3) / 1e12)
    else:
        opt = options.BaseOptions().parse(common.FLAGS)
        net = model.SuRSNet(opt).to(device=dev)
        net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
        S = opt.num_stack_lr
        x = torch.from_numpy(prng.uniform("t_tail_x", 1, (1, 256, H, H), -1.0, 1.0)).to(dev)
        G = [torch.from_numpy(prng.uniform("t_tail_G%d" % s, 2, (1, opt.hg_dim, H, H), -1.0, 1.0)).to(dev) for s in range(S)]
        out.update(stacks=S, depth=opt.hg_depth)
        if args.child == "filter":
            def f():
                net.filter_lr_train(x)
                net.filter_lr_backward(G)
            out["ms"] = timed(f, 3)
            out["train_ms"] = timed(lambda: net.filter_lr_train(x), 3)
            n = net._hg_native()
            out["tape_mb"] = native.filter_lr_tape_bytes(n, H, H) / 2 ** 20
            out["workspace_mb"] = native.filter_lr_backward_workspace_bytes(n, H, H) / 2 ** 20
        else:
            P, L = net.hg_parameters(), "image_filter_lr."
            conv1x1 = lambda k, t: F.conv2d(t, P[L + k + ".weight"], P[L + k + ".bias"])

            def filter_lr(feature_lr):
                previous, outs = autograd.conv_block(net, "conv2", feature_lr), []
                for s in range(S):
                    ll = autograd.conv_block(net, "top_m_%d" % s, autograd.hourglass(net, s, previous))
                    ll = F.relu(F.group_norm(conv1x1("conv_last%d" % s, ll), 32, P[L + "bn_end%d.weight" % s], P[L + "bn_end%d.bias" % s]))
                    outs.append(conv1x1("l%d" % s, ll))
                    if s < S - 1:
                        previous = previous + conv1x1("bl%d" % s, ll) + conv1x1("al%d" % s, outs[-1])
                return outs

            def f():
                xt = x.clone().requires_grad_()
                for v in P.values():
                    v.grad = None
                sum((gs * o).sum() for gs, o in zip(G, filter_lr(xt))).backward()
            out["ms"] = timed(f, 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["joint", "chain", "filter", "composition", "bench", "bench_parent"])
    ap.add_argument("--parent-lib", help="also run bench.py on this build of libsurs_hip.so")
    ap.add_argument("--kinds", nargs="+", help="the measurements to run (default: joint chain filter composition, + bench with --parent-lib)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="bench.py --steps")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    kinds = args.kinds or (["joint", "chain", "filter", "composition"] + (["bench", "bench_parent"] if args.parent_lib else []))
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
