"""Times one training step at the reference's default training options - --loadSize 512 (img_LR 256 x 256,
img_HR 512 x 512), --batch_size 2, --num_sample_inout 6000, ADAM - on seeded inputs and weights.

  children   full         forward_backward(encoder=True) + Optimizer.step(grads)
             full_guard   the same with step(grads, guard=True): the difference is the guard's launches and its one synchronisation
             autograd     the composition of surs_amd.autograd Functions it replaces (INTEGRATION.md "Training through autograd"):
                          super_res_features -> filter_lr -> point_loss + srweight l1_loss, loss.backward(), step() on the .grad
             loss_head    native.forward_losses_grad alone (device time between two events)
             loss_torch   forward_losses + the torch expression of the image term's gradient, alone
             bench / bench_parent   bench.py --gpus 1 on this tree / on another build of the library (--parent-lib FILE: the parent
                          commit's libsurs_hip.so), to show that the untouched paths stayed where they were
             optim / optim_parent   tools/gpu_optim_time.py's ADAM child (optim.Optimizer.step) on this tree / on that build
  per child  ms per step: host clock around STEPS steps and a closing synchronise, after WARMUP steps; peak_mib: torch's peak
             allocated device memory over the timed steps.

Every measurement runs in a process of its own, ROUNDS times, the children alternating, each under a time limit.  Prints one JSON
line per child and a summary (min / median / max over the rounds).

    python tools/gpu_train_step_time.py [--rounds 5] [--out FILE] [--parent-lib FILE] [--children full autograd ...]

--world N times the DATA-PARALLEL step instead (dist.TrainGroup; INTEGRATION.md "Data-parallel training"): N processes, rank r on GPU
r % device_count - RCCL when every rank has a GPU of its own, else gloo ranks sharing a GPU, which says nothing about xGMI and is
reported as such (`backend`) -, every rank at the options above on its own seeded batch.  Per rank: steps per second of
forward_backward + TrainGroup.step(guard=True) with the host running ahead, and, from a second loop with a synchronise on either side
of TrainGroup.step, the share of a step spent in pack + all-gather + fused step.  One JSON line (rank 0) per round with the slowest
rank's figures.

    python tools/gpu_train_step_time.py --world 8 [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHILDREN = ("full", "full_guard", "autograd", "loss_head", "loss_torch")
PARENT_CHILDREN = ("bench", "bench_parent", "optim", "optim_parent")
B, H, N = 2, 256, 6000
WARMUP, STEPS = 2, 5


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


def _training_inputs(opt, dev, seed=0):
    import numpy as np
    import torch
    import common
    from surs_amd import prng, weights
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    s = 100 * seed
    return dict(images_lr=up(np.concatenate([weights.synthetic_image(H, seed=s + 1 + b) for b in range(B)], 0)),
                images_hr=up(prng.uniform("img_hr", s + 7, (B, 3, 2 * H, 2 * H), -1.0, 1.0)),
                points_hr=up(np.stack([weights.synthetic_points(N, seed=s + 30 + b) for b in range(B)])),
                points_lr=up(np.stack([weights.synthetic_points(N, seed=s + 40 + b) for b in range(B)])),
                calibs=up(np.stack([common.CALIB] * B)),
                labels_hr=up(prng.uniform("lab_hr", s + 1, (B, 1, N), 0.0, 1.0) > 0.5),
                labels_lr=up(prng.uniform("lab_lr", s + 1, (B, 1, N), 0.0, 1.0) > 0.5))


def dp_worker(rank, world, port, backend):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import datetime
    import torch
    import torch.distributed as tdist
    from surs_amd import dist as sdist, model, optim, options, weights
    dev = torch.device("cuda:%d" % (rank % torch.cuda.device_count()))
    torch.cuda.set_device(dev)
    tdist.init_process_group(backend, init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                             timeout=datetime.timedelta(seconds=240))
    opt = options.BaseOptions().parse(["--residual", "--loadSize", "512", "--batch_size", str(B), "--num_sample_inout", str(N)])
    net = model.SuRSNet(opt).to(device=dev)
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.train()
    x = _training_inputs(opt, dev, seed=rank)
    o = optim.Optimizer(net, "ADAM", lr=1e-5)
    tg = sdist.TrainGroup(net, o)
    tg.broadcast_state(0)
    sync = torch.cuda.synchronize

    def grads():
        return net.forward_backward(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"], labels_lr=x["labels_lr"],
                                    labels_hr=x["labels_hr"], encoder=True)[3]
    for _ in range(WARMUP):
        tg.step(grads(), guard=True)
    sync()
    tdist.barrier()
    t = time.perf_counter()
    for _ in range(STEPS):
        tg.step(grads(), guard=True)
    sync()
    ms = (time.perf_counter() - t) / STEPS * 1e3
    exchange = 0.0
    t = time.perf_counter()
    for _ in range(STEPS):
        g = grads()
        sync()
        t0 = time.perf_counter()
        tg.step(g, guard=True)
        sync()
        exchange += time.perf_counter() - t0
    split_ms = (time.perf_counter() - t) / STEPS * 1e3
    tg.assert_replicas_equal()
    rows = sdist.all_gather_rows([ms, exchange / STEPS * 1e3, split_ms], dev)
    if rank == 0:
        slow = rows[rows[:, 0].argmax()]
        print(json.dumps(dict(child="dp", world=world, backend=backend, gpus=torch.cuda.device_count(), ms=float(slow[0]),
                              steps_per_s=1e3 / float(slow[0]), items_per_s=1e3 / float(slow[0]) * B * world,
                              exchange_ms=float(rows[:, 1].max()), exchange_share=float(rows[:, 1].max() / slow[2]),
                              gradient_bytes=4 * o._total, skipped=o.skipped)), flush=True)
    tdist.destroy_process_group()


def main_dp(args):
    """--world N: this process only starts the ranks (it never touches a GPU) and prints their lines."""
    import socket
    results = []
    for r in range(args.rounds):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-world", str(args.world), "--port", str(port)],
                           capture_output=True, text=True, timeout=900)
        if p.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("data-parallel child failed (%d)" % p.returncode)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    med = lambda k: sorted(d[k] for d in results)[len(results) // 2]
    text = json.dumps(dict(rounds=args.rounds, steps=STEPS, batch_per_rank=B, image=H, points=N, world=args.world, backend=results[0]["backend"],
                           gpus=results[0]["gpus"], gradient_bytes=results[0]["gradient_bytes"],
                           summary={k: dict(min=min(d[k] for d in results), median=med(k), max=max(d[k] for d in results))
                                    for k in ("ms", "steps_per_s", "items_per_s", "exchange_ms", "exchange_share")}), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def child_world(args):
    import torch
    import torch.multiprocessing as mp
    world = args.child_world
    backend = "nccl" if torch.cuda.device_count() >= world else "gloo"
    mp.spawn(dp_worker, args=(world, args.port, backend), nprocs=world, join=True)


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.child in PARENT_CHILDREN:
        if args.child.endswith("_parent"):
            _use_parent_lib(args.parent_lib)
        if args.child.startswith("bench"):
            import runpy
            sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
            return runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gpu_optim_time
        return gpu_optim_time.child(argparse.Namespace(kind="ADAM", child="ours"))
    import numpy as np
    import torch
    import common
    import gpu_common as g
    from surs_amd import autograd, model, native, optim, options, prng, weights
    dev = g.dev()
    opt = options.BaseOptions().parse(["--residual", "--loadSize", "512", "--batch_size", str(B), "--num_sample_inout", str(N)])
    net = model.SuRSNet(opt).to(device=dev)
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.train()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    x = dict(images_lr=up(np.concatenate([weights.synthetic_image(H, seed=1 + b) for b in range(B)], 0)),
             images_hr=up(prng.uniform("img_hr", 7, (B, 3, 2 * H, 2 * H), -1.0, 1.0)),
             points_hr=up(np.stack([weights.synthetic_points(N, seed=30 + b) for b in range(B)])),
             points_lr=up(np.stack([weights.synthetic_points(N, seed=40 + b) for b in range(B)])),
             calibs=up(np.stack([common.CALIB] * B)),
             labels_hr=up(prng.uniform("lab_hr", 1, (B, 1, N), 0.0, 1.0) > 0.5), labels_lr=up(prng.uniform("lab_lr", 1, (B, 1, N), 0.0, 1.0) > 0.5))
    sync = torch.cuda.synchronize
    name = args.child
    if name in ("full", "full_guard"):
        o = optim.Optimizer(net, "ADAM", lr=1e-5)

        def step():
            o.zero_grad()
            _, _, _, grads = net.forward_backward(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"],
                                                  labels_lr=x["labels_lr"], labels_hr=x["labels_hr"], encoder=True)
            o.step(grads, guard=name == "full_guard")
    elif name == "autograd":
        import torch.nn.functional as F
        o = optim.Optimizer(net, "ADAM", lr=1e-5)

        def step():
            o.zero_grad()
            img_SR, feature_lr, feat_hr = autograd.super_res_features(net, x["images_lr"])
            loss = autograd.point_loss(net, autograd.filter_lr(net, feature_lr), feat_hr, x["points_hr"], x["points_lr"], x["calibs"],
                                       x["labels_hr"], x["labels_lr"]) + net.opt.srweight * F.l1_loss(img_SR, x["images_hr"])
            loss.backward()
            for k, p in net.mlp_parameters().items():
                p.grad = net.last_classifier_grads[k].reshape(p.shape)
            o.step()
    else:
        S = opt.num_stack_lr
        gen = torch.Generator(device=dev).manual_seed(1)
        pl, ph = torch.rand((S, B * N), generator=gen, device=dev), torch.rand((S, B * N), generator=gen, device=dev)
        # (forward() holds the lr predictions against its labels_hr ARGUMENT and the hr ones against labels_lr: the reference's crossing)
        lab_for_lr, lab_for_hr = x["labels_hr"].reshape(-1), x["labels_lr"].reshape(-1)
        sr_nhwc = torch.randn((B, 2 * H, 2 * H, 3), generator=gen, device=dev)
        sr = sr_nhwc.permute(0, 3, 1, 2)
        w = (1.0, 1.0, 1.0, 1.0)
        if name == "loss_head":
            step = lambda: native.forward_losses_grad(pl, lab_for_lr, ph, lab_for_hr, sr_nhwc, x["images_hr"], w)
        else:
            def step():
                native.forward_losses(pred_lr=pl, lab_lr=lab_for_lr, pred_hr=ph, lab_hr=lab_for_hr, img_sr=sr.contiguous(), img_hr=x["images_hr"], weights=w)
                scale = torch.full((), 1.0, dtype=torch.float32, device=dev) / sr.numel()
                return torch.sign(sr - x["images_hr"]) * scale
    for _ in range(WARMUP):
        step()
    sync()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(STEPS):
        step()
    e1.record()
    sync()
    ms = (time.perf_counter() - t) / STEPS * 1e3
    out = dict(child=name, ms=ms, device_ms=e0.elapsed_time(e1) / STEPS, peak_mib=torch.cuda.max_memory_allocated() / 2.0 ** 20)
    if name == "full_guard":
        out["skipped"] = o.skipped
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=CHILDREN + PARENT_CHILDREN)
    ap.add_argument("--children", nargs="+", choices=CHILDREN + PARENT_CHILDREN,
                    help="default: %s, + %s with --parent-lib" % (" ".join(CHILDREN), " ".join(PARENT_CHILDREN)))
    ap.add_argument("--parent-lib", help="another build of libsurs_hip.so for bench_parent and optim_parent")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--world", type=int, help="time the data-parallel step on this many ranks instead")
    ap.add_argument("--child-world", type=int)
    ap.add_argument("--port", type=int)
    args = ap.parse_args()
    if args.child_world:
        return child_world(args)
    if args.world:
        return main_dp(args)
    if args.child:
        return child(args)
    children = args.children or list(CHILDREN + (PARENT_CHILDREN if args.parent_lib else ()))
    if any(c.endswith("_parent") for c in children) and not args.parent_lib:
        raise SystemExit("bench_parent and optim_parent need --parent-lib")
    results = []
    for r in range(args.rounds):
        for name in children:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name]
            if name.endswith("_parent"):
                cmd += ["--parent-lib", args.parent_lib]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
            d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            if name.startswith("bench"):       # bench.py's own result line: its headline value, whatever it is named
                d = dict(child=name, value=d.get("value", d.get("primary_value")), metric=d.get("metric", d.get("primary_metric")))
            d["child"] = name
            print(json.dumps(d), flush=True)
            results.append(d)
    by = {}
    for d in results:
        by.setdefault(d["child"], []).append(d)
    summary = {}
    for name, v in by.items():
        summary[name] = {k: dict(min=min(d[k] for d in v), median=sorted(d[k] for d in v)[len(v) // 2], max=max(d[k] for d in v))
                         for k in ("ms", "device_ms", "peak_mib", "value", "host_ms", "with_commit_ms") if isinstance(v[0].get(k), (int, float))}
    text = json.dumps(dict(rounds=args.rounds, steps=STEPS, batch=B, image=H, points=N, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
