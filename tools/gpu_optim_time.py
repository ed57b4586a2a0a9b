"""Times optim.Optimizer.step() at the released options, all three parameter sets, against torch.optim of the same
kind on the same masters and the same stable .grad tensors.

  sides    ours         optim.Optimizer(net, kind): one surs_optim_step launch over the device table
           foreach      torch.optim.<kind>(params): torch's default multi-tensor path
           fused        torch.optim.<kind>(params, fused=True), where torch offers it (SGD, ADAM, AMSgrad)
  per child, three figures per call, in ms:
           host         wall time of the call itself on an idle device (a synchronise before every call, none inside the clock)
           device       device time: CALLS calls enqueued behind a blocker long enough to hide their host time, between two device
                        events, divided by CALLS - what the step costs a loop whose host runs ahead
           with_commit  ours: step() (the launch, then net.commit()); torch: step() + net.commit(); host clock around CALLS calls
                        and a closing synchronise, divided by CALLS, everything packed
  ADAM moves 28 bytes per parameter (p, g, m, v read; p, m, v written): `fraction_of_copy_rate` holds device time against the
  measured 6.3 TB/s copy rate.

Every measurement runs in a process of its own, ROUNDS times, the (kind, side) pairs alternating, each child under a time limit.  Prints
one JSON line per child and a summary (min / median / max over the rounds).

    python tools/gpu_optim_time.py [--rounds 5] [--out FILE] [--kinds ADAM ...] [--sides ours foreach fused]

--ranks R [R ...] times the data-parallel step instead: surs_optim_step_ranks (native.optim_step_ranks, called directly) over the same
masters with the gradient read from a synthetic gathered [R, total] slab, device time only, and bytes per second - (R + the kind's
state and parameter traffic) x 4 bytes per parameter - against the copy rate.  --parent-lib FILE adds a child that calls surs_optim_step
of THAT build of the library (the parent commit's) on the same table, alternating with the others: R = 1 through the new entry must
be no slower, within the spread the medians show.

    python tools/gpu_optim_time.py --ranks 1 2 8 [--parent-lib FILE] [--kinds ADAM] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COPY_RATE = 6.3e12
KINDS = ("SGD", "ADAM", "AMSgrad", "RMSprop")
SIDES = ("ours", "foreach", "fused")
FUSED = ("SGD", "ADAM", "AMSgrad")
BYTES_PER_PARAMETER = {"SGD": 20, "ADAM": 28, "AMSgrad": 36, "RMSprop": 20}     # (SGD with momentum: p, g, buf read; p, buf written)
CALLS = 10


def device_ms_of(step, host_ms, dev):
    """(median device time of one step(), the blocker's length), in ms: CALLS calls enqueued behind a blocker - passes over 1 GiB, as
    many as outlast the host time of CALLS calls three times over - between two device events, five times."""
    import torch
    sync = torch.cuda.synchronize
    flush = torch.zeros(1 << 30, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):      # (the first passes touch the pages for the first time: not the rate the blocker then runs at)
        flush.add_(1)
    e0.record()
    for _ in range(10):
        flush.add_(1)
    e1.record()
    sync()
    pass_ms = e0.elapsed_time(e1) / 10
    passes = int(3.0 * host_ms * CALLS / pass_ms) + 4
    device = []
    for _ in range(5):
        for _ in range(passes):
            flush.add_(1)
        e0.record()
        for _ in range(CALLS):
            step()
        e1.record()
        sync()
        device.append(e0.elapsed_time(e1) / CALLS)
    return sorted(device)[len(device) // 2], passes * pass_ms


def child_ranks(args):
    """One (kind, R) of the data-parallel step, or the parent library's plain step on the same table (--parent-lib)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import torch
    import common
    import gpu_common as g
    from surs_amd import model, native, optim
    dev = g.dev()
    net = model.SuRSNet(common.opt()).to(device=dev)
    net.load_state_dict(common.state_dict())
    kind, R = args.kind, args.child_ranks
    o = optim.Optimizer(net, kind, lr=1e-4)
    total = o._total
    gathered = torch.randn((R, total), generator=torch.Generator(device=dev).manual_seed(1), device=dev) * 1e-3
    names = o._state_names()
    rows = []
    for k in o._keys:
        st = [o._slice(n, k).data_ptr() for n in names] + [None] * (3 - len(names))
        rows.append((o._masters[k].data_ptr(), gathered.data_ptr() + 4 * o._offset[k], st[0], st[1], st[2], o._masters[k].numel()))
    items = native.optim_items(rows)
    hyper = native.optim_hyper(kind, 5, 1e-4, 0.0, 0.9)
    native.optim_check(items, len(rows), hyper)
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    if args.parent_lib:
        assert R == 1
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        parent.surs_optim_step.restype = C.c_int
        parent.surs_optim_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        stream = torch.cuda.current_stream().cuda_stream

        def step():
            assert parent.surs_optim_step(table.data_ptr(), len(rows), C.byref(hyper), stream) == 0
    else:
        scale = 1.0 if R == 1 else C.c_float(1.0 / R).value

        def step():
            native.optim_step_ranks(table, len(rows), hyper, R, total, scale)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(CALLS):
        step()
    host_ms = (time.perf_counter() - t) / CALLS * 1e3
    torch.cuda.synchronize()
    device_ms, _ = device_ms_of(step, host_ms, dev)
    n = sum(m.numel() for m in o._masters.values())
    nbytes = (BYTES_PER_PARAMETER[kind] - 4 + 4 * R) * n
    print(json.dumps(dict(child="parent" if args.parent_lib else "ranks", kind=kind, ranks=R, tensors=len(rows), parameters=n,
                          gradient_bytes=4 * total, device_ms=device_ms, bytes_per_s=nbytes / (device_ms * 1e-3),
                          fraction_of_copy_rate=nbytes / (device_ms * 1e-3) / COPY_RATE)), flush=True)


def main_ranks(args):
    results = []
    configs = [(R, None) for R in args.ranks]
    if args.parent_lib:
        configs.insert(0, (1, args.parent_lib))
    for r in range(args.rounds):
        for kind in args.kinds:
            for R, parent in configs:
                cmd = [sys.executable, os.path.abspath(__file__), "--child-ranks", str(R), "--kind", kind] + (["--parent-lib", parent] if parent else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # nothing more is started on the device after a failure
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
                line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
                print(line, flush=True)
                results.append(json.loads(line))
    by = {}
    for d in results:
        by.setdefault("%s %s R=%d" % (d["kind"], d["child"], d["ranks"]), []).append(d)
    summary = {}
    for name, v in by.items():
        ms = sorted(d["device_ms"] for d in v)
        summary[name] = dict(device_ms=dict(min=ms[0], median=ms[len(ms) // 2], max=ms[-1]),
                             bytes_per_s=sorted(d["bytes_per_s"] for d in v)[len(v) // 2],
                             fraction_of_copy_rate=sorted(d["fraction_of_copy_rate"] for d in v)[len(v) // 2],
                             parameters=v[0]["parameters"], gradient_bytes=v[0]["gradient_bytes"])
    text = json.dumps(dict(rounds=args.rounds, calls=CALLS, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import common
    import gpu_common as g
    from surs_amd import encoder, model, optim
    dev = g.dev()
    net = model.SuRSNet(common.opt()).to(device=dev)
    net.load_state_dict(common.state_dict())
    W = net._encoder_weights()          # everything packed, so that commit() has its whole work to do
    encoder._native_net(W)
    net._mlp_blob()
    params = []
    for w in net.SETS:
        params += list(getattr(net, w + "_parameters")().values())
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen, device=dev) * 1e-3
    kind, side = args.kind, args.child
    if side == "ours":
        o = optim.Optimizer(net, kind, lr=1e-4)
        step, step_commit = (lambda: o.step(commit=False)), o.step
    else:
        kw = dict(fused=True) if side == "fused" else {}
        if kind == "SGD":
            o = torch.optim.SGD(params, lr=1e-4, momentum=0.9, **kw)
        elif kind == "RMSprop":
            o = torch.optim.RMSprop(params, lr=1e-4, momentum=0, **kw)
        else:
            o = torch.optim.Adam(params, lr=1e-4, amsgrad=kind == "AMSgrad", **kw)
        step = o.step

        def step_commit():
            o.step()
            net.commit()
    sync = torch.cuda.synchronize
    for _ in range(3):
        step()
    sync()
    host = []
    for _ in range(CALLS):
        sync()
        t = time.perf_counter()
        step()
        host.append((time.perf_counter() - t) * 1e3)
    sync()
    host_ms = sorted(host)[len(host) // 2]
    device_ms, blocker_ms = device_ms_of(step, host_ms, dev)
    for _ in range(2):
        step_commit()
    sync()
    t = time.perf_counter()
    for _ in range(CALLS):
        step_commit()
    sync()
    with_commit_ms = (time.perf_counter() - t) / CALLS * 1e3
    n = sum(p.numel() for p in params)
    out = dict(child=side, kind=kind, tensors=len(params), parameters=n, host_ms=host_ms, device_ms=device_ms, with_commit_ms=with_commit_ms,
               blocker_ms=blocker_ms,
               fraction_of_copy_rate=BYTES_PER_PARAMETER[kind] * n / (device_ms * 1e-3) / COPY_RATE)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=SIDES)
    ap.add_argument("--kind", choices=KINDS, default="ADAM")
    ap.add_argument("--kinds", nargs="+", choices=KINDS, default=list(KINDS))
    ap.add_argument("--sides", nargs="+", choices=SIDES, default=list(SIDES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--ranks", nargs="+", type=int)
    ap.add_argument("--parent-lib")
    ap.add_argument("--child-ranks", type=int)
    args = ap.parse_args()
    if args.child_ranks:
        return child_ranks(args)
    if args.ranks:
        if args.kinds == list(KINDS):
            args.kinds = ["ADAM"]
        return main_ranks(args)
    if args.child:
        return child(args)
    results = []
    for r in range(args.rounds):
        for kind in args.kinds:
            for side in args.sides:
                if side == "fused" and kind not in FUSED:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--kind", kind]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # nothing more is started on the device after a failure
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
                line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
                print(line, flush=True)
                results.append(json.loads(line))
    by = {}
    for d in results:
        by.setdefault("%s %s" % (d["kind"], d["child"]), []).append(d)
    med = lambda v, k: sorted(d[k] for d in v)[len(v) // 2]
    summary = {}
    for name, v in by.items():
        summary[name] = {k: dict(min=min(d[k] for d in v), median=med(v, k), max=max(d[k] for d in v))
                         for k in ("host_ms", "device_ms", "with_commit_ms")}
        summary[name]["fraction_of_copy_rate"] = med(v, "fraction_of_copy_rate")
        summary[name]["parameters"], summary[name]["tensors"] = v[0]["parameters"], v[0]["tensors"]
    text = json.dumps(dict(rounds=args.rounds, calls=CALLS, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
