"""Times SuRSNet.commit() at the released options against the route it replaces and against the gradient call
an optimiser step follows.

  commit   (a) net.commit() of all three parameter sets - classifiers, super-resolution net + conv5, image_filter_lr - with everything
               packed and every master present: the conv1x1 merges, ONE surs_conv_repack over every convolution, the GroupNorm / bias
               copies, the four launches of surs_mlp_repack
  reload   (b) the route it replaces, to a device synchronisation: .detach().cpu() of all three parameter dicts, load_state_dict,
               _encoder_weights() with its NativeNet, _mlp_blob(), _mlp_params(), sr_parameters(), hg_parameters()
  grads    (c) the gradient call of tools/gpu_grad_time.py (its `grads` child, released shape), in the same session
  repack       surs_conv_repack of the whole encoder's table alone: ms, bytes read + written, and bytes per second against the HBM
               peak of 8 TB/s - back to back (sources and images, 195 MB, stay in the 256 MiB Infinity Cache) and cache-cold (1 GiB
               of other traffic between two repacks, each between device events of its own)

Every measurement runs in a process of its own, ROUNDS times, the kinds alternating, each child under a time limit; a host clock
around work that ends in a device synchronise.  Prints one JSON line per child and a summary (min / median / max ms over the rounds).

    python tools/gpu_commit_time.py [--rounds 5] [--out FILE] [--kinds commit reload ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HBM_PEAK = 8e12
KINDS = ("commit", "reload", "grads", "repack")


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import common
    import gpu_common as g
    from surs_amd import encoder, model, native
    dev = g.dev()
    net = model.SuRSNet(common.opt()).to(device=dev)
    net.load_state_dict(common.state_dict())

    def pack_everything():
        W = net._encoder_weights()
        encoder._native_net(W)
        net._mlp_blob()
        net._mlp_params()
        return W, (net.mlp_parameters(), net.sr_parameters(), net.hg_parameters())

    def timed(f, reps, warm):
        for _ in range(warm):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    W, sets = pack_everything()
    out = dict(child=args.child, parameters=sum(p.numel() for s in sets for p in s.values()))
    if args.child == "commit":
        out["ms"] = timed(net.commit, 50, 5)
    elif args.child == "reload":
        sd = net.state_dict()

        def f():
            params = pack_everything()[1]
            sd.update({k: p.detach().cpu().reshape(sd[k].shape) for s in params for k, p in s.items()})
            net.load_state_dict(sd)
            pack_everything()
            torch.cuda.synchronize()
        out["ms"] = timed(f, 3, 1)
    else:
        tensors = dict(sets[1])
        tensors.update(sets[2])
        W.refresh(tensors)
        table = next(iter(W._refresh.values()))[0]
        nbytes = 0
        for it_w, cout, cin, k, packed, x2, x3 in [(cw._master, cw.cout, cw.cin, cw.k, cw.w, cw.w3 if cw.parts == 2 else None,
                                                    cw.w3 if cw.parts == 3 else None) for cw in W.conv.values() if cw._master is not None]:
            nbytes += it_w.numel() * 4 + sum(t.numel() * t.element_size() for t in (packed, x2, x3) if t is not None)
        out["ms"] = timed(lambda: native.conv_repack(table), 200, 10)
        # cache-cold: 1 GiB of other traffic (512 MiB read and written) between two repacks - more than the 256 MiB Infinity Cache
        # holds -, each repack between device events of its own
        flush = torch.zeros(512 << 20, dtype=torch.uint8, device=dev)
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(25)]
        for e0, e1 in events:
            flush.add_(1)
            e0.record()
            native.conv_repack(table)
            e1.record()
        torch.cuda.synchronize()
        cold = sorted(e0.elapsed_time(e1) for e0, e1 in events[5:])
        out.update(items=table.n, tiles=table.tiles, mbytes=nbytes / 1e6, fraction_of_hbm_peak=nbytes / (out["ms"] * 1e-3) / HBM_PEAK,
                   ms_cold=cold[len(cold) // 2], ms_cold_min=cold[0], ms_cold_max=cold[-1],
                   fraction_of_hbm_peak_cold=nbytes / (cold[len(cold) // 2] * 1e-3) / HBM_PEAK)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=[k for k in KINDS if k != "grads"])
    ap.add_argument("--kinds", nargs="+", choices=KINDS, default=list(KINDS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for r in range(args.rounds):
        for kind in args.kinds:
            if kind == "grads":
                cmd = [sys.executable, os.path.join(ROOT, "tools", "gpu_grad_time.py"), "--child", "grads", "--shape", "released"]
            else:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", kind]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
            line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
            print(line, flush=True)
            results.append(json.loads(line))
    by_kind = {}
    for d in results:
        by_kind.setdefault(d["child"], []).append(d)
    summary = {k: dict(min=min(d["ms"] for d in v), median=sorted(d["ms"] for d in v)[len(v) // 2], max=max(d["ms"] for d in v),
                       runs=[d["ms"] for d in v]) for k, v in by_kind.items()}
    if "repack" in by_kind:
        v = sorted(by_kind["repack"], key=lambda d: d["ms"])[len(by_kind["repack"]) // 2]
        summary["repack"].update(items=v["items"], tiles=v["tiles"], mbytes=v["mbytes"], fraction_of_hbm_peak=v["fraction_of_hbm_peak"])
        c = sorted(by_kind["repack"], key=lambda d: d["ms_cold"])[len(by_kind["repack"]) // 2]
        summary["repack cold"] = dict(median=c["ms_cold"], runs=[d["ms_cold"] for d in by_kind["repack"]],
                                      fraction_of_hbm_peak=c["fraction_of_hbm_peak_cold"])
    for a, b in (("commit", "reload"), ("commit", "grads")):
        if a in summary and b in summary:
            summary["%s / %s (medians)" % (a, b)] = summary[a]["median"] / summary[b]["median"]
    text = json.dumps(dict(rounds=args.rounds, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
