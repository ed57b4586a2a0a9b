"""Times the image half of a training item ("training images") at --loadSize 512: a 512 x 512 render and mask
on disk, --random_flip --random_scale --random_trans --aug_blur 2, one view.

  host      the parent path: TrainDataset(images=None).get_render - PIL from the decoded files through numpy's ToTensor / Normalize /
            mask - and the upload of img_LR and img_HR, ending in a device synchronise.  Colour jitter off: this path refuses it.
  device    TrainDataset(images="device").get_render on the same draws, jitter off: "host ms" is the host clock around the call with
            the device held busy by a blocker (a chain of large matrix products enqueued first), so it is what the calling thread
            pays; "device ms" is between two events on the stream behind the blocker, so the kernels and copies run back to back.
  device_jitter   the same with --aug_bri 0.2 --aug_con 0.3 --aug_sat 0.4 --aug_hue 0.1.
  decode    what both paths share: Image.open().convert() of the two files into numpy arrays.
  kernels   every stage's entry point alone, 50 calls behind a blocker between two events, with the bytes each must move (from the
            shapes) over that time, beside a device-to-device copy of the same bytes and one of 256 MiB.
  grad      the gradient call of tools/gpu_grad_time.py (child "grads", released shape) - what an item's image half is a share of.

Every measurement runs in a process of its own, ROUNDS times, the kinds alternating, each child under a time limit.  Prints one JSON
line per child and a summary (min / median / max over the rounds).

    python tools/gpu_train_images_time.py [--rounds 6] [--out FILE] [--kinds host device ...]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZE = 512
AUG = ["--random_flip", "--random_scale", "--random_trans", "--aug_blur", "2"]
JITTER = ["--aug_bri", "0.2", "--aug_con", "0.3", "--aug_sat", "0.4", "--aug_hue", "0.1"]
KINDS = ["host", "device", "device_jitter", "decode", "kernels", "grad"]


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import random
    import numpy as np
    import torch
    import mesh_ref as mr
    import train_data_common as tdc
    from surs_amd import _lib, data, native, prng
    dev = native.require_gpu()
    out = dict(child=args.child)
    big = torch.randn((8192, 8192), device=dev)

    def blocker(n=8):
        for _ in range(n):
            torch.mm(big, big)

    def seed(i):
        random.seed(i), np.random.seed(i), torch.manual_seed(i)

    if args.child in ("host", "device", "device_jitter", "decode"):
        root = tdc.make_dataroot(tempfile.mkdtemp(prefix="train_images_time_"), mr.torus(8, 6), mr.torus(6, 4), size=SIZE)
        more = AUG + (JITTER if args.child == "device_jitter" else [])
        ds = data.TrainDataset(tdc.opt(root, size=SIZE, more=more), "train", images=None if args.child in ("host", "decode") else "device")
        reps = 20
        if args.child == "decode":
            from PIL import Image
            t = time.perf_counter()
            for _ in range(reps):
                np.asarray(Image.open(os.path.join(root, "RENDER", "alpha", "0_0_00.png")).convert("RGB"), np.uint8)
                np.asarray(Image.open(os.path.join(root, "MASK", "alpha", "0_0_00.png")).convert("L"), np.uint8)
            out["ms"] = (time.perf_counter() - t) / reps * 1e3
        elif args.child == "host":
            def f(i):
                seed(i)
                r = ds.get_render("alpha", num_views=1)
                return r["img_LR"].to(dev), r["img_HR"].to(dev)
            for i in range(3):
                f(i)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(reps):
                f(i)
            torch.cuda.synchronize()
            out["ms"] = (time.perf_counter() - t) / reps * 1e3
        else:
            for i in range(3):
                seed(i)
                ds.get_render("alpha", num_views=1)
            torch.cuda.synchronize()
            host, devms, held = [], [], []
            for i in range(reps):
                seed(i)
                e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                e0.record()
                blocker()
                e1.record()
                t = time.perf_counter()
                ds.get_render("alpha", num_views=1)
                host.append((time.perf_counter() - t) * 1e3)
                e2.record()
                torch.cuda.synchronize()
                devms.append(e1.elapsed_time(e2))
                held.append(e0.elapsed_time(e1))
            out["ms"] = sorted(host)[reps // 2]
            out["device_ms"] = sorted(devms)[reps // 2]
            out["blocker_ms"] = sorted(held)[reps // 2]     # must exceed ms for device_ms to be free of launch gaps
        import shutil
        shutil.rmtree(root, ignore_errors=True)
    elif args.child == "kernels":
        L = native.lib()
        pad = int(0.1 * SIZE)
        full = int(1.07 * (SIZE + 2 * pad))
        x1 = int(round((full - SIZE) / 2.)) + 3
        plan = native.train_image_plan((SIZE, SIZE), pad=pad, flip=True, full=(full, full), window=(x1, x1, SIZE, SIZE),
                                       jitter=((3, 1, 0, 2), 1.1, 0.8, 1.3, 0.05), blur=1.5)
        p = plan.plan
        u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
        rgb = torch.from_numpy((prng.uniform01("time_rgb", 1, SIZE * SIZE * 3) * 256.0).astype(np.uint8).reshape(SIZE, SIZE, 3)).to(dev)
        mask = torch.full((SIZE, SIZE), 255, dtype=torch.uint8, device=dev)
        tables = torch.from_numpy(plan.tables).to(dev)
        nws = L.surs_train_images_workspace_bytes(p)
        ws, a, b, c, m = u8(nws), u8(SIZE, SIZE, 3), u8(SIZE, SIZE, 3), u8(SIZE, SIZE, 3), u8(SIZE, SIZE)
        hr, lr = torch.empty((SIZE, SIZE, 3), device=dev), torch.empty((SIZE // 2, SIZE // 2, 3), device=dev)
        ptr, st = native._ptr, native._stream
        px, src_px = SIZE * SIZE, SIZE * SIZE
        big_a, big_b = u8(1 << 28), u8(1 << 28)
        calls = {
            "geometry_rgb": (lambda: L.surs_image_resample(p.geo, ptr(tables), ptr(rgb), ptr(a), st()), 3 * src_px + 3 * px),
            "geometry_mask": (lambda: L.surs_image_nearest(p.geo, ptr(tables), ptr(mask), ptr(m), st()), 2 * px),
            "jitter_2_passes": (lambda: L.surs_image_jitter(p, ptr(a), SIZE, SIZE, ptr(ws), nws, ptr(b), st()), 4 * 3 * px),
            "blur_x_and_y": (lambda: L.surs_image_blur(p, ptr(b), SIZE, SIZE, ptr(c), ptr(a), st()), 4 * 3 * px),
            "prepare_hr": (lambda: L.surs_image_prepare(ptr(a), ptr(m), SIZE, SIZE, ptr(hr), 3, st()), 4 * px + 12 * px),
            "chain": (lambda: L.surs_train_images(p, ptr(tables), ptr(rgb), ptr(mask), ptr(ws), nws, ptr(hr), ptr(lr), st()), 0),
            "copy_same_bytes": (lambda: b.copy_(a), 2 * 3 * px),
            "copy_256MiB": (lambda: big_b.copy_(big_a), 2 << 28),
        }
        res = {}
        for name, (f, nbytes) in calls.items():
            reps = 50 if nbytes < (1 << 28) else 5
            for _ in range(3):
                r = f()
                if isinstance(r, int):
                    native.check(r)
            torch.cuda.synchronize()
            e1, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            blocker(4)
            e1.record()
            for _ in range(reps):
                f()
            e2.record()
            torch.cuda.synchronize()
            us = e1.elapsed_time(e2) / reps * 1e3
            res[name] = dict(us=us, bytes=nbytes, gb_per_s=nbytes / us / 1e3 if nbytes else None)
        out["kernels"] = res
        out["ms"] = res["chain"]["us"] / 1e3
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=KINDS)
    ap.add_argument("--kinds", nargs="+", default=KINDS)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    for r in range(args.rounds):
        for kind in args.kinds:
            if kind == "grad":
                cmd = [sys.executable, os.path.join(ROOT, "tools", "gpu_grad_time.py"), "--child", "grads", "--shape", "released"]
            else:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", kind]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
            if p.returncode != 0:   # nothing more is started on the device after a failure
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
            d = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
            d["child"] = kind
            print(json.dumps(d), flush=True)
            results.append(d)
    series = {}
    for d in results:
        series.setdefault(d["child"] + " ms", []).append(d["ms"])
        if "device_ms" in d:
            series.setdefault(d["child"] + " device ms", []).append(d["device_ms"])
            series.setdefault(d["child"] + " blocker ms", []).append(d["blocker_ms"])
        for k, v in d.get("kernels", {}).items():
            series.setdefault("kernel %s us" % k, []).append(v["us"])
            if v["gb_per_s"]:
                series.setdefault("kernel %s GB/s" % k, []).append(v["gb_per_s"])
    summary = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in series.items()}
    med = lambda k: summary[k]["median"] if k in summary else None
    if med("host ms") and med("device ms"):
        summary["device host ms / host ms (medians)"] = med("device ms") / med("host ms")
    if med("grad ms"):
        for k in ("host ms", "device ms", "device_jitter ms", "device device ms", "device_jitter device ms"):
            if med(k):
                summary["%s / grad ms (medians)" % k] = med(k) / med("grad ms")
    text = json.dumps(dict(rounds=args.rounds, size=SIZE, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
