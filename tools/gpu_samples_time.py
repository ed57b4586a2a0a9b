"""Times one training item's samples at the reference's size: N = 6000 (--num_sample_inout), a pool of
4 N + N / 4 = 25 500 points, procedural meshes of 200 000 (HR) and 50 000 (LR) faces, sigma 5, the default box.

  samples   one item, stage by stage: pool (surs_mesh_sample_pool + the shuffle's sort and gather), contains HR, contains LR,
            select, and the whole item back to back; point-triangle pairs per second of the two contains calls, and what
            that is of the fp32 vector peak (157.3 TFLOP/s, MI355X_MICROARCH.md) counting FLOP_PER_PAIR operations per pair -
            the formula's subtractions, products, sums and square roots, the atan2 as ONE operation (its reciprocal, polynomial
            and selects, about 20 more instructions, are not counted): an arithmetic bound, the kernel reads its triangles from LDS.
  step      the gradient part of a forward_backward step, the S = 3, B = 2, N = 6000 call of tools/gpu_grad_time.py (its
            `grads` child, released shape); a step consumes B items.

Every measurement runs in a process of its own, ROUNDS times, the two kinds alternating, each child under a time limit; a host
clock around work that ends in a device synchronise, after warm-up calls of the same shapes.  Prints one JSON line per child
and a summary with the medians over the rounds.

    python tools/gpu_samples_time.py [--rounds 6] [--step-rounds 6] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N, SIGMA, B = 6000, 5.0, 2
HR_GRID, LR_GRID = (400, 250), (250, 100)      # torus(nu, nv): 2 nu nv faces
FLOP_PER_PAIR = 66      # 9 (a, b, c) + 18 (three lengths) + 14 (determinant) + 15 (three dots) + 8 (denominator) + atan2 + the sum
PEAK_FP32_VECTOR = 157.3e12


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import mesh_ref as mr
    from surs_amd import native
    native.require_gpu()
    hr, lr = native.Mesh(*mr.torus(*HR_GRID)), native.Mesh(*mr.torus(*LR_GRID))
    n_pool = 4 * N + N // 4

    def timed(f, reps):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    seeds = iter(range(1, 1 << 20))
    make_pool = lambda: native.mesh_sample_pool(hr, 4 * N, N // 4, SIGMA, mr.B_MIN, mr.B_MAX, next(seeds))[0]
    pool = make_pool()
    in_hr, in_lr = native.mesh_contains(pool, hr), native.mesh_contains(pool, lr)

    def item():
        p = make_pool()
        return native.sample_select(p, native.mesh_contains(p, hr), native.mesh_contains(p, lr), N)

    ms = dict(pool=timed(make_pool, 50), contains_hr=timed(lambda: native.mesh_contains(pool, hr), 20),
              contains_lr=timed(lambda: native.mesh_contains(pool, lr), 20),
              select=timed(lambda: native.sample_select(pool, in_hr, in_lr, N), 50), item=timed(item, 20),
              area_cdf_hr=timed(lambda: native.mesh_area_cdf(hr.verts, hr.faces), 10))
    pairs = n_pool * (hr.nf + lr.nf)
    rate = pairs / ((ms["contains_hr"] + ms["contains_lr"]) * 1e-3)
    print(json.dumps(dict(child="samples", ms=ms, faces=[hr.nf, lr.nf], pool=n_pool, inside=[int(in_hr.sum()), int(in_lr.sum())],
                          pairs_per_s=rate, fp32_vector_peak_share=rate * FLOP_PER_PAIR / PEAK_FP32_VECTOR)), flush=True)


def run(cmd, limit):
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:   # nothing more is started on the device after a failure
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
    line = [x for x in p.stdout.splitlines() if x.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--step-rounds", type=int, default=6, help="rounds that also time the forward_backward gradient call")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child()
    samples, steps = [], []
    for r in range(args.rounds):
        samples.append(run([sys.executable, os.path.abspath(__file__), "--child"], 240))
        if r < args.step_rounds:
            steps.append(run([sys.executable, os.path.join(ROOT, "tools", "gpu_grad_time.py"), "--child", "grads", "--shape", "released"],
                             420)["ms"])
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {"ms " + k: dict(min=min(v), median=med(v), max=max(v)) for k in samples[0]["ms"] for v in [[s["ms"][k] for s in samples]]}
    summary["pairs_per_s (median)"] = med([s["pairs_per_s"] for s in samples])
    summary["fp32_vector_peak_share (median)"] = med([s["fp32_vector_peak_share"] for s in samples])
    if steps:
        summary["ms step grads"] = dict(min=min(steps), median=med(steps), max=max(steps))
        summary["item / step (medians)"] = summary["ms item"]["median"] / med(steps)
        summary["%d items / step (medians)" % B] = B * summary["ms item"]["median"] / med(steps)
    text = json.dumps(dict(rounds=args.rounds, step_rounds=len(steps), N=N, faces=samples[0]["faces"], pool=samples[0]["pool"],
                           flop_per_pair=FLOP_PER_PAIR, summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
