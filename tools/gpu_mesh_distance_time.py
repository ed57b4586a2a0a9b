"""Times the mesh distance at the paper's protocol: N = 10 000 surface samples against the procedural meshes
of tools/gpu_samples_time.py, 200 000 (HR) and 50 000 (LR) faces.

  distance   ms per native.mesh_distance call (with the faces) of the HR mesh's samples against the LR mesh and of the LR mesh's
             against the HR mesh, and ms per native.mesh_contains call on the SAME points and mesh - the yardstick: the same grid and
             staging, about as many instructions per pair; a distance call should cost at most twice the contains call.
             Point-triangle pairs per second of the two distance calls, and what that is of the fp32 vector peak (157.3 TFLOP/s,
             MI355X_MICROARCH.md) counting FLOP_PER_PAIR operations per pair: the formula's subtractions, products, sums and
             comparisons (a fused multiply-add counts two; the selects are not counted).
  metrics    ms of a whole metrics.mesh_metrics(HR, LR, n = N): both directions, the normals, the one read-back.

Every measurement runs in a process of its own, ROUNDS times, each child under a time limit; a host clock around work that ends in a
device synchronise, after warm-up calls of the same shapes.  Prints one JSON line per child and a summary with the medians.

    python tools/gpu_mesh_distance_time.py [--rounds 6] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = 10000
HR_GRID, LR_GRID = (400, 250), (250, 100)      # torus(nu, nv): 2 nu nv faces (tools/gpu_samples_time.py)
# 9 (ap, bp, cp) + 3 x 20 (an edge: the dot 5, s 1, the clamp 2, d 6, |d|^2 5, the minimum 1) + 15 (three plane dots) + 2 (the plane
# term) + 5 (inside) + 1 (the running minimum)
FLOP_PER_PAIR = 92
PEAK_FP32_VECTOR = 157.3e12


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import mesh_ref as mr
    from surs_amd import metrics, native
    native.require_gpu()
    hr, lr = native.Mesh(*mr.torus(*HR_GRID)), native.Mesh(*mr.torus(*LR_GRID))

    def timed(f, reps):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    on_hr, on_lr = metrics.surface_samples(hr, N, 1)[0], metrics.surface_samples(lr, N, 1)[0]
    ms = dict(distance_hr_to_lr=timed(lambda: native.mesh_distance(on_hr, lr, want_face=True), 20),
              distance_lr_to_hr=timed(lambda: native.mesh_distance(on_lr, hr, want_face=True), 20),
              contains_hr_to_lr=timed(lambda: native.mesh_contains(on_hr, lr), 20),
              contains_lr_to_hr=timed(lambda: native.mesh_contains(on_lr, hr), 20),
              metrics=timed(lambda: metrics.mesh_metrics(hr, lr, n=N), 10))
    rate = N * (hr.nf + lr.nf) / ((ms["distance_hr_to_lr"] + ms["distance_lr_to_hr"]) * 1e-3)
    print(json.dumps(dict(child="distance", ms=ms, faces=[hr.nf, lr.nf], n=N,
                          distance_over_contains=[ms["distance_hr_to_lr"] / ms["contains_hr_to_lr"],
                                                  ms["distance_lr_to_hr"] / ms["contains_lr_to_hr"]],
                          pairs_per_s=rate, fp32_vector_peak_share=rate * FLOP_PER_PAIR / PEAK_FP32_VECTOR,
                          scores=metrics.mesh_metrics(hr, lr, n=N))), flush=True)


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
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child()
    rows = [run([sys.executable, os.path.abspath(__file__), "--child"], 240) for _ in range(args.rounds)]
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {"ms " + k: dict(min=min(v), median=med(v), max=max(v)) for k in rows[0]["ms"] for v in [[r["ms"][k] for r in rows]]}
    for i, k in enumerate(("hr_to_lr", "lr_to_hr")):
        summary["distance / contains %s (medians)" % k] = summary["ms distance_" + k]["median"] / summary["ms contains_" + k]["median"]
    summary["pairs_per_s (median)"] = med([r["pairs_per_s"] for r in rows])
    summary["fp32_vector_peak_share (median)"] = med([r["fp32_vector_peak_share"] for r in rows])
    text = json.dumps(dict(rounds=args.rounds, n=N, faces=rows[0]["faces"], flop_per_pair=FLOP_PER_PAIR, scores=rows[0]["scores"],
                           summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
