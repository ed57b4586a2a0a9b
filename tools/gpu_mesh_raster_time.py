"""Times the mesh raster and the normal reprojection error at 512 x 512 on the procedural meshes of
tools/gpu_mesh_distance_time.py, 200 000 (HR) and 50 000 (LR) faces, and on one of 1 000 000 faces (the size of a 512^3
reconstruction), seen through a calib that holds the tests' box, tilted so that the torus shows its hole.

  raster        ms per native.mesh_raster call (face, depth and bary) per mesh.
                boxes: the bytes of pixel boxes the parts kernel reads per call - (tiles of 32 x 32) x faces x 16 - per second, and
                what that is of the HBM peak (8.0 TB/s, MI355X_MICROARCH.md; the boxes of a part fit in the caches, so this says how
                near the walk over the boxes is to a memory-bound one, not where the bytes come from).
                pairs: covered pixel-triangle pairs per second, the pairs taken as the sum of the faces' projected areas in pixels
                (float64; every face of these meshes is on the image, half of them hidden behind the others).
  normal_error  ms of a whole four-view metrics.normal_error(HR, LR) and (1M, HR): eight normal maps, the sums, the one read-back.
  metrics       the yardstick beside it: ms of metrics.mesh_metrics(HR, LR, n = 10 000) on the same pair of meshes.

Every measurement runs in a process of its own, ROUNDS times, each child under a time limit; a host clock around work that ends in a
device synchronise, after warm-up calls of the same shapes.  Prints one JSON line per child and a summary with the medians.

    python tools/gpu_mesh_raster_time.py [--rounds 6] [--part FACES] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZE = 512
N = 10000
GRIDS = {"hr": (400, 250), "lr": (250, 100), "big": (1000, 500)}      # torus(nu, nv): 2 nu nv faces
TILE = 32
PEAK_HBM = 8.0e12


def calib():
    import numpy as np
    s, t = 1.0 / 190.0, np.deg2rad(50.0)
    c = np.identity(4)
    c[:3, :3] = np.diag([s, -s, s]) @ np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])
    c[:3, 3] = -c[:3, :3] @ np.array([0.0, 100.0, 0.0])
    return c


def projected_area(mesh, view, size):
    """Sum over the faces of the projected area in pixels (float64)."""
    import numpy as np
    v = np.asarray(mesh[0], np.float64) @ view[:3, :3].T + view[:3, 3]
    s = (v[:, :2] + 1) * (0.5 * size)
    t = s[np.asarray(mesh[1])]
    d1, d2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return float(np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]).sum() * 0.5)


def child(part):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import mesh_ref as mr
    from surs_amd import _lib, metrics, native
    native.require_gpu()
    if part:
        native.set_option("raster_part", part)
    host = {k: mr.torus(*g) for k, g in GRIDS.items()}
    mesh = {k: native.Mesh(*m) for k, m in host.items()}
    view = calib()
    views = metrics.turntable_views(view, (0, 90, 180, 270), (0.0, 100.0, 0.0))

    def timed(f, reps):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / reps * 1e3

    ms, rates, covered = {}, {}, {}
    tiles = ((SIZE + TILE - 1) // TILE) ** 2
    for k, m in mesh.items():
        ms["raster_" + k] = timed(lambda: native.mesh_raster(m, view, SIZE, want_depth=True, want_bary=True), 20)
        sec = ms["raster_" + k] * 1e-3
        rates[k] = dict(box_bytes_per_s=tiles * m.nf * 16 / sec, pairs_per_s=projected_area(host[k], view, SIZE) / sec)
        rates[k]["hbm_peak_share"] = rates[k]["box_bytes_per_s"] / PEAK_HBM
        covered[k] = int((native.mesh_raster(m, view, SIZE) >= 0).sum())
    ms["normal_error_hr_lr"] = timed(lambda: metrics.normal_error(mesh["hr"], mesh["lr"], views, size=SIZE), 5)
    ms["normal_error_big_hr"] = timed(lambda: metrics.normal_error(mesh["big"], mesh["hr"], views, size=SIZE), 5)
    ms["metrics_hr_lr"] = timed(lambda: metrics.mesh_metrics(mesh["hr"], mesh["lr"], n=N), 10)
    lib = _lib.lib()
    print(json.dumps(dict(child="raster", ms=ms, rates=rates, covered_pixels=covered, faces={k: m.nf for k, m in mesh.items()},
                          raster_part=native.get_option("raster_part"),
                          workspace_mib={k: lib.surs_mesh_raster_workspace_bytes(SIZE, SIZE, m.nf) / 2.0 ** 20 for k, m in mesh.items()},
                          scores=metrics.normal_error(mesh["hr"], mesh["lr"], views, size=SIZE))), flush=True)


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
    ap.add_argument("--part", type=int, default=0, help="the option raster_part for this run (0: the library's default)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args.part)
    rows = [run([sys.executable, os.path.abspath(__file__), "--child", "--part", str(args.part)], 240) for _ in range(args.rounds)]
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {"ms " + k: dict(min=min(v), median=med(v), max=max(v)) for k in rows[0]["ms"] for v in [[r["ms"][k] for r in rows]]}
    for k in rows[0]["rates"]:
        for what in rows[0]["rates"][k]:
            summary["%s %s (median)" % (what, k)] = med([r["rates"][k][what] for r in rows])
    first = rows[0]
    text = json.dumps(dict(rounds=args.rounds, size=SIZE, faces=first["faces"], raster_part=first["raster_part"],
                           workspace_mib=first["workspace_mib"], covered_pixels=first["covered_pixels"], scores=first["scores"],
                           summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
