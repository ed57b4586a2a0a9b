"""Times the rendering of a scan's training views on the procedural meshes of tools/gpu_mesh_raster_time.py,
200 000 (HR) and 50 000 (LR) faces, stood upright (the ring in the x - y plane) and seen as render.view_param frames them.

  prt       ms of one native.mesh_prt call at n = 40 (1600 directions) per mesh, one per subject in practice.
            tests: the ray - triangle tests the kernel EXECUTED (surs_mesh_prt_counted: 64 x the triangles each wave looked at before
            its any-hit exit - lane slots, so the lanes of rays with n . d <= 0 or already hit, which ride along, are in it), per
            second of the plain call, and beside it the useful pairs before any exit (rays with n . d > 0 times faces).
            peak share: executed tests x FLOPS_PER_TEST over the fp32 vector peak (157.3 TFLOP/s, MI355X_MICROARCH.md); a test is
            prt_hit as written, 24 multiplications and 18 additions / subtractions, its selects and compares not counted.
  view      ms per shaded, resolved 512 x 512 view at ms = 2: raster at 1024 x 1024, surs_mesh_shade_prt with a 2048 x 2048 texture,
            surs_image_resolve; and the raster's share of it.
  subject   seconds for the 360 yaws of a subject through render.render_views (the images' copies to the host included, no files).

Every measurement runs in a process of its own, ROUNDS times, each child under a time limit; a host clock around work that ends in a
device synchronise, after a warm-up call of the same shapes.  Prints one JSON line per child and a summary with the medians.

    python tools/gpu_render_time.py [--rounds 6] [--n_prt 40] [--meshes hr,lr] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZE, MS, TEX = 512, 2, 2048
GRIDS = {"hr": (400, 250), "lr": (250, 100)}      # torus(nu, nv): 2 nu nv faces
FLOPS_PER_TEST = 42
PEAK_FP32 = 157.3e12


def child(which, key, n_prt):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import mesh_ref as mr
    from surs_amd import native, render
    native.require_gpu()
    nu, nv = GRIDS[key]
    v, f = mr.torus(nu, nv)
    v = np.ascontiguousarray(v[:, [0, 2, 1]] + np.array([0.0, 100.0, -100.0]))      # the ring upright, as a standing subject: the
    f = np.ascontiguousarray(f[:, ::-1])                                             # up axis is its largest extent (still outward)
    k = np.arange(len(v))
    uvs = np.stack([(k // nv + 0.5) / nu, (k % nv + 0.5) / nv], -1)
    tex = (np.random.RandomState(0).rand(TEX, TEX, 3) * 255).astype(np.uint8)
    sub = render.Subject((v, f, uvs, f.copy()), tex)
    dirs = render.prt_directions(n_prt, 0)
    offset = render.PRT_OFFSET * float(np.ptp(v, 0).max())
    out = dict(child=which, mesh=key, faces=len(f), verts=len(v), directions=len(dirs))

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    if which == "prt":
        native.mesh_prt(sub.mesh, sub.normals_dev, dirs[:64], offset)                    # warm-up: the code object, the allocator
        ms, _ = clock(lambda: native.mesh_prt(sub.mesh, sub.normals_dev, dirs, offset))
        _, (_, tests) = clock(lambda: native.mesh_prt(sub.mesh, sub.normals_dev, dirs, offset, want_tests=True))
        cast = int((sub.normals_dev @ torch.from_numpy(dirs).to(sub.normals_dev.device).T > 0).sum())
        out.update(ms=ms, tests_executed=tests, tests_before_exit=cast * len(f), tests_per_s=tests / (ms * 1e-3),
                   peak_share=tests * FLOPS_PER_TEST / (ms * 1e-3) / PEAK_FP32)
    else:
        prt = native.mesh_prt(sub.mesh, sub.normals_dev, dirs[:16], offset)              # any transfer vectors: the shading's cost is the same
        center, scale = render.subject_frame(v)
        yaws = list(range(360))
        params = [render.view_param(y, 0, SIZE, center, scale)[0] for y in yaws]
        lights = np.stack([render.sample_light(y) for y in yaws])
        tex_kw = dict(texture=sub.texture, faces_uv=sub.faces_uv, uvs=sub.uvs)
        calib = render.view_param(30, 0, SIZE, center, scale)[1]
        light = render.sh_rotate(lights[30], params[30]["R"].T)

        def raster():
            return native.mesh_raster(sub.mesh, calib, SIZE * MS, want_bary=True)

        def view():
            face, bary = raster()
            rgba = native.mesh_shade_prt(sub.mesh, calib, face, bary, light, prt=prt, **tex_kw)
            return native.image_resolve(rgba, MS)

        reps = 20
        for fn in (raster, view):
            fn()
        ms_raster = clock(lambda: [raster() for _ in range(reps)])[0] / reps
        ms_view = clock(lambda: [view() for _ in range(reps)])[0] / reps
        render.render_views(sub, None, prt, params[:4], lights[:4], SIZE, ms=MS)
        ms_subject, (_, masks) = clock(lambda: render.render_views(sub, None, prt, params, lights, SIZE, ms=MS))
        out.update(ms_view=ms_view, ms_raster=ms_raster, raster_share=ms_raster / ms_view, s_subject=ms_subject * 1e-3,
                   covered=float((masks > 0).mean()))
    print(json.dumps(out), flush=True)


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
    ap.add_argument("--child", choices=["prt", "view"])
    ap.add_argument("--mesh", default="hr")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--n_prt", type=int, default=40)
    ap.add_argument("--meshes", default="hr,lr")
    ap.add_argument("--only", choices=["prt", "view"], help="one of the two measurements")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.mesh, args.n_prt)
    med = lambda v: sorted(v)[len(v) // 2]
    summary = {}
    for which in ([args.only] if args.only else ["prt", "view"]):
        for key in args.meshes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--mesh", key, "--n_prt", str(args.n_prt)]
            rows = [run(cmd, 600) for _ in range(args.rounds)]
            row = {k: rows[0][k] for k in ("faces", "verts", "directions")}
            for k, x in rows[0].items():
                if isinstance(x, float) or k.startswith("tests"):
                    vals = [r[k] for r in rows]
                    row[k] = dict(min=min(vals), median=med(vals), max=max(vals))
            summary["%s %s" % (which, key)] = row
    text = json.dumps(dict(rounds=args.rounds, size=SIZE, ms_rate=MS, texture=TEX, n_prt=args.n_prt, flops_per_test=FLOPS_PER_TEST,
                           summary=summary), indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
