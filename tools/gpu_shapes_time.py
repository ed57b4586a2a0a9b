"""Times the fused evaluator of classifiers of any supported shape (surs_query_points_generic / surs_query_grid_generic) against the
released shape's layer-kernel point path (surs_query_points), on full-size feature maps (256 x 256^2, 64 x 1024^2) and 50 000 random
points, plus reconstruction sweeps of shape s1 (512-256-128, skips 1 2 3).  One JSON line per measurement.

    python tools/gpu_shapes_time.py points            # default shape: layer kernels vs fused, fp32-grade and one product; s1 fused
    python tools/gpu_shapes_time.py recon R [octree]  # s1: dense (or octree) reconstruction() at R, encoder on a 64 x 64 image
    python tools/gpu_shapes_time.py once              # one 50 000-point fused call per shape (for rocprofv3 --kernel-trace)
    python tools/gpu_shapes_time.py views             # multi-view evaluator: s1 / deep at V = 2, 4; V = 1 against the single-view
    python tools/gpu_shapes_time.py views-recon R     # two views, s1: dense and octree reconstruction() at R
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import common  # noqa: E402
import gpu_common as g  # noqa: E402
from surs_amd import mesh_util, model, native, options, weights  # noqa: E402

S1 = ["--mlp_dim_lr", "321", "512", "256", "128", "1", "--mlp_dim_hr", "322", "512", "256", "128", "1", "--mlp_res_layers_lr", "1", "2",
      "3", "--mlp_res_layers_hr", "1", "2", "3"]


def _ms(f, reps):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _split(parts):
    native.check(native.lib().surs_set_operand_split_local(parts))


def points():
    fl, fh = common.synth_features(hl=256, hh=1024)
    Fl, Fh = g.upload_nhwc(fl), g.upload_nhwc(fh)
    ws = native.Workspace(g.dev())
    pts = torch.from_numpy(weights.synthetic_points(50000, seed=2)).to(g.dev())
    cal = common.CALIB.reshape(-1)[:12]
    sd = {k: v for k, v in common.state_dict().items() if k.startswith("mlp_")}
    gdef = native.pack_mlp_generic(sd, g.dev())
    opt1 = options.BaseOptions().parse(common.FLAGS + S1)
    sd1 = {k: v for k, v in weights.synthetic_state_dict(opt1, seed=0).items() if k.startswith("mlp_")}
    gs1 = native.pack_mlp_generic(sd1, g.dev())
    blob = g.blob("bf16")
    layer = lambda: native.query_points(pts, cal, 512, 200.0, Fl, Fh, blob, ws)
    fused = lambda gm: (lambda: native.query_points_generic(pts, cal, 512, 200.0, Fl, Fh, gm))
    for label, parts in (("fp32-grade (two f16 parts)", 0), ("one f16 product", 1)):
        # alternate the two paths three times (the spread of the same command on a shared host)
        for rep in range(3):
            _split(parts)
            try:
                rows = [("default", "layer kernels", _ms(layer, 20)), ("default", "fused", _ms(fused(gdef), 20)),
                        ("s1", "fused", _ms(fused(gs1), 20))]
            finally:
                _split(0)
            for shape, path, ms in rows:
                print(json.dumps({"what": "50k points", "shape": shape, "path": path, "arith": label, "rep": rep, "ms": round(ms, 4)}))
    for name, gm in (("default", gdef), ("s1", gs1)):
        tp, lds, off = gm.info()
        print(json.dumps({"what": "tile", "shape": name, "points_per_tile": tp, "lds_bytes": lds,
                          "blob_MB": round(gm.blob.numel() / 1e6, 2)}))


def once():
    fl, fh = common.synth_features(hl=256, hh=1024)
    Fl, Fh = g.upload_nhwc(fl), g.upload_nhwc(fh)
    pts = torch.from_numpy(weights.synthetic_points(50000, seed=2)).to(g.dev())
    opt1 = options.BaseOptions().parse(common.FLAGS + S1)
    sd1 = {k: v for k, v in weights.synthetic_state_dict(opt1, seed=0).items() if k.startswith("mlp_")}
    gs1 = native.pack_mlp_generic(sd1, g.dev())
    for _ in range(3):
        native.query_points_generic(pts, common.CALIB.reshape(-1)[:12], 512, 200.0, Fl, Fh, gs1)
    torch.cuda.synchronize()
    print("3 fused calls of 50 000 points done")


DEEP = ["--mlp_dim_lr", "321", "1024", "1024", "512", "256", "128", "1", "--mlp_dim_hr", "322", "1024", "1024", "512", "256", "128", "1",
        "--mlp_res_layers_lr", "2", "3", "4", "5", "--mlp_res_layers_hr", "2", "3", "4", "5"]


def views():
    """50 000 points through surs_query_points_generic_views (full-size feature maps per view, rotated calibrations) for s1 and deep at
    V = 2, 4, fp32-grade and one product; V = 1 through the views entry against surs_query_points_generic."""
    Vmax = 4
    feats = [common.synth_features(seed=10 + v, hl=256, hh=1024) for v in range(Vmax)]
    FL = torch.from_numpy(np.stack([f[0].transpose(1, 2, 0) for f in feats])).to(g.dev())
    FH = torch.from_numpy(np.stack([f[1].transpose(1, 2, 0) for f in feats])).to(g.dev())
    Fl, Fh = g.upload_nhwc(feats[0][0]), g.upload_nhwc(feats[0][1])
    cals = np.stack([np.array([[2.0 * np.cos(a), 0, 2.0 * np.sin(a), 0], [0, -2.0, 0, 0], [-2.0 * np.sin(a), 0, 2.0 * np.cos(a), 0]],
                              np.float32).reshape(-1) for a in np.linspace(0.0, 0.6, Vmax)])
    pts = torch.from_numpy(weights.synthetic_points(50000, seed=2)).to(g.dev())
    for name, flags in (("s1", S1), ("deep", DEEP)):
        opt = options.BaseOptions().parse(common.FLAGS + flags)
        sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
        gm = native.pack_mlp_generic(sd, g.dev())
        for label, parts in (("fp32-grade (two f16 parts)", 0), ("one f16 product", 1)):
            for rep in range(3):
                _split(parts)
                try:
                    rows = [("single-view entry", 1, _ms(lambda: native.query_points_generic(pts, cals[0], 512, 200.0, Fl, Fh, gm), 10))]
                    for V in (1, 2, 4):
                        P = pts[None].expand(V, 3, pts.shape[1]).contiguous()
                        c = torch.from_numpy(cals[:V].copy()).to(g.dev())
                        fl, fh = FL[:V].contiguous(), FH[:V].contiguous()
                        rows.append(("views entry", V, _ms(lambda: native.query_points_generic_views(P, c, 512, 200.0, fl, fh, gm), 10)))
                finally:
                    _split(0)
                for path, V, ms in rows:
                    print(json.dumps({"what": "50k points", "shape": name, "path": path, "V": V, "arith": label, "rep": rep,
                                      "ms": round(ms, 4)}))
        print(json.dumps({"what": "tile", "shape": name, "views_points_per_tile_lds": native.mlp_generic_views_info(gm.shapes, 2)}))


def views_recon(R):
    opt = options.BaseOptions().parse(common.FLAGS + S1 + ["--resolution", str(R), "--num_views", "2"])
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(options.BaseOptions().parse(common.FLAGS + S1), seed=0))
    net.eval()
    img = torch.from_numpy(np.concatenate([weights.smooth_image(64, seed=1), weights.smooth_image(64, seed=2)])).to(g.dev())
    calib = torch.from_numpy(common.CALIB[None]).to(g.dev())
    with torch.no_grad():
        _, f_lr, f_hr = net.super_res(img)
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
        bmin, bmax = np.array([-0.6] * 3), np.array([0.6] * 3)
        for octree in (False, True):
            times = []
            for _ in range(2):
                torch.cuda.synchronize()
                t = time.time()
                out = mesh_util.reconstruction(opt, net, g.dev(), calib, R, bmin, bmax, use_octree=octree, want_normals=False)
                torch.cuda.synchronize()
                times.append(time.time() - t)
            print(json.dumps({"what": "reconstruction", "shape": "s1", "views": 2, "R": R, "octree": octree,
                              "s": [round(x, 4) for x in times], "verts_hr": int(out[0].shape[0]), "verts_lr": int(out[4].shape[0])}))


def recon(R, octree):
    opt = options.BaseOptions().parse(common.FLAGS + S1 + ["--resolution", str(R)])
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.eval()
    img = torch.from_numpy(weights.smooth_image(64, seed=1)).to(g.dev())
    calib = torch.from_numpy(common.CALIB[None]).to(g.dev())
    with torch.no_grad():
        _, f_lr, f_hr = net.super_res(img)
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
        bmin, bmax = np.array([-0.6] * 3), np.array([0.6] * 3)   # (past the image: s1's synthetic field is > 0.5 inside it)
        out = None
        times = []
        for _ in range(2):
            torch.cuda.synchronize()
            t = time.time()
            out = mesh_util.reconstruction(opt, net, g.dev(), calib, R, bmin, bmax, use_octree=octree, want_normals=False)
            torch.cuda.synchronize()
            times.append(time.time() - t)
    print(json.dumps({"what": "reconstruction", "shape": "s1", "R": R, "octree": octree, "s": [round(x, 4) for x in times],
                      "verts_hr": int(out[0].shape[0]), "verts_lr": int(out[4].shape[0])}))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "points"
    if what == "points":
        points()
    elif what == "once":
        once()
    elif what == "views":
        views()
    elif what == "views-recon":
        views_recon(int(sys.argv[2]))
    else:
        recon(int(sys.argv[2]), len(sys.argv) > 3 and sys.argv[3] == "octree")
