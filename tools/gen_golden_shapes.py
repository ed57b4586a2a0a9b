"""Golden vectors for SurfaceClassifier shapes other than the released one, from the upstream reference itself on CPU
(tools/ref_harness.py, weights.synthetic_state_dict for each shape's flags).

    python tools/gen_golden_shapes.py [query] [recon] [views]

query -> tests/golden/query_shapes.npz: one set of 7168 points (uniform in the box, on the image border, outside the image) and,
         per shape, pred_hr / pred_lr and the last convolution's logits (forward hooks); one query_sr-on-other-points case (B = 2).
recon -> tests/golden/recon_shapes_r32.npz: the reference's dense (eval_grid) and octree (eval_grid_octree, init_resolution 8)
         occupancy fields at R = 32 for shape s1, encoder on weights.synthetic_image(64, seed=1).
views -> tests/golden/query_shapes_views.npz, query_shapes_views4.npz, recon_shapes_views_r32.npz: the same shapes (and l2) with
         --num_views 2 (4 for s1 and deep), per-view features and calibrations (gen_views).
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from gen_golden import CALIB, FLAGS, GOLD, synth_features  # noqa: E402
from surs_amd import options, prng, weights  # noqa: E402


def _dims(tag, dims):
    return ["--mlp_dim_" + tag] + [str(d) for d in dims]


def _res(tag, res):
    return ["--mlp_res_layers_" + tag] + [str(r) for r in res]


S1 = _dims("lr", [321, 512, 256, 128, 1]) + _dims("hr", [322, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _res("hr", [1, 2, 3])
SHAPES = {
    "s1": S1,
    "nores": ["--no_residual"],
    "deep": _dims("lr", [321, 1024, 1024, 512, 256, 128, 1]) + _dims("hr", [322, 1024, 1024, 512, 256, 128, 1])
    + _res("lr", [2, 3, 4, 5]) + _res("hr", [2, 3, 4, 5]),
    "odd": _dims("lr", [321, 1000, 500, 250, 100, 1]) + _dims("hr", [322, 1000, 500, 250, 100, 1]),
    "res0": _res("lr", [0, 2]) + _res("hr", [0, 2]),
    "l1": _dims("lr", [321, 1]) + _dims("hr", [322, 1]) + ["--no_residual"],
    "mixed": _dims("lr", [321, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _dims("hr", [322, 1000, 500, 250, 100, 1]),
}


def make_net(extra, seed=0):
    net = rh.build_net(rh.parse_opt(FLAGS + extra))
    sd = weights.synthetic_state_dict(options.BaseOptions().parse(FLAGS + extra), seed=seed)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return net


def shape_points():
    """[3, 7168] float32: 4608 uniform in [-0.55, 0.55]^3, 1280 within 1e-3 of the image border (x or y = +-0.5 under CALIB),
    1280 outside the image (|x| or |y| in [0.5, 0.6])."""
    a = weights.synthetic_points(4608, seed=21)
    u = prng.uniform("shape_points_border", 22, (3, 1280), -0.5, 0.5)
    side = np.where(prng.uniform("shape_points_side", 22, (1280,), 0.0, 1.0) < 0.5, -0.5, 0.5).astype(np.float32)
    jit = prng.uniform("shape_points_jitter", 22, (1280,), -1e-3, 1e-3)
    b = u.copy()
    b[0, :640] = side[:640] + jit[:640]
    b[1, 640:] = side[640:] + jit[640:]
    o = prng.uniform("shape_points_out", 23, (3, 1280), -0.5, 0.5)
    mag = prng.uniform("shape_points_outmag", 23, (1280,), 0.5, 0.6)
    o[0, :640] = np.where(o[0, :640] < 0, -mag[:640], mag[:640])
    o[1, 640:] = np.where(o[1, 640:] < 0, -mag[640:], mag[640:])
    return np.ascontiguousarray(np.concatenate([a, b, o], 1), np.float32)


def run_query(net, pts, calib):
    cap = {}
    hooks = [getattr(net, m)._modules["conv%d" % (len(getattr(net, m).filters) - 1)].register_forward_hook(
        lambda mod, i, o, key=m: cap.__setitem__(key, o.detach().clone())) for m in ("mlp_lr", "mlp_hr")]
    with torch.no_grad(), rh.quiet():
        p, c = torch.from_numpy(pts[None].copy()), torch.from_numpy(calib[None].copy())
        net.query_mr(p, c)
        net.query_sr(p, c)
        phr, plr = net.get_preds()
    for h in hooks:
        h.remove()
    return phr[0, 0].numpy(), plr[0, 0].numpy(), cap["mlp_hr"][0, 0].numpy(), cap["mlp_lr"][0, 0].numpy()


def gen_query():
    fl, fh = synth_features()
    pts = shape_points()
    out = {"points": pts}
    for name, extra in SHAPES.items():
        net = make_net(extra)
        net.im_feat_list_lr = [torch.from_numpy(fl[None].copy())]
        net.im_feat_list_hr = [torch.from_numpy(fh[None].copy())]
        phr, plr, lhr, llr = run_query(net, pts, CALIB)
        out.update({name + "_pred_hr": phr, name + "_logit_hr": lhr})
        if name != "mixed":   # (mixed's lr classifier is s1's, same weights: the same lr outputs)
            out.update({name + "_pred_lr": plr, name + "_logit_lr": llr})
        inside = plr[plr > 0]
        print("%-6s pred_lr in-image range %.3f..%.3f, median %.3f; zeros %.3f" % (name, inside.min(), inside.max(), np.median(inside),
                                                                                   float((phr == 0).mean())))
    # query_sr on other points than query_mr's, two subjects (as gen_golden.gen_query_sr, shape s1)
    net = make_net(S1)
    fa, fb = synth_features(seed=3), synth_features(seed=4)
    net.im_feat_list_lr = [torch.from_numpy(np.stack([fa[0], fb[0]]))]
    net.im_feat_list_hr = [torch.from_numpy(np.stack([fa[1], fb[1]]))]
    calib_b = np.array([[1.7, 0.3, -0.2, 0.05], [0.25, -1.8, 0.15, -0.04], [0.1, 0.2, 1.9, 0.02], [0, 0, 0, 1]], np.float32)
    n = 4099
    pts_mr = np.stack([weights.synthetic_points(n, seed=11), weights.synthetic_points(n, seed=12)])
    pts_sr = np.stack([weights.synthetic_points(n, seed=13), weights.synthetic_points(n, seed=14)])
    cal_mr, cal_sr = np.stack([CALIB, calib_b]), np.stack([calib_b, CALIB])
    with torch.no_grad(), rh.quiet():
        net.query_mr(torch.from_numpy(pts_mr.copy()), torch.from_numpy(cal_mr.copy()))
        net.query_sr(torch.from_numpy(pts_sr.copy()), torch.from_numpy(cal_sr.copy()))
        phr, plr = net.get_preds()
    out.update(sr_cal_mr=cal_mr, sr_cal_sr=cal_sr, sr_pred_hr=phr[:, 0].numpy(), sr_pred_lr=plr[:, 0].numpy())
    np.savez_compressed(os.path.join(GOLD, "query_shapes.npz"), **out)
    print("query_shapes.npz: %d bytes" % os.path.getsize(os.path.join(GOLD, "query_shapes.npz")))


def gen_recon():
    ns = rh.load_reference()
    net = make_net(S1)
    opt_ref = rh.parse_opt(FLAGS + S1)
    img = weights.synthetic_image(64, seed=1)
    with torch.no_grad(), rh.quiet():
        _, f_lr, f_hr = net.super_res(torch.from_numpy(img.copy()))
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
    calib = torch.from_numpy(CALIB[None].copy())
    R = 32
    coords, mat = ns.sdf.create_grid(R, R, R, np.array([-0.5] * 3), np.array([0.5] * 3))

    def eval_func(points):   # lib/mesh_util.py:20-28
        points = np.expand_dims(points, axis=0)
        samples = torch.from_numpy(points).float()
        net.query_mr(samples, calib)
        net.query_sr(samples, calib)
        phr, plr = net.get_preds()
        return phr[0][0].detach().numpy(), plr[0][0].detach().numpy()

    with torch.no_grad(), rh.quiet():
        dh, dl = ns.sdf.eval_grid(coords, eval_func, num_samples=50000)
        oh, ol = ns.sdf.eval_grid_octree(types.SimpleNamespace(threshold=opt_ref.threshold), coords, eval_func, init_resolution=8,
                                         num_samples=50000)
    for k, v in (("dense hr", dh), ("dense lr", dl), ("octree hr", oh), ("octree lr", ol)):
        print("%-9s range %.3f..%.3f, mean %.3f, > 0.5: %.3f" % (k, v.min(), v.max(), v.mean(), float((v > 0.5).mean())))
    np.savez_compressed(os.path.join(GOLD, "recon_shapes_r32.npz"), dense_hr=dh.astype(np.float32), dense_lr=dl.astype(np.float32),
                        octree_hr=oh.astype(np.float32), octree_lr=ol.astype(np.float32), threshold=np.array(opt_ref.threshold),
                        init_resolution=np.array(8))
    print("recon_shapes_r32.npz: %d bytes" % os.path.getsize(os.path.join(GOLD, "recon_shapes_r32.npz")))


L2 = _dims("lr", [321, 64, 1]) + _dims("hr", [322, 64, 1]) + _res("lr", [1]) + _res("hr", [1])   # a skip at the merge layer, mean of the logits
VIEW_SHAPES = dict(SHAPES, l2=L2)
VIEW_COUNTS = {"s1": (2, 4), "deep": (2, 4)}   # every other shape: V = 2


def views_calibs(V):
    """[V,4,4] orthogonal calibrations rotated about y (as gen_golden.gen_views builds them): x' = 2 (cos a x + sin a z) moves
    points of shape_points() in and out of the views' images."""
    return np.stack([np.array([[2.0 * np.cos(a), 0, 2.0 * np.sin(a), 0.02 * v], [0, -2.0, 0, -0.01 * v],
                               [-2.0 * np.sin(a), 0, 2.0 * np.cos(a), 0], [0, 0, 0, 1]], np.float32)
                     for v, a in enumerate(np.linspace(0.0, 0.6, V))])


def views_features(V):
    """per-view feature maps: synth_features(seed=10 + v) stacked -> ([V,256,32,32], [V,64,128,128])"""
    f = [synth_features(seed=10 + v) for v in range(V)]
    return np.stack([a for a, _ in f]), np.stack([b for _, b in f])


def make_views_net(extra, V):
    net = rh.build_net(rh.parse_opt(FLAGS + extra + ["--num_views", str(V)]))
    sd = weights.synthetic_state_dict(options.BaseOptions().parse(FLAGS + extra), seed=0)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    fl, fh = views_features(V)
    net.im_feat_list_lr = [torch.from_numpy(fl)]
    net.im_feat_list_hr = [torch.from_numpy(fh)]
    return net


def gen_views():
    """views -> tests/golden/query_shapes_views.npz (V = 2, every shape), query_shapes_views4.npz (V = 4: s1, deep; the query_sr on
    other points case, s1, V = 2) and recon_shapes_views_r32.npz (dense and octree fields, s1, V = 2): the reference's own multi-view
    path (SurfaceClassifier.py:70-76, train_util.reshape_sample_tensor), per-view features synth_features(seed=10 + v), calibrations
    views_calibs(V).  pred_hr / pred_lr [V,N]; logits (the last convolution's single row per point) where the merge layer is not the
    last one."""
    ns = rh.load_reference()
    pts = shape_points()
    out2, out4 = {"points": pts}, {}
    for name, extra in VIEW_SHAPES.items():
        for V in VIEW_COUNTS.get(name, (2,)):
            net = make_views_net(extra, V)
            cap = {}
            hooks = [getattr(net, m)._modules["conv%d" % (len(getattr(net, m).filters) - 1)].register_forward_hook(
                lambda mod, i, o, key=m: cap.__setitem__(key, o.detach().clone())) for m in ("mlp_lr", "mlp_hr")]
            samples = ns.train_util.reshape_sample_tensor(torch.from_numpy(pts[None].copy()), V)
            c = torch.from_numpy(views_calibs(V))
            with torch.no_grad(), rh.quiet():
                net.query_mr(samples, c)
                net.query_sr(samples, c)
                phr, plr = net.get_preds()
            for h in hooks:
                h.remove()
            assert tuple(phr.shape) == (V, 1, pts.shape[1])
            out = out2 if V == 2 else out4
            key = "%s_v%d_" % (name, V)
            out.update({key + "pred_hr": phr[:, 0].numpy(), key + "pred_lr": plr[:, 0].numpy()})
            for m, tag in (("mlp_lr", "lr"), ("mlp_hr", "hr")):
                if cap[m].shape[0] == 1:   # (merge layer = last layer: the last convolution yields one row per view)
                    out[key + "logit_" + tag] = cap[m][0, 0].numpy()
            print("%-6s V=%d zeros per view %s" % (name, V, [round(float((phr[v] == 0).float().mean()), 3) for v in range(V)]))
    # query_sr on points other than query_mr's: s1, V = 2
    V, n = 2, 4099
    net = make_views_net(S1, V)
    c = torch.from_numpy(views_calibs(V))
    pts_mr = weights.synthetic_points(n, seed=11)
    pts_sr = weights.synthetic_points(n, seed=13)
    with torch.no_grad(), rh.quiet():
        net.query_mr(ns.train_util.reshape_sample_tensor(torch.from_numpy(pts_mr[None].copy()), V), c)
        net.query_sr(ns.train_util.reshape_sample_tensor(torch.from_numpy(pts_sr[None].copy()), V), c)
        phr, plr = net.get_preds()
    out4.update(sr_points_mr=pts_mr, sr_points_sr=pts_sr, sr_pred_hr=phr[:, 0].numpy(), sr_pred_lr=plr[:, 0].numpy())
    for fname, out in (("query_shapes_views.npz", out2), ("query_shapes_views4.npz", out4)):
        np.savez_compressed(os.path.join(GOLD, fname), **out)
        print("%s: %d bytes" % (fname, os.path.getsize(os.path.join(GOLD, fname))))
    # R = 32 dense and octree fields, s1, V = 2: eval_func's multi-view recipe (lib/mesh_util.py:20-28), view 0's predictions
    net = make_views_net(S1, V)
    opt_ref = rh.parse_opt(FLAGS + S1 + ["--num_views", str(V)])
    R = 32
    coords, mat = ns.sdf.create_grid(R, R, R, np.array([-0.5] * 3), np.array([0.5] * 3))

    def eval_func(points):
        samples = torch.from_numpy(np.repeat(np.expand_dims(points, axis=0), V, axis=0)).float()
        net.query_mr(samples, c)
        net.query_sr(samples, c)
        phr, plr = net.get_preds()
        return phr[0][0].detach().numpy(), plr[0][0].detach().numpy()

    with torch.no_grad(), rh.quiet():
        dh, dl = ns.sdf.eval_grid(coords, eval_func, num_samples=50000)
        oh, ol = ns.sdf.eval_grid_octree(types.SimpleNamespace(threshold=opt_ref.threshold), coords, eval_func, init_resolution=8,
                                         num_samples=50000)
    for k, v in (("dense hr", dh), ("dense lr", dl), ("octree hr", oh), ("octree lr", ol)):
        print("%-9s range %.3f..%.3f, mean %.3f, > 0.5: %.3f" % (k, v.min(), v.max(), v.mean(), float((v > 0.5).mean())))
    fname = "recon_shapes_views_r32.npz"
    np.savez_compressed(os.path.join(GOLD, fname), dense_hr=dh.astype(np.float32), dense_lr=dl.astype(np.float32),
                        octree_hr=oh.astype(np.float32), octree_lr=ol.astype(np.float32), threshold=np.array(opt_ref.threshold),
                        init_resolution=np.array(8))
    print("%s: %d bytes" % (fname, os.path.getsize(os.path.join(GOLD, fname))))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ["query", "recon"]:
        globals()["gen_" + w]()
