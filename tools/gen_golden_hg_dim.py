"""Golden vectors for --hg_dim other than 256 (the channel count of the hourglass encoder's output, lib/model/SuRSNet.py:62-65,
lib/model/HGFilters.py:166-174), from the upstream reference itself on CPU (tools/ref_harness.py, weights.synthetic_state_dict for
each case's flags).  Build container only.

    python tools/gen_golden_hg_dim.py [keys] [query] [encoder] [recon]

keys    -> tests/golden/state_dict_keys_hg_dim.json: {case: [[key, shape], ...]} of the reference's state_dict().
query   -> tests/golden/query_hg_dim.npz: per case (and d128w, a 16-point-tile shape on D = 128) pred_hr / pred_lr and the last
           convolution's logits on shape_points(), lr features prng.uniform("feat_lr", 3, (D, 32, 32), -1, 1) and the usual
           64-channel hr features; d128 also with --num_views 2
           (views_calibs(2), per-view features of seed 10 + v) and one query_sr on other points, B = 2.
encoder -> tests/golden/encoder_hg_dim_h64.npz: im_feat_lr of d48 (all three stacks, train mode) and d384 on
           weights.synthetic_image(64, seed=1), sub-sampled, with the per-channel means of the whole maps.
recon   -> tests/golden/recon_hg_dim_r32.npz: the reference's dense (eval_grid) and octree (eval_grid_octree, init_resolution 8)
           occupancy fields at R = 32 for d128 and d384, encoder on weights.synthetic_image(64, seed=1).
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from gen_golden import CALIB, FLAGS, GOLD  # noqa: E402
from gen_golden_encoder_configs import _put, _save  # noqa: E402
from gen_golden_shapes import _dims, _res, make_net, run_query, shape_points, views_calibs  # noqa: E402
from surs_amd import prng, weights  # noqa: E402


def _case(D, hidden, res=None):
    out = ["--hg_dim", str(D)] + _dims("lr", [D + 65] + hidden + [1]) + _dims("hr", [D + 66] + hidden + [1])
    if res is not None:
        out += _res("lr", res) + _res("hr", res)
    return out


CASES = {
    "d128": (128, _case(128, [1024, 512, 256, 128])),            # the released hidden widths on another D: input pads to 224
    "d384": (384, _case(384, [512, 256, 128], [1, 2, 3])),       # D > 256: wider feature rows, 32-point tile
    "d48": (48, _case(48, [1000, 500, 250, 100])),               # D not a multiple of 32, widths that need zero padding
}


# query only: a hidden layer too wide for the 32-point tile on D = 128 (the three cases above all fit it), skip at layer 1
QUERY_CASES = dict(CASES, d128w=(128, _case(128, [1200, 128], [1])))


def hg_features(D, seed=3, hl=32, hh=128):
    return prng.uniform("feat_lr", seed, (D, hl, hl), -1.0, 1.0), prng.uniform("feat_hr", seed, (64, hh, hh), -1.0, 1.0)


def gen_keys():
    out = {}
    for name, (D, extra) in CASES.items():
        net = rh.build_net(rh.parse_opt(FLAGS + extra))
        out[name] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        print(name, "keys", len(out[name]))
    with open(os.path.join(GOLD, "state_dict_keys_hg_dim.json"), "w") as f:
        json.dump(out, f)


def gen_query():
    ns = rh.load_reference()
    pts = shape_points()
    out = {"points": pts}
    for name, (D, extra) in QUERY_CASES.items():
        net = make_net(extra)
        fl, fh = hg_features(D)
        net.im_feat_list_lr = [torch.from_numpy(fl[None].copy())]
        net.im_feat_list_hr = [torch.from_numpy(fh[None].copy())]
        phr, plr, lhr, llr = run_query(net, pts, CALIB)
        out.update({name + "_pred_hr": phr, name + "_logit_hr": lhr, name + "_pred_lr": plr, name + "_logit_lr": llr})
        inside = plr[plr > 0]
        print("%-5s pred_lr in-image range %.3f..%.3f, median %.3f; zeros %.3f" % (name, inside.min(), inside.max(), np.median(inside),
                                                                                  float((phr == 0).mean())))
    # d128 seen by two views: per-view features of seed 10 + v, calibrations views_calibs(2)
    D, extra = CASES["d128"]
    V = 2
    net = rh.build_net(rh.parse_opt(FLAGS + extra + ["--num_views", str(V)]))
    net.load_state_dict(make_net(extra).state_dict(), strict=True)
    f = [hg_features(D, seed=10 + v) for v in range(V)]
    net.im_feat_list_lr = [torch.from_numpy(np.stack([a for a, _ in f]))]
    net.im_feat_list_hr = [torch.from_numpy(np.stack([b for _, b in f]))]
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
    assert tuple(phr.shape) == (V, 1, pts.shape[1]) and cap["mlp_lr"].shape[0] == 1
    out.update(d128_v2_pred_hr=phr[:, 0].numpy(), d128_v2_pred_lr=plr[:, 0].numpy(), d128_v2_logit_hr=cap["mlp_hr"][0, 0].numpy(),
               d128_v2_logit_lr=cap["mlp_lr"][0, 0].numpy())
    print("d128 V=2 zeros per view", [round(float((phr[v] == 0).float().mean()), 3) for v in range(V)])
    # query_sr on other points than query_mr's, two subjects (as gen_golden_shapes.gen_query does for s1), d128
    net = make_net(extra)
    fa, fb = hg_features(D, seed=3), hg_features(D, seed=4)
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
    _save("query_hg_dim.npz", out)


def _encode(net):
    img = weights.synthetic_image(64, seed=1)
    with torch.no_grad(), rh.quiet():
        _, f_lr, f_hr = net.super_res(torch.from_numpy(img.copy()))
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)


def gen_encoder():
    out = {}
    for name in ("d48", "d384"):
        net = make_net(CASES[name][1])
        if name == "d48":
            net.train()   # (GroupNorm: the same arithmetic; HGFilters.py:208-213 keeps every stack's output)
        _encode(net)
        maps = net.im_feat_list_lr
        assert len(maps) == (3 if name == "d48" else 1) and maps[-1].shape[1] == CASES[name][0]
        _put(out, name + "_im_feat_lr", maps[-1][0].numpy(), 2)
        if name == "d48":
            for s, m in enumerate(maps):
                _put(out, "d48_stack%d" % s, m[0].numpy(), 2)
        print(name, "im_feat_lr", tuple(maps[-1].shape), "max-abs %.3g" % float(maps[-1].abs().max()))
    _save("encoder_hg_dim_h64.npz", out)


def gen_recon():
    ns = rh.load_reference()
    out = {}
    for name in ("d128", "d384"):
        extra = CASES[name][1]
        net = make_net(extra)
        opt_ref = rh.parse_opt(FLAGS + extra)
        _encode(net)
        calib = torch.from_numpy(CALIB[None].copy())
        R = 32
        coords, mat = ns.sdf.create_grid(R, R, R, np.array([-0.5] * 3), np.array([0.5] * 3))

        def eval_func(points):   # lib/mesh_util.py:20-28
            samples = torch.from_numpy(np.expand_dims(points, axis=0)).float()
            net.query_mr(samples, calib)
            net.query_sr(samples, calib)
            phr, plr = net.get_preds()
            return phr[0][0].detach().numpy(), plr[0][0].detach().numpy()

        with torch.no_grad(), rh.quiet():
            dh, dl = ns.sdf.eval_grid(coords, eval_func, num_samples=50000)
            oh, ol = ns.sdf.eval_grid_octree(types.SimpleNamespace(threshold=opt_ref.threshold), coords, eval_func, init_resolution=8,
                                             num_samples=50000)
        for k, v in (("dense_hr", dh), ("dense_lr", dl), ("octree_hr", oh), ("octree_lr", ol)):
            print("%s %-9s range %.3f..%.3f, mean %.3f, > 0.5: %.3f" % (name, k, v.min(), v.max(), v.mean(), float((v > 0.5).mean())))
            out[name + "_" + k] = v.astype(np.float32)
        out["threshold"] = np.array(opt_ref.threshold)
    out["init_resolution"] = np.array(8)
    _save("recon_hg_dim_r32.npz", out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for w in sys.argv[1:] or ["keys", "query", "encoder", "recon"]:
        globals()["gen_" + w]()
