"""GPU parity of the fused multi-view evaluator (surs_query_points_generic_views / surs_query_grid_generic_views) for SurfaceClassifier
shapes other than the released one, against the reference's own --num_views outputs (tests/golden/query_shapes_views.npz,
query_shapes_views4.npz, recon_shapes_views_r32.npz; tools/gen_golden_shapes.py views).  fp32-grade: 1e-4 on occupancies and
logits; one f16 product per MAC (--precision bf16): 4e-3 on the occupancies."""
import os

import numpy as np
import pytest
import torch

import common

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 1024 // 2, 200.0


def _dims(tag, dims):
    return ["--mlp_dim_" + tag] + [str(d) for d in dims]


def _res(tag, res):
    return ["--mlp_res_layers_" + tag] + [str(r) for r in res]


S1 = _dims("lr", [321, 512, 256, 128, 1]) + _dims("hr", [322, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _res("hr", [1, 2, 3])
SHAPES = {   # (the flags tools/gen_golden_shapes.py ran the reference with)
    "s1": S1,
    "nores": ["--no_residual"],
    "deep": _dims("lr", [321, 1024, 1024, 512, 256, 128, 1]) + _dims("hr", [322, 1024, 1024, 512, 256, 128, 1])
    + _res("lr", [2, 3, 4, 5]) + _res("hr", [2, 3, 4, 5]),
    "odd": _dims("lr", [321, 1000, 500, 250, 100, 1]) + _dims("hr", [322, 1000, 500, 250, 100, 1]),
    "res0": _res("lr", [0, 2]) + _res("hr", [0, 2]),
    "l1": _dims("lr", [321, 1]) + _dims("hr", [322, 1]) + ["--no_residual"],
    "mixed": _dims("lr", [321, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _dims("hr", [322, 1000, 500, 250, 100, 1]),
    "l2": _dims("lr", [321, 64, 1]) + _dims("hr", [322, 64, 1]) + _res("lr", [1]) + _res("hr", [1]),
}
CASES = [(name, 2) for name in SHAPES] + [("s1", 4), ("deep", 4)]


def views_calibs(V):
    """tools/gen_golden_shapes.views_calibs: orthogonal calibrations rotated about y"""
    return np.stack([np.array([[2.0 * np.cos(a), 0, 2.0 * np.sin(a), 0.02 * v], [0, -2.0, 0, -0.01 * v],
                               [-2.0 * np.sin(a), 0, 2.0 * np.cos(a), 0], [0, 0, 0, 1]], np.float32)
                     for v, a in enumerate(np.linspace(0.0, 0.6, V))])


def views_features(V):
    f = [common.synth_features(seed=10 + v) for v in range(V)]
    return np.stack([a for a, _ in f]), np.stack([b for _, b in f])


def _opt(extra, more=()):
    from surs_amd import options
    return options.BaseOptions().parse(common.FLAGS + list(extra) + list(more))


def _model(name, V, more=(), projection="orthogonal", features=True):
    import gpu_common as g
    from surs_amd import model, weights
    opt = _opt(SHAPES[name], ["--num_views", str(V)] + list(more))
    net = model.SuRSNet(opt, projection_mode=projection).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(_opt(SHAPES[name]), seed=0))
    net.eval()
    if features:
        fl, fh = views_features(V)
        net.im_feat_list_lr = [torch.from_numpy(fl).to(g.dev())]
        net.im_feat_list_hr = [torch.from_numpy(fh).to(g.dev())]
    return net, opt


@pytest.fixture(scope="module")
def gold():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = dict(np.load(os.path.join(d, "query_shapes_views.npz")))
    out.update(np.load(os.path.join(d, "query_shapes_views4.npz")))
    return out


def _query(net, pts, calibs, pts_sr=None):
    dev = net._device()
    V = calibs.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], V, 0))).to(dev)
    c = torch.from_numpy(calibs).to(dev)
    with torch.no_grad():
        net.query_mr(p, c)
        if pts_sr is not None:
            p = torch.from_numpy(np.ascontiguousarray(np.repeat(pts_sr[None], V, 0))).to(dev)
        net.query_sr(p, c)
        phr, plr = net.get_preds()
    assert tuple(phr.shape) == (V, 1, p.shape[2]) and tuple(plr.shape) == (V, 1, p.shape[2])
    return phr[:, 0].cpu().numpy(), plr[:, 0].cpu().numpy()


def _native(net, pts, calibs, parts=None, p_lr=None, want_logits=True):
    from surs_amd import native
    V = calibs.shape[0]
    dev = net._device()
    p = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], V, 0) if pts.ndim == 2 else pts)).to(dev)
    fl, fh = net.views_features()
    if parts is not None:
        native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        outs = native.query_points_generic_views(p, calibs.reshape(V, 16)[:, :12], ZMUL, ZDIV, fl, fh, net.generic_mlp(),
                                                 p_lr=p_lr, want_logits=want_logits)
    finally:
        if parts is not None:
            native.check(native.lib().surs_set_operand_split_local(0))
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("name,V", CASES)
def test_views_fp32_grade_vs_reference(gold, name, V):
    """SuRSNet.query_mr / query_sr / get_preds on [V,3,N] samples: 1e-4, exact zeros where a view's mask is 0; the logits (where the
    last convolution yields one row per point) and both operand splits through the native entry."""
    net, _ = _model(name, V)
    key = "%s_v%d_" % (name, V)
    pts = gold["points"]
    phr, plr = _query(net, pts, views_calibs(V))
    for got, want in ((phr, gold[key + "pred_hr"]), (plr, gold[key + "pred_lr"])):
        assert np.abs(got - want).max() < 1e-4
        assert ((got == 0) == (want == 0)).all()
    for v in range(V):
        assert 0 < (phr[v] == 0).mean() < 0.6   # (points inside and outside every view's image)
    for parts in (2, 3):
        h, l, lh, ll = _native(net, pts, views_calibs(V), parts=parts)
        assert np.abs(h - gold[key + "pred_hr"]).max() < 1e-4 and np.abs(l - gold[key + "pred_lr"]).max() < 1e-4
        if key + "logit_hr" in gold:
            assert np.abs(lh - gold[key + "logit_hr"]).max() < 1e-4
            assert np.abs(ll - gold[key + "logit_lr"]).max() < 1e-4
    assert (key + "logit_hr" in gold) == (len(net.generic_mlp().shapes[1][0]) - 1 > 2)


@pytest.mark.parametrize("name", ["s1", "deep", "odd", "l2"])
def test_views_one_product(gold, name):
    """--precision bf16: one f16 product per MAC (reduced_point_operands), 4e-3 on the occupancies."""
    net, _ = _model(name, 2, ["--precision", "bf16"])
    phr, plr = _query(net, gold["points"], views_calibs(2))
    assert np.abs(phr - gold[name + "_v2_pred_hr"]).max() < 4e-3
    assert np.abs(plr - gold[name + "_v2_pred_lr"]).max() < 4e-3


def test_views_query_sr_other_points(gold):
    """query_sr on points other than query_mr's: the hr classifier alone, channel 321 of view v = query_mr's pred_lr of view v."""
    net, _ = _model("s1", 2)
    phr, plr = _query(net, gold["sr_points_mr"], views_calibs(2), pts_sr=gold["sr_points_sr"])
    assert np.abs(plr - gold["sr_pred_lr"]).max() < 1e-4
    assert np.abs(phr - gold["sr_pred_hr"]).max() < 1e-4


@pytest.mark.parametrize("parts", [1, 2, 3])
def test_one_view_is_the_single_view_kernel(gold, parts):
    """V = 1 through both views entries gives surs_query_points_generic's / surs_query_grid_generic's bits."""
    import gpu_common as g
    from surs_amd import native
    net, _ = _model("s1", 1)
    gm = net.generic_mlp()
    cal = views_calibs(2)[1:]   # (a rotated calibration: x and y depend on z)
    pts = gold["points"]
    fl, fh = net.views_features()
    native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        p = torch.from_numpy(pts).to(g.dev())
        one = native.query_points_generic(p, cal[0].reshape(-1)[:12], ZMUL, ZDIV, *net.features(), gm, want_logits=True)
        many = native.query_points_generic_views(p[None], cal.reshape(1, 16)[:, :12], ZMUL, ZDIV, fl, fh, gm, want_logits=True)
        sr_one = native.query_points_generic(p, cal[0].reshape(-1)[:12], ZMUL, ZDIV, *net.features(), gm, p_lr=one[1])
        sr_many = native.query_points_generic_views(p[None], cal.reshape(1, 16)[:, :12], ZMUL, ZDIV, fl, fh, gm, p_lr=one[1][None])
        R = 24
        from surs_amd.sdf import create_grid
        mat = create_grid(R, R, R, np.array([-0.5] * 3), np.array([0.5] * 3))[1][:3].reshape(-1)
        g_one = native.query_grid_generic(3, 17, R, R, mat, cal[0].reshape(-1)[:12], ZMUL, ZDIV, *net.features(), gm)
        g_many = native.query_grid_generic_views(3, 17, R, R, mat, cal.reshape(1, 16)[:, :12], ZMUL, ZDIV, fl, fh, gm)
    finally:
        native.check(native.lib().surs_set_operand_split_local(0))
    for a, b in zip(one, many):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
    assert torch.equal(sr_one[0], sr_many[0][0])
    for a, b in zip(g_one, g_many):
        assert torch.equal(a, b)


def test_same_bits_whatever_the_batch(gold):
    """A point's result does not depend on N, its position or its tile: a permuted order, in pieces of ragged sizes (4099 among
    them), gives the same bits per point."""
    net, _ = _model("odd", 2)
    pts = gold["points"]
    cal = views_calibs(2)
    ref = _native(net, pts, cal)
    perm = np.random.RandomState(5).permutation(pts.shape[1])
    cuts = [0, 1, 18, 4117, pts.shape[1]]   # (4099 points in the third piece)
    got = [np.empty_like(r) for r in ref]
    for a, b in zip(cuts[:-1], cuts[1:]):
        idx = perm[a:b]
        outs = _native(net, pts[:, idx], cal)
        for g_, o, r in zip(got, outs, ref):
            g_[..., idx] = o
    for g_, r in zip(got, ref):
        assert np.array_equal(g_, r)


def test_reconstruction_fields_r32():
    """Dense and octree sweeps at R = 32 (shape s1, two views) against the reference's eval_grid / eval_grid_octree fields over its
    multi-view eval_func (view 0's predictions)."""
    from surs_amd import mesh_util
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recon_shapes_views_r32.npz"))
    net, opt = _model("s1", 2)
    calib = torch.from_numpy(views_calibs(2)).to(net._device())
    bmin, bmax = np.array([-0.5] * 3), np.array([0.5] * 3)
    with torch.no_grad():
        vh, vl, _ = mesh_util.eval_volumes_views(opt, net, calib, 32, bmin, bmax)
        assert np.abs(vh.cpu().numpy() - gold["dense_hr"]).max() < 1e-4
        assert np.abs(vl.cpu().numpy() - gold["dense_lr"]).max() < 1e-4
        opt.threshold = float(gold["threshold"])
        oh, ol, _ = mesh_util.eval_volumes_octree_views(opt, net, calib, 32, bmin, bmax, init_resolution=int(gold["init_resolution"]))
    for got, want in ((oh.cpu().numpy(), gold["octree_hr"]), (ol.cpu().numpy(), gold["octree_lr"])):
        assert np.abs(got - want).max() < 1e-4
        assert ((got == 0) == (want == 0)).all()


def test_gen_mesh_writes_both_objs(tmp_path):
    """train_util.gen_mesh end to end with --num_views 2 (shape s1; its one calibration serves both views), octree and dense."""
    import gpu_common as g
    from surs_amd import train_util, weights
    net, opt = _model("s1", 2, ["--resolution", "64"], features=False)
    img = torch.from_numpy(np.concatenate([weights.smooth_image(64, seed=1), weights.smooth_image(64, seed=2)]))
    data = {"img_LR": img, "b_min": np.array([-0.6] * 3), "b_max": np.array([0.6] * 3)}
    for octree in (False, True):
        path = str(tmp_path / ("s1_%d.obj" % octree))
        with torch.no_grad():
            vh, fh, vl, fl = train_util.gen_mesh(opt, net, g.dev(), data, path, use_octree=octree)
        for suffix, f in (("_HR.obj", fh), ("_LR.obj", fl)):
            txt = open(path[:-4] + suffix).read()
            assert txt.startswith("v ") and txt.count("\nf ") + txt.startswith("f ") == len(f) > 0


def test_perspective_still_refused(gold):
    net, _ = _model("s1", 2, projection="perspective")
    with pytest.raises(NotImplementedError):
        _query(net, gold["points"][:, :100], views_calibs(2))
