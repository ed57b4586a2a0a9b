"""GPU parity of the fused evaluator (surs_query_points_generic / surs_query_grid_generic) for SurfaceClassifier shapes other than
the released one, against the reference's own outputs (tests/golden/query_shapes.npz, recon_shapes_r32.npz; tools/gen_golden_shapes.py).
fp32-grade: 1e-4 on occupancies and logits; one f16 product per MAC (--precision bf16): 4e-3 on the occupancies, the bound of
test_query_50k_full_size_features_one_product_path."""
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
}


def _opt(extra, more=()):
    from surs_amd import options
    return options.BaseOptions().parse(common.FLAGS + list(extra) + list(more))


def _mlp_sd(opt):
    from surs_amd import weights
    return {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}


_packed = {}


def _packed_for(name):
    import gpu_common as g
    from surs_amd import native
    if name not in _packed:
        opt = _opt(SHAPES[name])
        sd = _mlp_sd(opt)
        _packed[name] = native.pack_mlp_generic(sd, g.dev(), native.mlp_shapes(sd, opt))
    return _packed[name]


@pytest.fixture(scope="module")
def setup():
    import gpu_common as g
    fl, fh = common.synth_features()
    return dict(g=g, Fl=g.upload_nhwc(fl), Fh=g.upload_nhwc(fh))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "query_shapes.npz"))


def _run(setup, gm, pts, calib=common.CALIB, parts=None, p_lr=None):
    from surs_amd import native
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(setup["g"].dev())
    pl = None if p_lr is None else torch.from_numpy(np.ascontiguousarray(p_lr, np.float32)).to(p.device)
    if parts is not None:
        native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        outs = native.query_points_generic(p, np.asarray(calib, np.float32).reshape(-1)[:12], ZMUL, ZDIV, setup["Fl"], setup["Fh"], gm,
                                           p_lr=pl, want_logits=True)
    finally:
        if parts is not None:
            native.check(native.lib().surs_set_operand_split_local(0))
    return [None if o is None else o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("parts", [2, 3])
def test_shapes_fp32_grade_vs_reference(setup, gold, name, parts):
    phr, plr, lhr, llr = _run(setup, _packed_for(name), gold["points"], parts=parts)
    lr = "s1" if name == "mixed" else name
    assert np.abs(phr - gold[name + "_pred_hr"]).max() < 1e-4
    assert np.abs(lhr - gold[name + "_logit_hr"]).max() < 1e-4
    assert np.abs(plr - gold[lr + "_pred_lr"]).max() < 1e-4
    assert np.abs(llr - gold[lr + "_logit_lr"]).max() < 1e-4
    assert ((phr == 0) == (gold[name + "_pred_hr"] == 0)).all() and ((plr == 0) == (gold[lr + "_pred_lr"] == 0)).all()
    assert 0 < (phr == 0).mean() < 0.6    # (the fixture has points outside the image and inside it)


@pytest.mark.parametrize("name", ["s1", "odd", "deep"])
def test_shapes_one_product(setup, gold, name):
    phr, plr, _, _ = _run(setup, _packed_for(name), gold["points"], parts=1)
    lr = "s1" if name == "mixed" else name
    assert np.abs(phr - gold[name + "_pred_hr"]).max() < 4e-3
    assert np.abs(plr - gold[lr + "_pred_lr"]).max() < 4e-3


def test_same_bits_whatever_the_batch(setup, gold):
    """A point's result does not depend on the batch, tile or position it is evaluated in."""
    pts = gold["points"]
    gm = _packed_for("odd")
    ref = _run(setup, gm, pts)
    perm = np.random.RandomState(5).permutation(pts.shape[1])
    cuts = [0, 1, 18, 1000, 1001, 4097, pts.shape[1]]
    got = [np.empty_like(r) for r in ref]
    for a, b in zip(cuts[:-1], cuts[1:]):
        idx = perm[a:b]
        outs = _run(setup, gm, pts[:, idx])
        for g_, o in zip(got, outs):
            g_[idx] = o
    for g_, r in zip(got, ref):
        assert np.array_equal(g_, r)


def test_default_shape_through_the_fused_kernel(setup, golden_dir):
    """The released shape packed generically and run through the new kernel agrees with query.npz (the proven path's fixture)."""
    from surs_amd import native, weights
    g = np.load(os.path.join(golden_dir, "query.npz"))
    sd = {k: v for k, v in common.state_dict().items() if k.startswith("mlp_")}
    gm = native.pack_mlp_generic(sd, setup["g"].dev())
    assert native.is_default_mlp(gm.shapes)
    phr, plr, lhr, llr = _run(setup, gm, weights.synthetic_points(50000, seed=2))
    assert np.abs(phr - g["a_pred_hr"]).max() < 1e-4 and np.abs(plr - g["a_pred_lr"]).max() < 1e-4
    assert np.abs(lhr - g["a_logit_hr"]).max() < 1e-4 and np.abs(llr - g["a_logit_lr"]).max() < 1e-4
    assert ((phr == 0) == (g["a_pred_hr"] == 0)).all()


def _model(extra, more=()):
    import gpu_common as g
    from surs_amd import model, weights
    opt = _opt(extra, more)
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.eval()
    return net, opt


def test_model_query_sr_other_points_batch_of_two(gold):
    """SuRSNet.query_mr / query_sr with B = 2 and query_sr on other points (the hr classifier alone, fed query_mr's lr occupancies)."""
    import gpu_common as g
    from surs_amd import weights
    net, _ = _model(S1)
    assert net.generic_mlp() is not None
    fa, fb = common.synth_features(seed=3), common.synth_features(seed=4)
    net.im_feat_list_lr = [torch.from_numpy(np.stack([fa[0], fb[0]])).to(g.dev())]
    net.im_feat_list_hr = [torch.from_numpy(np.stack([fa[1], fb[1]])).to(g.dev())]
    n = 4099
    pts_mr = np.stack([weights.synthetic_points(n, seed=11), weights.synthetic_points(n, seed=12)])
    pts_sr = np.stack([weights.synthetic_points(n, seed=13), weights.synthetic_points(n, seed=14)])
    with torch.no_grad():
        net.query_mr(torch.from_numpy(pts_mr).to(g.dev()), torch.from_numpy(gold["sr_cal_mr"]).to(g.dev()))
        net.query_sr(torch.from_numpy(pts_sr).to(g.dev()), torch.from_numpy(gold["sr_cal_sr"]).to(g.dev()))
        phr, plr = net.get_preds()
    assert np.abs(plr[:, 0].cpu().numpy() - gold["sr_pred_lr"]).max() < 1e-4
    assert np.abs(phr[:, 0].cpu().numpy() - gold["sr_pred_hr"]).max() < 1e-4


def test_model_refuses_multiview_and_perspective():
    import gpu_common as g
    from surs_amd import model, weights
    opt = _opt(S1)
    net = model.SuRSNet(opt, projection_mode="perspective").to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    fl, fh = common.synth_features()
    net.im_feat_list_lr = [torch.from_numpy(fl[None]).to(g.dev())]
    net.im_feat_list_hr = [torch.from_numpy(fh[None]).to(g.dev())]
    pts = torch.from_numpy(weights.synthetic_points(100, seed=1)[None]).to(g.dev())
    with pytest.raises(NotImplementedError):
        net.query_mr(pts, torch.from_numpy(common.CALIB[None]).to(g.dev()))


def _encoded_s1():
    import gpu_common as g
    from surs_amd import weights
    net, opt = _model(S1)
    img = torch.from_numpy(weights.synthetic_image(64, seed=1)).to(g.dev())
    with torch.no_grad():
        _, f_lr, f_hr = net.super_res(img)
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
    return net, opt


def test_reconstruction_fields_r32(golden_dir):
    """Dense and octree sweeps at R = 32 (shape s1) against the reference's eval_grid / eval_grid_octree fields."""
    from surs_amd import mesh_util
    gold = np.load(os.path.join(golden_dir, "recon_shapes_r32.npz"))
    net, opt = _encoded_s1()
    calib = torch.from_numpy(common.CALIB[None]).to(net.device)
    bmin, bmax = np.array([-0.5] * 3), np.array([0.5] * 3)
    with torch.no_grad():
        vh, vl, _ = mesh_util.eval_volumes(opt, net, calib, 32, bmin, bmax)
        assert np.abs(vh.cpu().numpy() - gold["dense_hr"]).max() < 1e-4
        assert np.abs(vl.cpu().numpy() - gold["dense_lr"]).max() < 1e-4
        opt.threshold = float(gold["threshold"])
        oh, ol, _ = mesh_util.eval_volumes_octree(opt, net, calib, 32, bmin, bmax, init_resolution=int(gold["init_resolution"]))
    assert np.abs(oh.cpu().numpy() - gold["octree_hr"]).max() < 1e-4
    assert np.abs(ol.cpu().numpy() - gold["octree_lr"]).max() < 1e-4
    assert ((ol.cpu().numpy() == 0) == (gold["octree_lr"] == 0)).all()


def test_reconstruction_streamed_steps_aside():
    net, opt = _encoded_s1()
    net._workspace().mc_capacity.update({0: (1, 1), 1: (1, 1)})
    calib = torch.from_numpy(common.CALIB[None]).to(net.device)
    from surs_amd import mesh_util
    assert mesh_util.reconstruction_streamed(opt, net, calib, 32, np.array([-0.5] * 3), np.array([0.5] * 3)) is None


def test_gen_mesh_writes_both_objs(tmp_path):
    """train_util.gen_mesh end to end for shape s1 (octree and dense).  The box reaches past the image (|x|, |y| > 0.5 under gen_mesh's
    calibration): s1's synthetic field is above 0.5 everywhere inside it, and the masked zeros outside give the surface.  R = 64: below
    gen_mesh's init_resolution (64) the octree walk evaluates nothing, in the reference as here."""
    import gpu_common as g
    from surs_amd import train_util, weights
    net, opt = _model(S1, ["--resolution", "64"])
    img = torch.from_numpy(weights.smooth_image(64, seed=1))
    data = {"img_LR": img, "b_min": np.array([-0.6] * 3), "b_max": np.array([0.6] * 3)}
    for octree in (False, True):
        path = str(tmp_path / ("s1_%d.obj" % octree))
        with torch.no_grad():
            vh, fh, vl, fl = train_util.gen_mesh(opt, net, g.dev(), data, path, use_octree=octree)
        for suffix, f in (("_HR.obj", fh), ("_LR.obj", fl)):
            txt = open(path[:-4] + suffix).read()
            assert txt.startswith("v ") and txt.count("\nf ") + txt.startswith("f ") == len(f) > 0
