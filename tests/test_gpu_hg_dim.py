"""GPU parity of --hg_dim other than 256 (D lr channels per point: the fused evaluators with D as a launch argument, the encoder with
l{s} of cout = D and al{s} of cin = D), against the reference's own outputs (tests/golden/query_hg_dim.npz, encoder_hg_dim_h64.npz,
recon_hg_dim_r32.npz; tools/gen_golden_hg_dim.py).  fp32-grade: 1e-4 on occupancies and logits; one f16 product per MAC: 4e-3 on
the occupancies (the bounds of tests/test_gpu_mlp_shapes.py)."""
import os

import numpy as np
import pytest
import torch

import common

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 1024 // 2, 200.0


def _flags(D, hidden, res=None):
    s = lambda tag, v: ["--mlp_" + tag] + [str(x) for x in v]
    out = ["--hg_dim", str(D)] + s("dim_lr", [D + 65] + hidden + [1]) + s("dim_hr", [D + 66] + hidden + [1])
    if res is not None:
        out += s("res_layers_lr", res) + s("res_layers_hr", res)
    return out


CASES = {   # (the flags tools/gen_golden_hg_dim.py ran the reference with)
    "d128": (128, _flags(128, [1024, 512, 256, 128])),            # the released hidden widths on another D: input pads to 224
    "d384": (384, _flags(384, [512, 256, 128], [1, 2, 3])),       # D > 256: wider feature rows, 32-point tile
    "d48": (48, _flags(48, [1000, 500, 250, 100])),               # D not a multiple of 32, widths that need zero padding
    "d128w": (128, _flags(128, [1200, 128], [1])),                # too wide for the 32-point tile: the 16-point instantiations on D != 256
}
ENCODED = ("d128", "d384", "d48")   # (the cases with encoder / sweep fixtures)


def hg_features(D, seed=3, hl=32, hh=128):
    from surs_amd import prng
    return prng.uniform("feat_lr", seed, (D, hl, hl), -1.0, 1.0), prng.uniform("feat_hr", seed, (64, hh, hh), -1.0, 1.0)


def views_calibs(V):
    """tools/gen_golden_shapes.views_calibs: orthogonal calibrations rotated about y"""
    return np.stack([np.array([[2.0 * np.cos(a), 0, 2.0 * np.sin(a), 0.02 * v], [0, -2.0, 0, -0.01 * v],
                               [-2.0 * np.sin(a), 0, 2.0 * np.cos(a), 0], [0, 0, 0, 1]], np.float32)
                     for v, a in enumerate(np.linspace(0.0, 0.6, V))])


def _opt(extra, more=()):
    from surs_amd import options
    return options.BaseOptions().parse(common.FLAGS + list(extra) + list(more))


_packed = {}


def _packed_for(name):
    import gpu_common as g
    from surs_amd import native, weights
    if name not in _packed:
        opt = _opt(CASES[name][1])
        sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
        fl, fh = hg_features(CASES[name][0])
        _packed[name] = (native.pack_mlp_generic(sd, g.dev(), native.mlp_shapes(sd, opt)), g.upload_nhwc(fl), g.upload_nhwc(fh))
    return _packed[name]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "query_hg_dim.npz"))


def _run(name, pts, parts=None):
    import gpu_common as g
    from surs_amd import native
    gm, Fl, Fh = _packed_for(name)
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(g.dev())
    if parts is not None:
        native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        outs = native.query_points_generic(p, common.CALIB.reshape(-1)[:12], ZMUL, ZDIV, Fl, Fh, gm, want_logits=True)
    finally:
        if parts is not None:
            native.check(native.lib().surs_set_operand_split_local(0))
    return [o.cpu().numpy() for o in outs]


def test_tiles():
    from surs_amd import native
    assert [_packed_for(n)[0].info()[0] for n in ("d128", "d384", "d48", "d128w")] == [32, 32, 32, 16]
    assert native.mlp_hg_dim(_packed_for("d48")[0].shapes) == 48


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("parts", [2, 3])
def test_hg_dim_fp32_grade_vs_reference(gold, name, parts):
    phr, plr, lhr, llr = _run(name, gold["points"], parts=parts)
    for got, key in ((phr, "_pred_hr"), (lhr, "_logit_hr"), (plr, "_pred_lr"), (llr, "_logit_lr")):
        err = np.abs(got - gold[name + key]).max()
        print("%s parts %d %s max error %.3e" % (name, parts, key, err))
        assert err < 1e-4
    assert ((phr == 0) == (gold[name + "_pred_hr"] == 0)).all() and ((plr == 0) == (gold[name + "_pred_lr"] == 0)).all()
    assert 0 < (phr == 0).mean() < 0.6    # (the fixture has points outside the image and inside it)


@pytest.mark.parametrize("name", list(CASES))
def test_hg_dim_one_product(gold, name):
    phr, plr, _, _ = _run(name, gold["points"], parts=1)
    eh, el = np.abs(phr - gold[name + "_pred_hr"]).max(), np.abs(plr - gold[name + "_pred_lr"]).max()
    print("%s one product: max error hr %.3e lr %.3e" % (name, eh, el))
    assert eh < 4e-3 and el < 4e-3


def test_same_bits_whatever_the_batch(gold):
    """A point's result does not depend on the batch, tile or position it is evaluated in (D = 48: a wave's gather is partly lr,
    partly hr channels)."""
    pts = gold["points"]
    ref = _run("d48", pts)
    perm = np.random.RandomState(5).permutation(pts.shape[1])
    cuts = [0, 1, 18, 1000, 1001, 4097, pts.shape[1]]
    got = [np.empty_like(r) for r in ref]
    for a, b in zip(cuts[:-1], cuts[1:]):
        idx = perm[a:b]
        outs = _run("d48", pts[:, idx])
        for g_, o in zip(got, outs):
            g_[idx] = o
    for g_, r in zip(got, ref):
        assert np.array_equal(g_, r)


def _model(name, more=(), V=1):
    import gpu_common as g
    from surs_amd import model, weights
    opt = _opt(CASES[name][1], list(more) + (["--num_views", str(V)] if V > 1 else []))
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(_opt(CASES[name][1]), seed=0))
    net.eval()
    return net, opt


def test_two_views_d128(gold):
    """d128 seen by two views through SuRSNet.query_mr / query_sr / get_preds and the native entry, both operand splits."""
    import gpu_common as g
    from surs_amd import native
    V = 2
    net, _ = _model("d128", V=V)
    f = [hg_features(128, seed=10 + v) for v in range(V)]
    net.im_feat_list_lr = [torch.from_numpy(np.stack([a for a, _ in f])).to(g.dev())]
    net.im_feat_list_hr = [torch.from_numpy(np.stack([b for _, b in f])).to(g.dev())]
    pts = gold["points"]
    p = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], V, 0))).to(g.dev())
    c = torch.from_numpy(views_calibs(V)).to(g.dev())
    with torch.no_grad():
        net.query_mr(p, c)
        net.query_sr(p, c)
        phr, plr = net.get_preds()
    assert tuple(phr.shape) == (V, 1, pts.shape[1])
    for got, want in ((phr[:, 0].cpu().numpy(), gold["d128_v2_pred_hr"]), (plr[:, 0].cpu().numpy(), gold["d128_v2_pred_lr"])):
        print("d128 V=2 max error %.3e" % np.abs(got - want).max())
        assert np.abs(got - want).max() < 1e-4
        assert ((got == 0) == (want == 0)).all()
    fl, fh = net.views_features()
    assert fl.shape[3] == 128
    for parts in (2, 3):
        native.check(native.lib().surs_set_operand_split_local(parts))
        try:
            h, l, lh, ll = native.query_points_generic_views(p, views_calibs(V).reshape(V, 16)[:, :12], ZMUL, ZDIV, fl, fh, net.generic_mlp(),
                                                             want_logits=True)
        finally:
            native.check(native.lib().surs_set_operand_split_local(0))
        for got, key in ((h, "pred_hr"), (l, "pred_lr"), (lh, "logit_hr"), (ll, "logit_lr")):
            assert np.abs(got.cpu().numpy() - gold["d128_v2_" + key]).max() < 1e-4


@pytest.mark.parametrize("name", ["d128", "d48"])
@pytest.mark.parametrize("parts", [1, 2, 3])
def test_one_view_is_the_single_view_kernel(gold, name, parts):
    """V = 1 through the views entry gives surs_query_points_generic's bits."""
    import gpu_common as g
    from surs_amd import native
    gm, Fl, Fh = _packed_for(name)
    cal = views_calibs(2)[1:]   # (a rotated calibration: x and y depend on z)
    p = torch.from_numpy(gold["points"]).to(g.dev())
    D = CASES[name][0]
    fl, fh = Fl.buf.view(1, Fl.h, Fl.w, D), Fh.buf.view(1, Fh.h, Fh.w, 64)
    native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        one = native.query_points_generic(p, cal[0].reshape(-1)[:12], ZMUL, ZDIV, Fl, Fh, gm, want_logits=True)
        many = native.query_points_generic_views(p[None], cal.reshape(1, 16)[:, :12], ZMUL, ZDIV, fl, fh, gm, want_logits=True)
    finally:
        native.check(native.lib().surs_set_operand_split_local(0))
    for a, b in zip(one, many):
        assert torch.equal(a.reshape(-1), b.reshape(-1))


def test_model_query_sr_other_points_batch_of_two(gold):
    """SuRSNet.query_mr / query_sr with B = 2 and query_sr on other points (the hr classifier alone, fed query_mr's lr occupancies), d128."""
    import gpu_common as g
    from surs_amd import weights
    net, _ = _model("d128")
    assert net.generic_mlp() is not None
    fa, fb = hg_features(128, seed=3), hg_features(128, seed=4)
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


def test_hand_assigned_features_of_another_width_are_refused():
    """256-channel maps on a --hg_dim 128 model: ValueError naming both numbers, nothing read out of bounds."""
    import gpu_common as g
    from surs_amd import weights
    net, _ = _model("d128")
    fl, fh = common.synth_features()
    net.im_feat_list_lr = [torch.from_numpy(fl[None]).to(g.dev())]
    net.im_feat_list_hr = [torch.from_numpy(fh[None]).to(g.dev())]
    pts = torch.from_numpy(weights.synthetic_points(100, seed=1)[None]).to(g.dev())
    with pytest.raises(ValueError, match=r"256 lr .* read 128 \(--hg_dim\)"):
        net.query_mr(pts, torch.from_numpy(common.CALIB[None]).to(g.dev()))
    net2, _ = _model("d128", V=2)
    net2.im_feat_list_lr = [torch.from_numpy(np.stack([fl, fl])).to(g.dev())]
    net2.im_feat_list_hr = [torch.from_numpy(np.stack([fh, fh])).to(g.dev())]
    with pytest.raises(ValueError, match=r"256 lr .* read 128 \(--hg_dim\)"):
        net2.query_mr(pts.repeat(2, 1, 1), torch.from_numpy(views_calibs(2)).to(g.dev()))


# ------------------------------------------------------------------ encoder
def _encode(net):
    import gpu_common as g
    from surs_amd import weights
    img = torch.from_numpy(weights.synthetic_image(64, seed=1)).to(g.dev())
    with torch.no_grad():
        _, f_lr, f_hr = net.super_res(img)
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
    return [t.clone() for t in net.im_feat_list_lr]


def _check_map(enc, key, t, D):
    a = t[0].cpu().numpy()
    assert a.shape == tuple(enc[key + "_shape"]) and a.shape[0] == D, (key, a.shape)
    st = int(enc[key + "_step"])
    e1 = common.rel_err(a[..., ::st, ::st], enc[key])
    e2 = float(np.abs(a.astype(np.float64).mean((1, 2)) - enc[key + "_mean"]).max() / np.abs(enc[key]).max())
    print("%-16s rel_err %.3e, channel means %.3e of the range" % (key, e1, e2))
    assert e1 < 1e-4 and e2 < 1e-4, (key, e1, e2)


@pytest.fixture(scope="module")
def enc(golden_dir):
    return np.load(os.path.join(golden_dir, "encoder_hg_dim_h64.npz"))


@pytest.mark.parametrize("name", ["d48", "d384"])
def test_encoder_vs_reference_both_sequencers(monkeypatch, enc, name):
    """im_feat_lr [1,D,32,32] of a 64 x 64 image against the reference, from the library's sequencing and from encoder.py's
    (SURS_ENC_NATIVE=0), which return the same bits (with a ConvBlock's closing sum as a launch of its own: GroupNorm's epilogue form
    sums the statistics in another order, tests/test_gpu_encoder_net.py); train(): every stack's [D]-channel map.  D = 48: l{s}'s
    cout is not a multiple of 32 - the masked store of the pointwise kernel in its GroupNorm-statistics form."""
    from surs_amd import encoder
    D = CASES[name][0]
    net, _ = _model(name)
    assert encoder.native_enabled(net._encoder_weights())
    (last,) = _encode(net)
    assert tuple(last.shape) == (1, D, 32, 32)
    _check_map(enc, name + "_im_feat_lr", last, D)
    monkeypatch.setenv("SURS_ENC_SEPARATE_SUM", "1")
    net, _ = _model(name)
    net.train()
    a = _encode(net)
    monkeypatch.setenv("SURS_ENC_NATIVE", "0")
    assert not encoder.native_enabled(net._encoder_weights())
    b = _encode(net)
    assert len(a) == len(b) == 3 and all(tuple(t.shape) == (1, D, 32, 32) for t in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    _check_map(enc, name + "_im_feat_lr", a[-1], D)
    if name == "d48":
        for s in range(3):
            _check_map(enc, "d48_stack%d" % s, a[s], D)


@pytest.mark.parametrize("name", ["d48", "d384"])
def test_encoder_unfused_sequencing(monkeypatch, enc, name):
    """SURS_ENC_FUSED_GN=0: encoder.py's sequencing with l{s} in the in_scale / in_shift form and al{s} as a convolution of its own
    (cin = D, where the multiple-of-16 rule bites)."""
    D = CASES[name][0]
    monkeypatch.setenv("SURS_ENC_FUSED_GN", "0")
    net, _ = _model(name)
    (last,) = _encode(net)
    _check_map(enc, name + "_im_feat_lr", last, D)


# ------------------------------------------------------------------ sweeps and meshes
def _encoded(name, more=()):
    net, opt = _model(name, more)
    _encode(net)
    return net, opt


@pytest.mark.parametrize("name", ["d128", "d384"])
def test_reconstruction_fields_r32(golden_dir, name):
    """Dense and octree sweeps at R = 32 against the reference's eval_grid / eval_grid_octree fields."""
    from surs_amd import mesh_util
    gold = np.load(os.path.join(golden_dir, "recon_hg_dim_r32.npz"))
    net, opt = _encoded(name)
    calib = torch.from_numpy(common.CALIB[None]).to(net.device)
    bmin, bmax = np.array([-0.5] * 3), np.array([0.5] * 3)
    with torch.no_grad():
        vh, vl, _ = mesh_util.eval_volumes(opt, net, calib, 32, bmin, bmax)
        eh, el = np.abs(vh.cpu().numpy() - gold[name + "_dense_hr"]).max(), np.abs(vl.cpu().numpy() - gold[name + "_dense_lr"]).max()
        print("%s dense fields: max error hr %.3e lr %.3e" % (name, eh, el))
        assert eh < 1e-4 and el < 1e-4
        opt.threshold = float(gold["threshold"])
        oh, ol, _ = mesh_util.eval_volumes_octree(opt, net, calib, 32, bmin, bmax, init_resolution=int(gold["init_resolution"]))
    assert np.abs(oh.cpu().numpy() - gold[name + "_octree_hr"]).max() < 1e-4
    assert np.abs(ol.cpu().numpy() - gold[name + "_octree_lr"]).max() < 1e-4
    assert ((ol.cpu().numpy() == 0) == (gold[name + "_octree_lr"] == 0)).all()


def test_reconstruction_meshes_d128():
    """mesh_util.reconstruction (dense): both meshes non-empty and, array for array, mesh_from_volume of eval_volumes' fields (the
    normals, which marching cubes accumulates with float atomics, to 1e-5 as everywhere in the suite)."""
    from surs_amd import mesh_util
    net, opt = _encoded("d128")
    calib = torch.from_numpy(common.CALIB[None]).to(net.device)
    bmin, bmax = np.array([-0.5] * 3), np.array([0.5] * 3)
    with torch.no_grad():
        out = mesh_util.reconstruction(opt, net, net.device, calib, 32, bmin, bmax, use_octree=False)
        vh, vl, mat = mesh_util.eval_volumes(opt, net, calib, 32, bmin, bmax)
        want = mesh_util.mesh_from_volume(net, vh, mat) + mesh_util.mesh_from_volume(net, vl, mat)
    assert len(out) == len(want) == 8 and out[0].shape[0] > 0 and out[1].shape[0] > 0 and out[4].shape[0] > 0 and out[5].shape[0] > 0
    for i, (a, b) in enumerate(zip(out, want)):
        assert a.dtype == b.dtype and a.shape == b.shape
        if i in (2, 6):
            assert np.allclose(a, b, atol=1e-5)     # normals: float atomics, order-dependent in the last bits (tests/test_gpu_model.py)
        else:
            assert np.array_equal(a, b)


def test_gen_mesh_writes_both_objs(tmp_path):
    """train_util.gen_mesh end to end for d128, octree and dense, R = 64 (below gen_mesh's init_resolution the octree walk evaluates
    nothing, in the reference as here)."""
    import gpu_common as g
    from surs_amd import train_util, weights
    net, opt = _model("d128", ["--resolution", "64"])
    img = torch.from_numpy(weights.synthetic_image(64, seed=1))
    data = {"img_LR": img, "b_min": np.array([-0.5] * 3), "b_max": np.array([0.5] * 3)}
    for octree in (False, True):
        path = str(tmp_path / ("d128_%d.obj" % octree))
        with torch.no_grad():
            vh, fh, vl, fl = train_util.gen_mesh(opt, net, g.dev(), data, path, use_octree=octree)
        for suffix, f in (("_HR.obj", fh), ("_LR.obj", fl)):
            txt = open(path[:-4] + suffix).read()
            assert txt.startswith("v ") and txt.count("\nf ") + txt.startswith("f ") == len(f) > 0
