"""Encoders trained with --norm batch or with another --scale, against the reference's own outputs (tools/gen_golden_encoder_configs.py:
encoder_bn_h64*.npz, encoder_scale*.npz, recon_bn_scale4_r32.npz).  Tolerances are the project's for the same quantities: encoder tensors
common.rel_err < 1e-4 (tests/test_gpu_model.py::test_encoder_vs_reference), occupancy volumes < 1e-4 absolute (the recon_* tests).  Every map
of the fixtures is a strided sub-sample (the stride is stored with it) plus the per-channel means of the whole map."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import common

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL = 1e-4
MAPS = ("img_sr", "feature_lr", "feature_hr", "im_feat_lr", "im_feat_hr")


def _stats(gold):
    return {k[5:]: gold[k] for k in gold.files if k.startswith("stat:")}


def _model(extra, stats=None, more=()):
    """SuRSNet for common.FLAGS + extra with the synthetic weights; stats: the reference's calibrated running statistics."""
    from surs_amd import model, options, weights
    opt = options.BaseOptions().parse(common.FLAGS + list(extra) + list(more))
    sd = weights.synthetic_state_dict(opt, seed=0)
    if stats is not None:
        assert set(stats) == {k for k in sd if k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")}
        sd.update(stats)
    net = model.SuRSNet(opt).to(device=torch.device("cuda:0"))
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.eval(), opt


def _encode(net, img):
    with torch.no_grad():
        img_sr, f_lr, f_hr = net.super_res(img)
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
    assert len(net.im_feat_list_lr) == 1 and len(net.im_feat_list_hr) == 1
    return img_sr, f_lr, f_hr, net.im_feat_list_lr[-1], net.im_feat_list_hr[0]


def _check_against(gold, outs):
    for name, t in zip(MAPS, outs):
        a = t[0].cpu().numpy()
        assert a.shape == tuple(gold[name + "_shape"]), (name, a.shape)
        st = int(gold[name + "_step"])
        e1 = common.rel_err(a[..., ::st, ::st], gold[name])
        e2 = float(np.abs(a.astype(np.float64).mean((1, 2)) - gold[name + "_mean"]).max() / np.abs(gold[name]).max())
        print("%-11s rel_err %.3e, channel means %.3e of the range" % (name, e1, e2))
        assert e1 < TOL and e2 < TOL, (name, e1, e2)


def test_batchnorm_encoder_vs_reference(golden_dir):
    """--norm batch on synthetic_image(64, seed=1) with the running statistics the reference calibrated (running_var 1e-6 .. 16: eps
    and the fold both matter), every stack's output included.  Measured on the MI355X: img_SR 8.4e-7, feature_lr 1.3e-6, feature_hr 7.0e-7,
    im_feat_lr 1.8e-5, im_feat_hr 7.7e-7 of each tensor's range (bound: the encoder's 1e-4)."""
    from surs_amd import weights
    gold = np.load(os.path.join(golden_dir, "encoder_bn_h64.npz"))
    more = np.load(os.path.join(golden_dir, "encoder_bn_h64_stats.npz"))
    net, _ = _model(["--norm", "batch"], _stats(more))
    net.train()   # (keeps every stack's output - the taps - and must NOT switch to batch statistics)
    img = torch.from_numpy(weights.synthetic_image(64, seed=1)).to("cuda:0")
    with torch.no_grad():
        _, f_lr, _ = net.super_res(img)
        net.filter_lr(f_lr)
    assert len(net.im_feat_list_lr) == 3
    for i, t in enumerate(net.im_feat_list_lr):
        st = int(more["tap_out%d_step" % i])
        assert common.rel_err(t[0].cpu().numpy()[..., ::st, ::st], more["tap_out%d" % i]) < TOL, i
    net.eval()
    _check_against(gold, _encode(net, img))


@pytest.mark.parametrize("scale,h", [(4, 32), (3, 64), (1, 128)])
def test_scale_encoder_vs_reference(golden_dir, scale, h):
    from surs_amd import weights
    gold = np.load(os.path.join(golden_dir, "encoder_scale%d_h%d.npz" % (scale, h)))
    net, _ = _model(["--scale", str(scale)])
    outs = _encode(net, torch.from_numpy(weights.synthetic_image(h, seed=1)).to("cuda:0"))
    E = scale * h
    assert [tuple(t.shape) for t in outs[:3]] == [(1, 3, E, E), (1, 256, E // 4, E // 4), (1, 64, E, E)]
    _check_against(gold, outs)


def test_batchnorm_scale4_reconstruction_vs_reference(golden_dir, tmp_path):
    """--norm batch --scale 4 end to end on a 32 x 32 input: the dense R = 32 volumes of reconstruction(use_octree=False) against the
    reference's eval_grid, and gen_mesh writes both OBJ files."""
    from surs_amd import mesh_util, train_util, weights
    gold = np.load(os.path.join(golden_dir, "recon_bn_scale4_r32.npz"))
    net, opt = _model(["--norm", "batch", "--scale", "4"], _stats(gold), ["--resolution", "32"])
    img = torch.from_numpy(weights.synthetic_image(32, seed=1)).to("cuda:0")
    _encode(net, img)
    calib = torch.from_numpy(common.CALIB[None]).to(net.device)
    bmin, bmax = np.array([-0.5] * 3), np.array([0.5] * 3)
    with torch.no_grad():
        out = mesh_util.reconstruction(opt, net, net.device, calib, 32, bmin, bmax, use_octree=False)
        vh, vl, _ = mesh_util.eval_volumes(opt, net, calib, 32, bmin, bmax)
    eh, el = float(np.abs(vh.cpu().numpy() - gold["dense_hr"]).max()), float(np.abs(vl.cpu().numpy() - gold["dense_lr"]).max())
    print("dense volumes: max |d| hr %.3e, lr %.3e" % (eh, el))
    assert eh < 1e-4 and el < 1e-4
    assert out[0].shape[0] > 0 and out[1].shape[1] == 3
    path = str(tmp_path / "m.obj")
    data = {"img_LR": img.cpu(), "b_min": bmin, "b_max": bmax}
    with torch.no_grad():
        train_util.gen_mesh(opt, net, net.device, data, path, use_octree=False)
    assert all(os.path.getsize(path[:-4] + sfx) > 0 for sfx in ("_HR.obj", "_LR.obj"))


@pytest.mark.parametrize("extra,h", [(["--norm", "batch"], 64), (["--norm", "batch"], 512), (["--scale", "4"], 32),
                                     (["--norm", "batch", "--scale", "3"], 64)])
def test_both_sequencers_return_the_same_bits(monkeypatch, extra, h):
    """SURS_ENC_NATIVE=0 (encoder.py, launch by launch) and the library's sequencing (one call per network), training mode (every
    stack's output).  512: the ConvBlocks' sums leave in the convolutions' epilogues (surs_conv2d_nhwc_sum) in the library and as a launch
    of their own in encoder.py - without statistics both are the same values."""
    from surs_amd import encoder, weights
    if "batch" not in extra:   # (GroupNorm: the epilogue form sums the statistics in another order - tests/test_gpu_encoder_net.py)
        monkeypatch.setenv("SURS_ENC_SEPARATE_SUM", "1")
    net, _ = _model(extra)
    net.train()
    img = torch.from_numpy(weights.synthetic_image(h, seed=1)).to("cuda:0")

    def run():
        with torch.no_grad():
            img_sr, f_lr, f_hr = net.super_res(img)
            net.filter_hr(f_hr)
            net.filter_lr(f_lr)
        return [img_sr.clone(), f_lr.clone(), f_hr.clone(), net.im_feat_list_hr[0].clone()] + [t.clone() for t in net.im_feat_list_lr]
    assert encoder.native_enabled(net._encoder_weights())
    a = run()
    monkeypatch.setenv("SURS_ENC_NATIVE", "0")
    assert not encoder.native_enabled(net._encoder_weights())
    b = run()
    assert len(a) == len(b) == 7 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_batchnorm_graph_replays_the_eager_bits(monkeypatch):
    from surs_amd import encoder, weights
    monkeypatch.delenv("SURS_ENC_GRAPH", raising=False)
    eager, _ = _model(["--norm", "batch"], more=["--encoder_graph", "0"])
    graphed, _ = _model(["--norm", "batch"], more=["--encoder_graph", "1"])
    imgs = [torch.from_numpy(weights.synthetic_image(128, seed=s)).to("cuda:0") for s in (1, 2)]
    want = [[t.clone() for t in _encode(eager, im)] for im in imgs]
    n0 = len(encoder._graphs)
    for im, w in zip(imgs + imgs[:1], want + want[:1]):
        got = _encode(graphed, im)
        assert all(torch.equal(a, b) for a, b in zip(got, w))
    assert len(encoder._graphs) == n0 + 2   # super_res + filter_lr, captured once


def test_batchnorm_runs_no_statistics_code(monkeypatch):
    """Structural: the library counts the calls into its statistics entry points (surs_groupnorm_coeffs*, surs_*_gn, surs_conv2d_nhwc_gn_sum);
    a BatchNorm forward - either sequencer, eval and training mode, the wide-operand retry - makes none and allocates no statistics
    buffer, a GroupNorm forward makes dozens."""
    from surs_amd import native, weights
    img = torch.from_numpy(weights.synthetic_image(64, seed=1)).to("cuda:0")
    bn, _ = _model(["--norm", "batch"])
    gn, _ = _model([])
    made = []
    real = native.GnStats.__init__
    monkeypatch.setattr(native.GnStats, "__init__", lambda self, *a, **k: made.append(1) or real(self, *a, **k))
    n0 = native.stats_calls()
    def forward(net):
        with torch.no_grad():
            _, f_lr, f_hr = net.super_res(img)
            net.filter_hr(f_hr)
            net.filter_lr(f_lr)
    for seq in ("1", "0"):
        monkeypatch.setenv("SURS_ENC_NATIVE", seq)
        for training in (False, True):
            forward(bn.train(training))
    with native.wide_operands():
        forward(bn)
    assert native.stats_calls() == n0 and not made
    forward(gn)
    assert native.stats_calls() > n0 + 50


def _torch_up(x_chw, s, align):
    return torch.nn.Upsample(scale_factor=s, mode="bicubic", align_corners=align)(torch.from_numpy(x_chw[None]))[0].numpy()


def test_bicubic_up_factor_2_and_1_are_exact():
    """scale = 2: the bits of surs_bicubic_up2 (both alignments, with an addend); scale = 1: the input itself."""
    import gpu_common as g
    from surs_amd import native, prng
    x = g.upload_nhwc(prng.uniform("bu_x", 1, (3, 40, 56), -1, 1))
    ad = g.upload_nhwc(prng.uniform("bu_a", 2, (3, 80, 112), -1, 1))
    for align in (False, True):
        assert torch.equal(native.bicubic_up(x, 2, align).buf, native.bicubic_up2(x, align).buf)
        assert torch.equal(native.bicubic_up(x, 2, align, addend=ad).buf, native.bicubic_up2(x, align, addend=ad).buf)
    assert torch.equal(native.bicubic_up(x, 1).buf, x.buf)
    x32 = g.upload_nhwc(prng.uniform("bu_x32", 3, (32, 24, 40), -1, 1))
    ad32 = g.upload_nhwc(prng.uniform("bu_a32", 4, (32, 48, 80), -1, 1))
    for align in (False, True):   # the 2 x 2-block form without statistics: bicubic_up2's bits
        assert torch.equal(native.bicubic_up2_block(x32, align, addend=ad32).buf, native.bicubic_up2(x32, align, addend=ad32).buf)
    with pytest.raises(native._lib.SursError, match="integer in 1..4"):
        native.bicubic_up(x, 5)


# What is left between surs_bicubic_up and torch's CPU nn.Upsample once the coordinate arithmetic is PyTorch's.  MEASURED on the MI355X box
# (this test's printout, as a fraction of the map's range): 9.59e-7 for s = 3 on 64 -> 192, 8.6e-8 for s = 4 on 64 -> 256.  The kernel's
# arithmetic restated in numpy float32 equals torch's scalar CPU kernels (ATEN_CPU_CAPABILITY=default) bit for bit for both factors; the
# figures above are the distance of torch's own AVX512 kernels (the ones a default run takes) from its scalar ones.  Asserted: twice the
# measured value, never more than 5e-6 - the exact-phase shortcut (weights from dst mod s) measures 6.9e-6 for s = 3 on 64 -> 192.
BICUBIC_MEASURED = {3: 9.6e-7, 4: 8.6e-8}


@pytest.mark.parametrize("s", [3, 4])
def test_bicubic_up_vs_torch(s):
    import gpu_common as g
    from surs_amd import native, prng
    x = prng.uniform("bu_t", 5, (3, 64, 64), -1, 1)
    got = native.bicubic_up(g.upload_nhwc(x), s)
    got = got.buf.view(got.h, got.w, got.c).permute(2, 0, 1).cpu().numpy()
    want = _torch_up(x, s, False)
    assert got.shape == want.shape == (3, 64 * s, 64 * s)
    err = float(np.abs(got - want).max() / (want.max() - want.min()))
    print("bicubic x%d 64 -> %d: max |d| / range = %.3e" % (s, 64 * s, err))
    bound = min(2 * BICUBIC_MEASURED[s], 5e-6)
    assert err <= bound, (err, bound)


def test_conv_sum_without_statistics_against_conv_then_add():
    """surs_conv2d_nhwc_sum: value and value + residual with BatchNorm's constants in the staging - the bits of surs_conv2d_nhwc_x2
    followed by surs_add3; ragged tiles are refused."""
    import ctypes as C
    import gpu_common as g
    from surs_amd import native, prng
    h, w, cin, cout, ctot = 40, 96, 64, 32, 128
    x = g.upload_nhwc(prng.uniform("cs_x", 1, (cin, h, w), -1, 1))
    xin = g.upload_nhwc(prng.uniform("cs_r", 2, (ctot, h, w), -1, 1))
    cw = native.ConvWeights(prng.uniform("cs_w", 3, (cout, cin, 3, 3), -0.2, 0.2), None, x.buf.device)
    sc, sh = [torch.from_numpy(prng.uniform(n, 4, (cin,), -1.5, 1.5)).to("cuda:0") for n in ("cs_s", "cs_h")]
    ref_raw = native.conv2d(x, cw, in_scale=sc, in_shift=sh)
    ref_sum = native.add3(ref_raw, xin.slice(64, cout))
    raw, out = native.Img(h, w, cout), native.Img(h, w, ctot)

    def call(hh):
        native.check(native.lib().surs_conv2d_nhwc_sum(2, x.ptr(), hh, w, cin, x.ld, native._ptr(cw.w3), None, native._ptr(sc), native._ptr(sh),
                                                       raw.ptr(), cout, raw.ld, xin.slice(64, cout).ptr(), xin.ld, out.slice(64, cout).ptr(),
                                                       out.ld, native._stream()))
    n0 = native.stats_calls()
    call(h)
    hwc = lambda t: torch.as_strided(t.buf, (t.h, t.w, t.c), (t.w * t.ld, t.ld, 1), t.buf.storage_offset() + t.off)
    assert torch.equal(hwc(raw), hwc(ref_raw)) and torch.equal(hwc(out.slice(64, cout)), hwc(ref_sum))
    assert native.stats_calls() == n0
    with pytest.raises(native._lib.SursError, match="whole tiles"):
        call(h - 1)


def test_native_net_validates_the_appended_fields():
    """check_net() on the fields behind bn_end: a BatchNorm site without coefficients, an unknown norm, a factor outside 1..4 - refused
    with SURS_E_INVALID by the C entry points; the released configuration hands the struct over without the extension flag."""
    import ctypes as C
    from surs_amd import _lib, encoder, native
    bn, _ = _model(["--norm", "batch", "--scale", "4"])
    nn = encoder.NativeNet(bn._encoder_weights())
    assert nn.net.flags & _lib.ENC_EXTENDED and nn.net.norm == _lib.NORM_BATCH and nn.net.sr_scale == 4
    ask = lambda: native.lib().surs_encoder_workspace_bytes(C.byref(nn.net), 32, 32)
    assert ask() > 0
    keep = nn.net.bn_hg[5].shift
    nn.net.bn_hg[5].shift = None
    assert ask() == 0 and b"without folded coefficients" in native.lib().surs_last_error()
    nn.net.bn_hg[5].shift = keep
    nn.net.sr_scale = 5
    assert ask() == 0 and b"integer in 1..4" in native.lib().surs_last_error()
    nn.net.sr_scale, nn.net.norm = 4, 7
    assert ask() == 0 and b"'group' and 'batch'" in native.lib().surs_last_error()
    nn.net.norm = _lib.NORM_BATCH
    x, out = native.Img(31, 32, 3), (native.Img(32, 32, 256), native.Img(128, 128, 64))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_lib.SursError, match="31x32 enlarged by the factor 4 is 124x128"):
        native.check(native.lib().surs_encoder_super_res(C.byref(nn.net), x.ptr(), 31, 32, 3, 0, None, out[0].ptr(), out[1].ptr(),
                                                         native._ptr(ws), ws.numel(), native._stream()))
    gn, _ = _model([])
    assert encoder.NativeNet(gn._encoder_weights()).net.flags & _lib.ENC_EXTENDED == 0


def test_views_and_reduced_precision_follow_the_options():
    """--num_views 2 (views_features) and the one-product encoder (--encoder_precision f16) on a BatchNorm --scale 4 model: the
    per-view features are the single-view ones, the reduced encoder stays within the reduced encoder's documented distance."""
    from surs_amd import weights
    extra = ["--norm", "batch", "--scale", "4"]
    one, _ = _model(extra)
    two, _ = _model(extra, more=["--num_views", "2"])
    imgs = torch.cat([torch.from_numpy(weights.synthetic_image(32, seed=s)) for s in (1, 2)]).to("cuda:0")
    _encode(two, imgs)
    fl, fh = two.views_features()
    assert tuple(fl.shape) == (2, 32, 32, 256) and tuple(fh.shape) == (2, 128, 128, 64)
    for v in range(2):
        o = _encode(one, imgs[v:v + 1])
        assert torch.equal(o[3][0].permute(1, 2, 0), fl[v]) and torch.equal(o[4][0].permute(1, 2, 0), fh[v])
    red, _ = _model(extra, more=["--encoder_precision", "f16"])
    assert red._encoder_weights().reduced
    a, b = _encode(one, imgs[:1]), _encode(red, imgs[:1])
    assert 0 < common.rel_err(b[3].cpu().numpy(), a[3].cpu().numpy()) < 1e-2
    # reencode_wide: the retry on three bf16 parts runs the same options
    assert one.reencode_wide() and tuple(one.im_feat_list_lr[-1].shape) == (1, 256, 32, 32)
    assert common.rel_err(one.im_feat_list_lr[-1].cpu().numpy(), a[3].cpu().numpy()) < TOL


def test_encode_sharded_refuses_other_factors_and_shards_batchnorm():
    from surs_amd import dist as sdist, weights
    net, _ = _model(["--scale", "4"])
    img = torch.from_numpy(weights.synthetic_image(32, seed=1)).to("cuda:0")
    calib = torch.from_numpy(common.CALIB[None])
    with pytest.raises(ValueError, match="written for --scale 2"):
        sdist.encode_sharded(net, img, calib, 32, np.array([-0.5] * 3), np.array([0.5] * 3))
    # --norm batch, two ranks sharing the GPU (gloo): feature maps and meshes equal the replicated encoder's bit for bit
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_slab_check.py"), "2", "64", "256", "--norm", "batch"],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("sharded encoder used") == 2 and "DIFFERENT" not in r.stdout and "fallback" not in r.stdout, r.stdout
    assert "sharded == replicated == one GPU" in r.stdout and "MISMATCH" not in r.stdout, r.stdout
