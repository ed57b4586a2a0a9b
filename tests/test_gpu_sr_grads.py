"""GPU checks of the super-resolution gradients: the primitives of csrc/surs_sr_grad.hip against torch-CPU float64, and the network
(native.sr_train_forward / sr_backward, SuRSNet.super_res_train / super_res_backward, autograd.super_res_features) against the
reference's own float64 gradients on kink-safe images (tests/golden/sr_grads_*.npz, tools/gen_golden_sr_grads.py,
tests/sr_grad_common.py).

Bounds.  Primitives: fp32 inputs, nothing rounded to 22 bits -  max |t - t64| <= 8 * 2^-22 max |t64|  per tensor.  Network, for every
stored quantity t:  max |g - g64| / max |g64| <= 8 max(e_ref(t), 2^-20)  (e_ref: the reference's own fp32 distance from its float64
value; 2^-20: four times the classifier gradients' floor, because the forward these gradients rest on rounds its operands to 22
bits).  Every parity test prints its worst ratio before it asserts."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grad_common as gc
import sr_grad_common as sg
from surs_amd import prng

pytestmark = pytest.mark.gpu

PRIM_BOUND = 8.0 * 2.0 ** -22
LRELU, RELU = 0.2, 0.0
LRELU2 = float(np.float32(0.2) * np.float32(0.2))


# ------------------------------------------------------------------ helpers
def _dev():
    import gpu_common as g
    return g.dev()


def _img(a, ld=None):
    """numpy [C,H,W] -> native.Img with channel pitch ld, NaN in the gap."""
    from surs_amd import native
    c, h, w = a.shape
    ld = c if ld is None else ld
    buf = torch.full((h * w, ld), float("nan"), dtype=torch.float32)
    buf[:, :c] = torch.from_numpy(np.ascontiguousarray(a.transpose(1, 2, 0))).reshape(h * w, c)
    return native.Img(h, w, c, ld, buf.reshape(-1).to(_dev()))


def _chw(img):
    """native.Img -> numpy [C,H,W] (the channels only), and the gap [H*W, ld - c]."""
    t = img.buf.reshape(img.h * img.w, img.ld).cpu()
    return t[:, :img.c].reshape(img.h, img.w, img.c).permute(2, 0, 1).numpy(), t[:, img.c:]


def _u(tag, seed, shape, lo=-1.0, hi=1.0):
    return prng.uniform("sr_grad_prim_" + tag, seed, shape, lo, hi)


def _close(name, got, ref, bound=PRIM_BOUND):
    ref = np.asarray(ref, np.float64)
    dev = float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())
    print("%s: deviation %.3g of max |t64| (%.2f of the bound %.3g)" % (name, dev, dev / bound, bound))
    assert np.isfinite(np.asarray(got)).all(), name
    assert dev <= bound, (name, dev, bound)


_prim_ref = {}


def _prim(cin, cout, h, w, k, stride, slope=None):
    """Seeded inputs of one convolution and the float64 gradients of <g, act(conv(x))> (cached: computed once per shape)."""
    key = (cin, cout, h, w, k, stride, slope)
    if key not in _prim_ref:
        pad = k // 2
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        x, wt = _u("x", cin + h, (cin, h, w)), _u("w", cout + k, (cout, cin, k, k))
        g = _u("g", cout + ho, (cout, ho, wo))
        y = None
        x64 = torch.from_numpy(x).double()[None].requires_grad_()
        w64 = torch.from_numpy(wt).double().requires_grad_()
        b64 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        z = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
        if slope is not None:
            # the STORED output decides the mask: a seeded map with exact zeros of both signs, not conv(x)'s own sign
            y = _u("y", cout + wo, (cout, ho, wo))
            y.reshape(-1)[::7] = 0.0
            y.reshape(-1)[3::11] = -0.0
            dz = torch.from_numpy(g).double() * torch.where(torch.from_numpy(y) > 0, 1.0, float(np.float32(slope))).double()
        else:
            dz = torch.from_numpy(g).double()
        gx, gw, gb = torch.autograd.grad((z * dz[None]).sum(), (x64, w64, b64))
        _prim_ref[key] = dict(x=x, w=wt, g=g, y=y, dx=gx[0].numpy(), dw=gw.numpy(), db=gb.numpy(), ho=ho, wo=wo)
    return _prim_ref[key]


def _run_prim(p, k, stride, slope=None, pitch=0, want_dx=True):
    from surs_amd import native
    cin, cout = p["x"].shape[0], p["g"].shape[0]
    x, g = _img(p["x"], cin + pitch if pitch else None), _img(p["g"], cout + pitch if pitch else None)
    y = _img(p["y"], cout + 2 * pitch if pitch else None) if p["y"] is not None else None
    s = 1.0 if slope is None else slope
    dw, db = native.conv_grad_weight(g, x, k, stride, y=y, slope=s)
    dx = None
    if want_dx:
        wt = torch.from_numpy(p["w"]).to(_dev())
        out = _img(np.full(p["x"].shape, np.nan, np.float32), cin + pitch if pitch else None)
        dx = native.conv_grad_input(g, wt, x.h, x.w, stride, y=y, slope=s, dx=out)
    return dw, db, dx


# ------------------------------------------------------------------ primitives
PRIMS = [  # cin, cout, h, w, k, stride, input gradient too
    (32, 3, 8, 16, 3, 1, True), (3, 32, 8, 16, 3, 1, False), (512, 512, 1, 2, 3, 1, True),
    (64, 64, 24, 44, 3, 1, True),      # 1056 output pixels: two parts of the 1024-pixel split, the second stage of the reduction adds
    (32, 32, 8, 16, 3, 2, True), (32, 32, 6, 10, 3, 2, True), (64, 64, 8, 16, 1, 1, True),
]


@pytest.mark.parametrize("cin,cout,h,w,k,stride,want_dx", PRIMS)
def test_conv_gradients_against_float64(cin, cout, h, w, k, stride, want_dx):
    p = _prim(cin, cout, h, w, k, stride)
    dw, db, dx = _run_prim(p, k, stride, want_dx=want_dx)
    tag = "%d->%d %dx%d k%d s%d" % (cin, cout, h, w, k, stride)
    assert tuple(dw.shape) == (cout, cin, k, k) and tuple(db.shape) == (cout,)
    _close(tag + " dW", dw.cpu().numpy(), p["dw"])
    _close(tag + " db", db.cpu().numpy(), p["db"])
    if want_dx:
        got, _ = _chw(dx)
        _close(tag + " dX", got, p["dx"])


@pytest.mark.parametrize("slope", [LRELU, RELU])
@pytest.mark.parametrize("stride", [1, 2])
def test_activation_masks_from_the_stored_output(slope, stride):
    """LeakyReLU(0.2) and ReLU: the derivative comes from the stored output y, y == 0 and y == -0 on the negative side; with channel
    pitches above the channel count and NaN in every gap, before and after."""
    p = _prim(32, 32, 8, 16, 3, stride, slope)
    assert (p["y"] == 0).sum() > 50 and np.signbit(p["y"][p["y"] == 0]).any() and not np.signbit(p["y"][p["y"] == 0]).all()
    dw, db, dx = _run_prim(p, 3, stride, slope, pitch=5)
    tag = "mask %.1f s%d" % (slope, stride)
    _close(tag + " dW", dw.cpu().numpy(), p["dw"])
    _close(tag + " db", db.cpu().numpy(), p["db"])
    got, gap = _chw(dx)
    _close(tag + " dX", got, p["dx"])
    assert gap.shape[1] == 5 and bool(torch.isnan(gap).all())       # the gap of the output was not written
    # the same values without pitches: the bits do not depend on the pitch
    dw0, db0, dx0 = _run_prim(p, 3, stride, slope)
    assert torch.equal(dw, dw0) and torch.equal(db, db0) and np.array_equal(got, _chw(dx0)[0])


def test_unshuffle_mask_is_exact():
    """conv -> LeakyReLU -> PixelShuffle -> LeakyReLU stores the shuffled map: (y > 0 ? 1 : 0.2f * 0.2f), pitches with NaN gaps."""
    from surs_amd import native
    c, h, w = 8, 3, 5
    g, y = _u("ug", 1, (c, 2 * h, 2 * w)), _u("uy", 2, (c, 2 * h, 2 * w))
    y.reshape(-1)[::5] = 0.0
    y.reshape(-1)[2::9] = -0.0
    want = F.pixel_unshuffle(torch.from_numpy(g) * torch.where(torch.from_numpy(y) > 0, torch.tensor(1.0), torch.tensor(LRELU2)), 2).numpy()
    for pitch in (0, 3):
        out = _img(np.full((4 * c, h, w), np.nan, np.float32), 4 * c + pitch)
        native.pixel_unshuffle2_grad(_img(g, c + pitch), _img(y, c + 2 * pitch), LRELU2, out=out)
        got, gap = _chw(out)
        assert np.array_equal(got, want)
        assert bool(torch.isnan(gap).all())


def test_input_gradient_adds_into_a_filled_buffer():
    from surs_amd import native
    for stride in (1, 2):
        p = _prim(32, 32, 8, 16, 3, stride)
        g, wt = _img(p["g"]), torch.from_numpy(p["w"]).to(_dev())
        plain = native.conv_grad_input(g, wt, 8, 16, stride)
        fill = _u("fill", stride, (32, 8, 16))
        acc = native.conv_grad_input(g, wt, 8, 16, stride, dx=_img(fill, 37), add=True)
        got, gap = _chw(acc)
        assert np.array_equal(got, fill + _chw(plain)[0])           # one fp32 addition per element
        assert bool(torch.isnan(gap).all())


def test_weight_gradient_accumulates():
    from surs_amd import native
    p = _prim(64, 64, 24, 44, 3, 1)
    g, x = _img(p["g"]), _img(p["x"])
    dw, db = native.conv_grad_weight(g, x, 3, 1)
    dw2, db2 = dw.clone(), db.clone()
    native.conv_grad_weight(g, x, 3, 1, dw=dw2, db=db2, accumulate=True)
    assert torch.equal(dw2, dw + dw) and torch.equal(db2, db + db)


# ------------------------------------------------------------------ the network
_nets = {}


class _Case:
    def __init__(self, golden_dir, name):
        from surs_amd import model
        self.name = name
        self.gold = sg.load_fixture(golden_dir, name)
        self.opt = sg.opt(name)
        self.net = model.SuRSNet(self.opt).to(device=_dev())
        self.net.load_state_dict(sg.state_dict(name))
        self.x_np = sg.images(name, int(self.gold["seed"]))
        self.x = torch.from_numpy(self.x_np).to(_dev())
        self.G_np = sg.upstream(name)
        self.G = tuple(torch.from_numpy(g).to(_dev()) for g in self.G_np)
        self.B = self.x.shape[0]
        self._golds = {(True, True, True): self.gold}

    def gold_for(self, use):
        """The fixture for all three terms; for a subset, the float64 restatement with its own fp32 distance as e_ref (computed once)."""
        if use not in self._golds:
            g64, _, _ = sg.grads_of(self.name, self.x_np, self.G_np, torch.float64, use=use)
            g32, _, _ = sg.grads_of(self.name, self.x_np, self.G_np, torch.float32, use=use)
            gold = {}
            for k in g64:
                for (qn, q64), (_, q32) in zip(gc.quantities(k, g64[k]), gc.quantities(k, g32[k])):
                    top = float(np.abs(q64).max())
                    gold[qn], gold[qn + "|e_ref"] = q64, (float(np.abs(q32 - q64).max()) / top if top > 0 else 0.0)
            self._golds[use] = gold
        return self._golds[use]

    def native_net(self):
        from surs_amd import encoder
        return encoder._native_net(self.net._encoder_weights()).net

    def params(self):
        return self.net._sr_param_set()[0]

    def hw(self):
        return self.x.shape[2], self.x.shape[3]

    def nhwc(self, i, b):
        return self.G[i][b].permute(1, 2, 0).contiguous()


def _case(golden_dir, name):
    if name not in _nets:
        _nets[name] = _Case(golden_dir, name)
    return _nets[name]


def _check(c, grads, use=(True, True, True), scale=1.0, tag=""):
    assert list(grads) == sg.param_keys(c.name)
    sd = sg.state_dict(c.name)
    for k, v in grads.items():
        assert tuple(v.shape) == tuple(sd[k].shape) and v.dtype == torch.float32 and v.is_cuda, k
    rows = sg.compare(c.gold_for(use), OrderedDict((k, v.cpu().numpy()) for k, v in grads.items()), scale=scale)
    name, ratio = sg.worst(rows)
    print("%s%s: %d quantities, worst deviation / bound = %.3f at %s; worst deviation / max(e_ref, 2^-20) = %.3f (bound 8)"
          % (c.name, tag, len(rows), ratio, name, max(d / (b / 8.0) for _, d, b in rows)))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad[:5]


USES = [(True, True, True), (True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.parametrize("use", USES, ids=["all", "img", "lr", "hr"])
@pytest.mark.parametrize("name", list(sg.CASES))
def test_model_parity_with_the_reference(golden_dir, name, use):
    c = _case(golden_dir, name)
    c.net.super_res_train(c.x)
    grads = c.net.super_res_backward(*[g if u else None for g, u in zip(c.G, use)])
    _check(c, grads, use, tag=" model %s" % (use,))
    if not use[0]:      # no gradient reaches last.*: exact zeros
        assert float(grads["super_resolution.last.0.weight"].abs().max()) == 0.0 and float(grads["super_resolution.last.2.bias"].abs().max()) == 0.0
    if not use[2]:
        assert float(grads["image_filter_hr.conv5.weight"].abs().max()) == 0.0
    if use == (False, True, False):
        for m in ("ups2.0", "ups3.0", "ups4.0"):
            assert float(grads["super_resolution.%s.weight" % m].abs().max()) == 0.0, m
        assert float(grads["super_resolution.head.0.weight"].abs().max()) > 0.0


@pytest.mark.parametrize("name", list(sg.CASES))
def test_native_parity_image_by_image(golden_dir, name):
    """native.sr_train_forward + native.sr_backward: one call per image, the second with accumulate; tiny's batch of two equals the sum
    of its images' gradients and the model's result bit for bit."""
    from surs_amd import native
    from surs_amd.model import _as_img
    c = _case(golden_dir, name)
    n, params, (h, w), s = c.native_net(), c.params(), c.hw(), c.opt.scale
    tapes = [native.sr_train_forward(n, _as_img(c.x[b:b + 1]), s)[-1] for b in range(c.B)]
    grads, single = None, []
    for b in range(c.B):
        single.append(native.sr_backward(n, params, tapes[b], h, w, c.nhwc(0, b), c.nhwc(1, b), c.nhwc(2, b), scale=s))
        grads = native.sr_backward(n, params, tapes[b], h, w, c.nhwc(0, b), c.nhwc(1, b), c.nhwc(2, b), grads=grads, accumulate=b > 0, scale=s)
    _check(c, grads, tag=" native")
    c.net.super_res_train(c.x)
    model_grads = c.net.super_res_backward(*c.G)
    for k in grads:
        assert torch.equal(grads[k], model_grads[k]), k
        if c.B == 2:
            assert torch.equal(grads[k], single[0][k] + single[1][k]), k
        else:
            assert torch.equal(grads[k], single[0][k]), k


@pytest.mark.parametrize("name", list(sg.CASES))
def test_tape_forward_equals_the_plain_forward(golden_dir, name):
    c = _case(golden_dir, name)
    img, f_lr, f_hr = (t.clone() for t in c.net.super_res(c.x))
    c.net.filter_hr(c.net.feature_hr)
    im_hr = c.net.im_feat_list_hr[0].clone()
    img2, f_lr2, f_hr2 = c.net.super_res_train(c.x)
    assert img2.shape == img.shape and f_lr2.shape == f_lr.shape and f_hr2.shape == f_hr.shape
    assert torch.equal(img2, img) and torch.equal(f_lr2, f_lr) and torch.equal(f_hr2, f_hr)
    assert len(c.net.im_feat_list_hr) == 1 and torch.equal(c.net.im_feat_list_hr[0], im_hr)
    assert c.net.im_SR is img2 and c.net.feature_lr is f_lr2 and c.net.feature_hr is f_hr2
    assert bool(torch.isfinite(img2).all()) and float(img2.abs().max()) > 0.0


def _fenced(nbytes, offset_bytes=0):
    """A float32 buffer of NaN with `nbytes` usable bytes starting 1024 + offset_bytes bytes into it; (whole buffer, the usable view)."""
    n = (nbytes + 3) // 4
    buf = torch.full((256 + offset_bytes // 4 + n + 256,), float("nan"), dtype=torch.float32, device=_dev())
    return buf, buf[256 + offset_bytes // 4: 256 + offset_bytes // 4 + n]


def _fences_intact(buf, view):
    lo = view.data_ptr() - buf.data_ptr()
    return bool(torch.isnan(buf[:lo // 4]).all()) and bool(torch.isnan(buf[lo // 4 + view.numel():]).all())


def _run_native(c, tape, ws, grads):
    from surs_amd import native
    from surs_amd.model import _as_img
    n, params, (h, w), s = c.native_net(), c.params(), c.hw(), c.opt.scale
    outs = None
    for b in range(c.B):
        *outs, _ = native.sr_train_forward(n, _as_img(c.x[b:b + 1]), s, tape=tape)
        native.sr_backward(n, params, tape, h, w, c.nhwc(0, b), c.nhwc(1, b), c.nhwc(2, b), grads=grads, accumulate=b > 0, workspace=ws, scale=s)
    return outs


@pytest.mark.parametrize("name", ["tiny", "blocks"])
def test_same_bits_twice_and_nothing_outside_is_written(golden_dir, name):
    """Two runs on other gradient buffers, a tape and a workspace at other addresses and other offsets inside their allocations give the
    same bits; tape, workspace and every gradient buffer sit between NaN fences that stay NaN, and every gradient is finite."""
    from surs_amd import native
    c = _case(golden_dir, name)
    n, params, (h, w) = c.native_net(), c.params(), c.hw()
    tb, wb = native.sr_tape_bytes(n, h, w), native.sr_backward_workspace_bytes(n, h, w)
    runs = []
    for tape_off, ws_off in ((0, 0), (768, 132)):        # (the tape must stay 256-byte aligned; the workspace aligns itself)
        tape_buf, tape = _fenced(tb, tape_off)
        ws_buf, ws = _fenced(wb, ws_off)
        assert tape.data_ptr() % 256 == 0
        fenced = OrderedDict((k, _fenced(v.numel() * 4)) for k, v in params.tensors.items())
        grads = OrderedDict((k, fenced[k][1].view(params.tensors[k].shape)) for k in fenced)
        outs = _run_native(c, tape, ws, grads)
        torch.cuda.synchronize()
        assert _fences_intact(tape_buf, tape) and _fences_intact(ws_buf, ws)
        for k, (buf, view) in fenced.items():
            assert _fences_intact(buf, view), k
            assert bool(torch.isfinite(view).all()), k
        runs.append((grads, [o.buf.clone() for o in outs]))
    (g0, o0), (g1, o1) = runs
    assert all(g0[k].data_ptr() != g1[k].data_ptr() for k in g0)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    _check(c, g0, tag=" fenced")


def test_small_gradients_are_not_flushed(golden_dir):
    c = _case(golden_dir, "tiny")
    c.net.super_res_train(c.x)
    scale = 2.0 ** -40
    grads = c.net.super_res_backward(*[g * scale for g in c.G])
    assert all(float(v.abs().max()) > 0.0 for v in grads.values())
    _check(c, grads, scale=scale, tag=" x 2^-40")
    full = c.net.super_res_backward(*c.G)
    for k in grads:     # a power of two commutes with every rounding on the way
        assert torch.equal(grads[k], full[k] * scale), k


def test_zero_upstream_gradient_gives_exact_zeros(golden_dir):
    c = _case(golden_dir, "tiny")
    c.net.super_res_train(c.x)
    grads = c.net.super_res_backward(*[torch.zeros_like(g) for g in c.G])
    for k, v in grads.items():
        assert float(v.abs().max()) == 0.0, k
    with pytest.raises(ValueError, match="no upstream gradient"):
        c.net.super_res_backward()


def test_reduced_encoder_is_refused_by_name(golden_dir):
    from surs_amd import encoder, model, native, options
    o = options.BaseOptions().parse(sg.flags("tiny") + ["--encoder_precision", "f16"])
    net = model.SuRSNet(o).to(device=_dev())
    net.load_state_dict(sg.state_dict("tiny"))
    x = _case(golden_dir, "tiny").x
    with pytest.raises(RuntimeError, match="parts == 1"):
        net.super_res_train(x)
    n = encoder._native_net(net._encoder_weights()).net
    assert n.parts == 1
    with pytest.raises(ValueError, match="parts == 1"):
        native.sr_tape_bytes(n, 4, 8)
    with pytest.raises(ValueError, match="parts == 1"):
        native.sr_backward_workspace_bytes(n, 4, 8)


def test_parameters_are_cached_and_dropped_by_load_state_dict(golden_dir):
    c = _case(golden_dir, "tiny")
    p = c.net.sr_parameters()
    assert p is c.net.sr_parameters() and list(p) == sg.param_keys("tiny")
    sd = sg.state_dict("tiny")
    for k, v in p.items():
        assert isinstance(v, torch.nn.Parameter) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == tuple(sd[k].shape)
        assert v.data_ptr() == c.params().tensors[k].data_ptr()             # the tensors SrParams points at
        assert np.array_equal(v.detach().cpu().numpy(), sd[k])
    c.net.load_state_dict(sd)
    assert c.net.sr_parameters() is not p


# ------------------------------------------------------------------ autograd.super_res_features
def test_autograd_function(golden_dir):
    from surs_amd import autograd
    c = _case(golden_dir, "tiny")
    net = c.net
    params = net.sr_parameters()
    outs = autograd.super_res_features(net, c.x)
    assert len(outs) == 3 and all(o.grad_fn is not None and o.requires_grad for o in outs)
    plain = net.super_res_train(c.x)
    assert torch.equal(outs[0], plain[0]) and torch.equal(outs[1], plain[1]) and torch.equal(outs[2], net.im_feat_list_hr[0])
    want = net.super_res_backward(*c.G)
    L = sum((g * o).sum() for g, o in zip(c.G, outs))
    got = torch.autograd.grad(L, list(params.values()), retain_graph=True)
    for (k, w), g in zip(want.items(), got):
        assert torch.equal(g, w), k
    # grad_output scaled by 4 scales every .grad exactly
    for p in params.values():
        p.grad = None
    (4.0 * L).backward()
    for k, p in params.items():
        assert torch.equal(p.grad, 4.0 * want[k]), k
        p.grad = None
    # an output that receives no gradient costs nothing and changes nothing: the bits of the call without it
    outs = autograd.super_res_features(net, c.x)
    got = torch.autograd.grad((c.G[0] * outs[0]).sum(), list(params.values()))
    only_img = net.super_res_backward(grad_img_SR=c.G[0])
    for (k, w), g in zip(only_img.items(), got):
        assert torch.equal(g, w), k
    assert float(only_img["image_filter_hr.conv5.weight"].abs().max()) == 0.0
    # a backward long after other work has replaced the tape on the net uses the tape of ITS forward
    outs = autograd.super_res_features(net, c.x)
    net.super_res_train(c.x[:1] * 0.5)
    got = torch.autograd.grad(sum((g * o).sum() for g, o in zip(c.G, outs)), list(params.values()))
    for (k, w), g in zip(want.items(), got):
        assert torch.equal(g, w), k


def test_autograd_backward_leaves_the_models_tape_alone(golden_dir):
    """The Function owns the tape of its forward: its backward, run after super_res_train() on ONE other image has filed the model's own
    latest tape, gives the first forward's gradients, and super_res_backward() then gives what it gives on a fresh net after that
    super_res_train() alone - the model's tape and its image count are as the train call left them."""
    from surs_amd import autograd, model
    c = _case(golden_dir, "tiny")
    net, params = c.net, c.net.sr_parameters()
    net.super_res_train(c.x)
    want = net.super_res_backward(*c.G)
    outs = autograd.super_res_features(net, c.x)
    net.super_res_train(c.x[:1] * 0.5)
    kept, filed = net._tapes[net.SR_TAPES], set(net._tapes)
    got = torch.autograd.grad(sum((g * o).sum() for g, o in zip(c.G, outs)), list(params.values()))
    for (k, w), g in zip(want.items(), got):
        assert torch.equal(g, w), k
    assert net._tapes[net.SR_TAPES] is kept and len(kept[2]) == 1 and set(net._tapes) == filed
    grads = net.super_res_backward(*[g[:1] for g in c.G])
    fresh = model.SuRSNet(c.opt).to(device=_dev())
    fresh.load_state_dict(sg.state_dict("tiny"))
    fresh.super_res_train(c.x[:1] * 0.5)
    fresh_grads = fresh.super_res_backward(*[g[:1] for g in c.G])
    assert list(grads) == list(fresh_grads)
    for k in grads:
        assert torch.equal(grads[k], fresh_grads[k]), k


def test_sgd_step_lowers_the_super_resolution_loss(golden_dir):
    """One SGD step on sr_parameters(), then load_state_dict: srweight * l1_loss(img_SR, images_hr) goes down on the same image (step
    0.01: the float64 restatement's loss falls from 0.5111 to 0.4897 with it); forward() still has no graph afterwards."""
    import forward_common as fc
    from surs_amd import autograd, model
    c = _case(golden_dir, "tiny")
    net = model.SuRSNet(c.opt).to(device=_dev())
    net.load_state_dict(sg.state_dict("tiny"))
    hr = torch.from_numpy(prng.uniform("sr_grad_hr_tiny", 21, sg.shapes("tiny")[1], 0.0, 1.0)).to(_dev())
    srweight = float(c.opt.srweight)
    params = net.sr_parameters()
    optim = torch.optim.SGD(list(params.values()), lr=0.01)
    img, _, _ = autograd.super_res_features(net, c.x)
    loss = srweight * F.l1_loss(img, hr)
    optim.zero_grad()
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    optim.step()
    sd = net.state_dict()
    sd.update({k: p.detach().cpu() for k, p in params.items()})
    net.load_state_dict(sd)
    assert net.sr_parameters() is not params
    img2, _, _ = autograd.super_res_features(net, c.x)
    loss2 = srweight * F.l1_loss(img2, hr)
    loss, loss2 = float(loss.detach()), float(loss2.detach())
    print("l1 loss %.6f -> %.6f" % (loss, loss2))
    assert loss2 < loss
    # nothing else in the package grows a graph
    net.eval()
    x = {k: torch.from_numpy(v).to(_dev()) for k, v in fc.inputs().items()}
    _, error, _ = net.forward(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"], labels_lr=x["labels_lr"],
                              labels_hr=x["labels_hr"])
    assert error.grad_fn is None and not error.requires_grad
