"""GPU checks of the feature-map gradients (native.mlp_grads(feat_grads=...), SuRSNet.classifier_grads / forward_backward(features=True),
autograd.point_loss) against the reference's own float64 gradients on kink-safe point sets (tests/golden/feat_grads_*.npz,
tools/gen_golden_feat_grads.py, tests/feat_grad_common.py).

Parity bound, for every map tensor t:  max |g - g64| / max |g64|  <=  8 max(e_ref(t), 2^-22) - the bound of tests/test_gpu_mlp_grads.py
for the same reasons (e_ref: the reference's own fp32 distance from its float64 value; 8: another summation order and the fp32
products' roundings; 2^-22: the floor).  A pixel's sum has fewer terms than a weight's, so the bound is no looser here.  Every
parity test prints its worst ratio dev / max(e_ref, 2^-22) before it asserts."""
import numpy as np
import pytest
import torch

import common
import feat_grad_common as fg
import forward_common as fc
import grad_common as gc

pytestmark = pytest.mark.gpu

_cases = {}


class _Case:
    def __init__(self, golden_dir, name):
        import gpu_common as g
        from surs_amd import native
        dev = g.dev()
        self.name = name
        self.gold, self.x = fg.kept_inputs(golden_dir, name)
        self.sd = gc.mlp_state(name)
        self.shapes = native.mlp_shapes(self.sd, fg.opt(name))
        self.params = native.MlpParams(self.sd, dev, self.shapes)
        self.S, self.B, self.N = fg.CASES[name][:3]
        self.feat_lr = [[g.upload_nhwc(f) for f in row] for row in self.x["feat_lr"]]
        self.feat_hr = [g.upload_nhwc(f) for f in self.x["feat_hr"]]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.pts_mr, self.pts_sr = up(self.x["points_mr"]), up(self.x["points_sr"])
        self.lab_lr, self.lab_hr = up(self.x["lab_lr"]), up(self.x["lab_hr"])

    def image(self, b, weights=gc.LOSS_WEIGHTS, m_total=None, feat_grads=True, **over):
        """native.mlp_grads on image b; `over`: points_mr / points_sr / lab_lr / lab_hr and any keyword of mlp_grads."""
        from surs_amd import native
        a = dict(points_mr=self.pts_mr[b].contiguous(), points_sr=self.pts_sr[b].contiguous(), lab_lr=self.lab_lr[b],
                 lab_hr=self.lab_hr[b])
        a.update({k: over.pop(k) for k in list(over) if k in a})
        return native.mlp_grads(a["points_mr"], a["points_sr"], self.x["calib_mr"][b].reshape(-1)[:12],
                                self.x["calib_sr"][b].reshape(-1)[:12], gc.ZMUL, gc.ZDIV, self.feat_lr[b], self.feat_hr[b], self.params,
                                a["lab_lr"], a["lab_hr"], weights, m_total or self.B * self.N, feat_grads=feat_grads, **over)

    def batch(self, weights=gc.LOSS_WEIGHTS):
        """name -> numpy [B,C,h,w] of every image's maps (each image has maps of its own)."""
        per = [self.image(b, weights=weights)[1] for b in range(self.B)]
        return _stacked(per)


def _nchw(t):
    return t.permute(2, 0, 1).cpu().numpy()


def _stacked(per_image):
    S = len(per_image[0].lr)
    return fg.named([np.stack([_nchw(f.lr[s]) for f in per_image]) for s in range(S)], np.stack([_nchw(f.hr) for f in per_image]))


def _maps(f):
    return list(f.lr) + [f.hr]


def _case(golden_dir, name):
    if name not in _cases:
        _cases[name] = _Case(golden_dir, name)
    return _cases[name]


def _check(c, got, scale=1.0, tag=""):
    res = fg.compare(c.gold, got, scale=scale)
    ratio = max(dev / (bound / 8.0) for _, dev, bound in res)
    worst = max(res, key=lambda r: r[1] / r[2])
    print(c.name + tag, "tensors", len(res), "worst ratio dev / max(e_ref, 2^-22) = %.3f (bound 8) at %s: dev %.3g, bound %.3g"
          % (ratio, worst[0], worst[1], worst[2]))
    bad = [r for r in res if not r[1] <= r[2]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", list(fg.CASES))
def test_parity_with_the_reference(golden_dir, name):
    c = _case(golden_dir, name)
    got = c.batch()
    for k in fg.tensor_names(name):
        assert got[k].shape == c.gold[k].shape and got[k].dtype == np.float32, k
    _check(c, got)
    # a pixel no tap reaches (the reference's gradient is exactly 0 in all of its channels) holds exact zeros
    empty = 0
    for k in got:
        none = np.abs(c.gold[k]).max(1, keepdims=True) == 0
        empty += int(none.sum())
        assert float(np.abs(np.where(none, got[k], 0.0)).max()) == 0.0, k
    print(name, "pixels without contribution:", empty)
    assert name != "d48" or empty >= 1


@pytest.mark.parametrize("name", ["d48", "tiny"])
def test_parameter_gradients_keep_their_bits(golden_dir, name):
    c = _case(golden_dir, name)
    for b in range(c.B):
        plain = c.image(b, feat_grads=None)
        both, _ = c.image(b)
        assert list(plain) == list(both) and all(torch.equal(plain[k], both[k]) for k in plain)
        assert all(float(v.abs().max()) > 0.0 for v in plain.values())
    # ... and the predictions of the call's own forward
    _, plr0, phr0 = c.image(0, feat_grads=None, want_preds=True)
    _, plr1, phr1, f = c.image(0, want_preds=True)
    assert torch.equal(plr0, plr1) and torch.equal(phr0, phr1) and len(f.lr) == c.S


def test_two_runs_give_the_same_bits(golden_dir):
    """Other output buffers and a workspace at another address (and another offset inside its allocation)."""
    import gpu_common as g
    from surs_amd import native
    c = _case(golden_dir, "d48")
    need = native.mlp_grad_features_workspace_bytes(c.shapes) // 4
    ws_a = torch.empty(need, dtype=torch.float32, device=g.dev())
    ws_b = torch.empty(need + 4096, dtype=torch.float32, device=g.dev())[1984:1984 + need]      # (a multiple of 64 floats: 256 bytes)
    _, a = c.image(0, workspace=ws_a)
    _, b = c.image(0, workspace=ws_b)
    assert ws_a.data_ptr() != ws_b.data_ptr()
    for s, t in zip(_maps(a), _maps(b)):
        assert s.data_ptr() != t.data_ptr() and torch.equal(s, t) and float(s.abs().max()) > 0.0


def test_accumulate_features(golden_dir):
    from surs_amd import native
    c = _case(golden_dir, "tiny")
    _, fresh = c.image(1)
    nan = lambda t: torch.full_like(t, float("nan"))
    _, dirty = c.image(1, feat_grads=native.FeatGrads([nan(t) for t in fresh.lr], nan(fresh.hr)), accumulate_features=False)
    assert all(torch.equal(s, t) for s, t in zip(_maps(fresh), _maps(dirty)))
    # accumulate_features adds: image 1 on top of image 1 is twice it, up to the roundings of the additions to a map element
    _, twice = c.image(1, feat_grads=native.FeatGrads([t.clone() for t in fresh.lr], fresh.hr.clone()), accumulate_features=True)
    for s, t in zip(_maps(fresh), _maps(twice)):
        assert float((t - 2 * s).abs().max()) <= 2 * c.S * 2.0 ** -23 * float(s.abs().max())
    with pytest.raises(ValueError, match="accumulate_features needs"):
        c.image(1, feat_grads=None, accumulate_features=True)


def test_points_outside_the_image_give_exact_zeros(golden_dir):
    import gpu_common as g
    c = _case(golden_dir, "tiny")
    n = 333
    out = common.prng.uniform("grad_outside", 1, (3, n), -0.5, 0.5)
    out[0] = np.where(out[0] < 0, -0.6, 0.6) + 0.05 * out[0]          # |x| in [0.575, 0.625]: |2 x| > 1 under CALIB
    pts = torch.from_numpy(out).to(g.dev())
    zero = torch.zeros(n, device=g.dev())
    rnd = (torch.rand(n, generator=torch.Generator().manual_seed(3)) > 0.5).float().to(g.dev())
    for lab_lr, lab_hr in ((zero, zero), (rnd, 1 - rnd)):
        grads, f = c.image(0, points_mr=pts, points_sr=pts, lab_lr=lab_lr, lab_hr=lab_hr, m_total=n)
        for t in _maps(f) + list(grads.values()):
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0
    # no points at all: the maps are still zeroed
    from surs_amd import native
    none = torch.zeros((3, 0), device=g.dev())
    nan = lambda t: torch.full_like(t, float("nan"))
    _, f0 = c.image(0, points_mr=none, points_sr=none, lab_lr=zero[:0], lab_hr=zero[:0], m_total=1,
                    feat_grads=native.FeatGrads([nan(t) for t in f.lr], nan(f.hr)))
    assert all(float(t.abs().max()) == 0.0 for t in _maps(f0))


def test_border_taps_stay_inside(golden_dir):
    """Points exactly on x = +-1 / y = +-1 (in the image; the upper tap falls at W / H) among others, maps that are views into
    NaN-filled buffers, a workspace between NaN sentinels: nothing outside the views is written, and the maps are the host
    restatement's (1e-5 of each maximum: fp32 products and sums against float64)."""
    import gpu_common as g
    from surs_amd import native
    c = _case(golden_dir, "tiny")
    dev = g.dev()
    n = 96
    pts = common.prng.uniform("grad_border", 2, (3, n), -0.45, 0.45).astype(np.float32)
    pts[0, 0:12], pts[0, 12:24] = 0.5, -0.5                 # x = 2 px = +-1
    pts[1, 24:36], pts[1, 36:48] = 0.5, -0.5                # y = -2 py = -+1
    pts[0, 48:52], pts[1, 48:52] = [0.5, 0.5, -0.5, -0.5], [0.5, -0.5, 0.5, -0.5]     # the corners
    pts_sr = np.ascontiguousarray(pts[:, ::-1])
    lab = (common.prng.uniform("grad_border_lab", 3, (2, n), 0.0, 1.0) > 0.5).astype(np.float32)
    x = dict(c.x, feat_lr=c.x["feat_lr"][:1], feat_hr=c.x["feat_hr"][:1], points_mr=pts[None], points_sr=pts_sr[None],
             calib_mr=c.x["calib_mr"][:1], calib_sr=c.x["calib_sr"][:1], lab_lr=lab[:1], lab_hr=lab[1:])
    xy = gc.project(pts, common.CALIB)
    assert (np.abs(xy[0, :12]) == 1).all() and (np.abs(xy[1, 24:36]) == 1).all()
    assert all(gc.point_rows(x["feat_lr"][0][0], x["feat_hr"][0], p, common.CALIB)[1].all() for p in (pts, pts_sr))   # all in the image
    g_lr, g_hr, _ = fg.map_grads_f64(c.sd, x)
    pad = 1024
    (hl, wl), (hh, wh) = fg.CASES["tiny"][3:5]
    D = fg.opt("tiny").hg_dim
    sizes = [hl * wl * D] * c.S + [hh * wh * 64]
    buf = torch.full((pad + sum(s + pad for s in sizes),), float("nan"), device=dev)
    views, at = [], pad
    for s in sizes:
        views.append(buf[at:at + s])
        at += s + pad
    f = native.FeatGrads([v.view(hl, wl, D) for v in views[:-1]], views[-1].view(hh, wh, 64))
    need = native.mlp_grad_features_workspace_bytes(c.shapes) // 4
    big = torch.full((pad + need + pad,), float("nan"), device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c.image(0, points_mr=up(pts), points_sr=up(pts_sr), lab_lr=up(lab[0]), lab_hr=up(lab[1]), m_total=n, feat_grads=f,
            workspace=big[pad:pad + need])
    torch.cuda.synchronize()
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + need:]).all())
    inside = torch.zeros_like(buf, dtype=torch.bool)
    at = pad
    for s in sizes:
        inside[at:at + s] = True
        at += s + pad
    assert bool(torch.isnan(buf[~inside]).all()) and bool(torch.isfinite(buf[inside]).all())
    for k, got in _stacked([f]).items():
        ref = fg.named(g_lr, g_hr)[k]
        dev_ = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("border", k, "against the host restatement: %.3g of the tensor's maximum" % dev_)
        assert dev_ <= 1e-5, k


def test_small_values_survive(golden_dir):
    """All three loss weights scaled by 2^-40: 2^-40 times the unscaled gradients, within the parity bound."""
    c = _case(golden_dir, "tiny")
    k = 2.0 ** -40
    got = c.batch(weights=tuple(w * k for w in gc.LOSS_WEIGHTS))
    assert all(float(np.abs(v).max()) > 0.0 for v in got.values())
    _check(c, got, scale=k, tag=" x 2^-40")


def test_point_loss(golden_dir):
    """autograd.point_loss on the tiny case's maps as NCHW leaves: its value, torch.autograd.grad against
    classifier_grads(features=True), linearity in grad_output, the parameter gradients it leaves."""
    import gpu_common as g
    from surs_amd import autograd, model, weights
    c = _case(golden_dir, "tiny")
    dev = g.dev()
    opt = fg.opt("tiny")
    net = model.SuRSNet(opt).to(device=dev)
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.train()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    x = dict(c.x, calib_mr=c.x["calib_sr"])                       # (point_loss takes one calibration for both point sets)
    leaves = lambda: ([up(np.stack([x["feat_lr"][b][s] for b in range(c.B)])).requires_grad_() for s in range(c.S)],
                      up(np.stack(x["feat_hr"])).requires_grad_())
    args = (up(x["points_mr"]), up(x["points_sr"]), up(x["calib_sr"]), up(x["lab_lr"][:, None]), up(x["lab_hr"][:, None]))
    maps_lr, map_hr = leaves()
    loss = autograd.point_loss(net, maps_lr, map_hr, *args)
    assert loss.grad_fn is not None and loss.dim() == 0 and loss.dtype == torch.float32
    g_lr, g_hr, error = fg.map_grads_f64(c.sd, x, (opt.mlp1, opt.mlp2, opt.dispweight))
    print("point_loss", float(loss.detach()), "host restatement", error)
    assert abs(float(loss.detach()) - error) <= 1e-5 * error
    got = torch.autograd.grad(loss, maps_lr + [map_hr])
    left = net.last_classifier_grads
    grads, ref = net.classifier_grads(features=True)
    assert all(torch.equal(a, b) and a.shape == m.shape for a, b, m in zip(got, ref["lr"] + [ref["hr"]], maps_lr + [map_hr]))
    assert list(left) == list(grads) and all(torch.equal(left[k], grads[k]) for k in grads)
    for a, r in zip(got, g_lr + [g_hr]):
        assert float(np.abs(a.cpu().numpy() - r).max() / np.abs(r).max()) <= 1e-5
    # grad_output scales the result linearly (a power of two: exactly)
    maps_lr, map_hr = leaves()
    (autograd.point_loss(net, maps_lr, map_hr, *args) * 4.0).backward()
    assert all(torch.equal(m.grad, 4.0 * a) for m, a in zip(maps_lr + [map_hr], got))
    # a map that does not require grad gets none, the others theirs
    maps_lr, map_hr = leaves()
    map_hr = map_hr.detach()
    autograd.point_loss(net, maps_lr, map_hr, *args).backward()
    assert map_hr.grad is None and all(torch.equal(m.grad, a) for m, a in zip(maps_lr, got))


def test_through_the_model():
    """forward_backward(features=True) on the forward_h64 inputs (released shape, training mode: three stacks, two images)."""
    import gpu_common as g
    from surs_amd import autograd, model, options, weights
    opt = options.BaseOptions().parse(fc.flags("released"))
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.train()
    x = {k: torch.from_numpy(v).to(g.dev()) for k, v in fc.inputs().items()}
    fwd = lambda f, **kw: f(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"], labels_lr=x["labels_lr"],
                            labels_hr=x["labels_hr"], **kw)
    res_hr0, error0, res_lr0 = [t.clone() for t in fwd(net.forward)]
    grads0 = fwd(net.forward_backward)[3]
    res_hr, error, res_lr, grads, fgr = fwd(net.forward_backward, features=True)
    assert torch.equal(res_hr, res_hr0) and torch.equal(error, error0) and torch.equal(res_lr, res_lr0)
    assert error.grad_fn is None and not error.requires_grad
    assert list(grads) == list(grads0) and all(torch.equal(grads[k], grads0[k]) for k in grads)
    maps, fh = list(net.im_feat_list_lr), net.im_feat_list_hr[0]
    assert sorted(fgr) == ["hr", "img_SR", "lr"] and len(fgr["lr"]) == len(maps) == 3
    for got, m in zip(fgr["lr"] + [fgr["hr"], fgr["img_SR"]], maps + [fh, net.im_SR]):
        assert tuple(got.shape) == tuple(m.shape) and got.dtype == torch.float32 and got.is_cuda
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.0
    # img_SR: torch's own L1 backward on the same tensors
    sr = net.im_SR.detach().clone().float().requires_grad_()
    (opt.srweight * torch.nn.functional.l1_loss(sr, x["images_hr"])).backward()
    assert torch.equal(fgr["img_SR"], sr.grad)
    # against the host restatement on the encoder's own feature maps: NOT kink-safe inputs, so only loosely
    n = lambda k: x[k].cpu().numpy()
    ml, mh = [m.cpu().numpy() for m in maps], fh.cpu().numpy()
    xin = dict(feat_lr=[[m[b] for m in ml] for b in range(fc.B)], feat_hr=[mh[b] for b in range(fc.B)], points_mr=n("points_hr"),
               points_sr=n("points_lr"), calib_mr=n("calibs"), calib_sr=n("calibs"), lab_lr=n("labels_hr")[:, 0], lab_hr=n("labels_lr")[:, 0])
    sd = net.state_dict()
    g_lr, g_hr, _ = fg.map_grads_f64({k: sd[k].numpy() for k in sd if k.startswith("mlp_")}, xin, (opt.mlp1, opt.mlp2, opt.dispweight))
    for name, got, ref in [("lr%d" % s, fgr["lr"][s], g_lr[s]) for s in range(3)] + [("hr", fgr["hr"], g_hr)]:
        d = float(np.abs(got.cpu().numpy() - ref).max() / np.abs(ref).max())
        print(name, "against the host restatement: %.3g of the tensor's maximum" % d)
        assert d <= 1e-2, name
    # point_loss on the same maps, points and labels (forward's own crossing of its label arguments) gives the same gradients
    leaves = [m.detach().clone().requires_grad_() for m in maps + [fh]]
    loss = autograd.point_loss(net, leaves[:-1], leaves[-1], x["points_hr"], x["points_lr"], x["calibs"], x["labels_hr"], x["labels_lr"])
    back = torch.autograd.grad(loss, leaves)
    assert all(torch.equal(a, b) for a, b in zip(back, fgr["lr"] + [fgr["hr"]]))
    assert all(torch.equal(net.last_classifier_grads[k], grads[k]) for k in grads)
    # one gradient-descent step on im_feat_list_hr[0] itself, assigned back to the model, lowers the loss of the same batch
    step = 0.01 / float(fgr["hr"].abs().max())                    # the largest change of a map element: 0.01
    net.im_feat_list_lr, net.im_feat_list_hr = maps, [fh - step * fgr["hr"]]
    net.query_mr(x["points_hr"], x["calibs"], labels=x["labels_hr"])
    net.query_sr(x["points_lr"], x["calibs"], labels=x["labels_lr"])
    _, error1 = net.loss_terms(net.im_SR, x["images_hr"])
    print("error", float(error0), "->", float(error1), "after one step on the hr map, step", step)
    assert float(error1) < float(error0)
    # forward() still builds no graph
    _, error2, _ = fwd(net.forward)
    assert error2.grad_fn is None and torch.equal(error2, error0)
