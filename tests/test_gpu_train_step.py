"""GPU checks of the whole-network training step (tests/train_step_common.py has the cases and the fixture's rule).

Against the fixture (tests/golden/train_step_*.npz): forward_backward(encoder=True), one plain SGD step on one parameter set with the
stored learning rate, forward(): both error values within r = 8 max(|e32 - e64|, 2^-20 |e64|) of the reference's float64 ones - at most
1/256 of the step's own effect on the error -; a set the variant's error does not depend on is left bit for bit where it was.
Composition: grads bit for bit the chain of public calls made by hand with NCHW tensors between them; res_hr, error, res_lr,
loss_values and the maps bit for bit forward()'s; two calls the same bits; B = 1 and 2; an image with every point outside.
Loss head: terms and total bit for bit surs_forward_losses on the NCHW-flattened inputs, d_img_sr bit for bit the torch expression.
Guard: the tables of train_step_common on the device against the host twin; Optimizer.step(guard=True) on poisoned and clean gradients."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import train_step_common as ts

pytestmark = pytest.mark.gpu

_cache = {}


def _dev():
    import gpu_common as g
    return g.dev()


def _x(case, outside=None):
    key = (case, outside)
    if key not in _cache:
        x = {k: v.copy() for k, v in ts.inputs(case).items()}
        if outside is not None:          # every point of image `outside`, of both sets, beside the image
            x["points_hr"][outside, 0] += 5.0
            x["points_lr"][outside, 0] += 5.0
        _cache[key] = {k: torch.from_numpy(v).to(_dev()) for k, v in x.items()}
    return _cache[key]


def _args(x, B=None):
    s = slice(0, B)
    return ((x["images_lr"][s], x["images_hr"][s], x["points_lr"][s], x["points_hr"][s], x["calibs"][s]),
            dict(labels_lr=x["labels_lr"][s], labels_hr=x["labels_hr"][s]))


def _sd(case):
    return OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in ts.state_dict(case).items())


def _net(case, variant="w1111", train=True):
    from surs_amd import model
    net = model.SuRSNet(ts.opt(case, variant)).to(device=_dev())
    net.load_state_dict(_sd(case))
    net.train(train)
    return net


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _masters(net):
    out = OrderedDict()
    for s in net.SETS:
        out.update(getattr(net, s + "_parameters")())
    return OrderedDict((k, p.detach().clone()) for k, p in out.items())


# ------------------------------------------------------------------ against the fixture
@pytest.mark.parametrize("case,variant", [(c, v) for c in ts.CASES for v in ts.VARIANTS])
def test_sgd_step_moves_the_error_as_the_reference(case, variant, golden_dir):
    from surs_amd import optim
    rows = ts.load_fixture(golden_dir, case)
    args, kw = _args(_x(case))
    net = _net(case, variant)
    worst = 0.0
    for which in ts.SETS:
        row = rows[(variant, which)]
        net.load_state_dict(_sd(case))
        res_hr, error, res_lr, grads = net.forward_backward(*args, encoder=True, **kw)
        assert list(grads) == ts.set_keys(case, "all")
        before = _masters(net)
        o = optim.Optimizer(net, "SGD", which=net.SETS if which == "all" else which, lr=row["lr"], momentum=0)
        assert sorted(o._keys) == sorted(ts.set_keys(case, which))
        o.step(grads)
        _, after, _ = net.forward(*args, **kw)
        e = [float(error), float(after)]
        r = ts.resolution(row)
        ratios = [abs(e[i] - row["e64"][i]) / r for i in range(2)]
        print("%s %s %s lr %g: error %.9g -> %.9g, reference %.9g -> %.9g, r %.3g, |e - e64| / r = %.3f %.3f, step / r = %.0f" % (
            case, variant, which, row["lr"], e[0], e[1], row["e64"][0], row["e64"][1], r, ratios[0], ratios[1], row["ratio"]))
        worst = max(worst, *ratios)
        if not row["live"]:
            # no gradient reaches this set: the step and the error after it are bit for bit what they were
            assert all(not g.any() for k, g in grads.items() if k in o._keys), which
            assert all(torch.equal(_bits(before[k]), _bits(v)) for k, v in _masters(net).items()), which
            _same(after, error, which)
            continue
        assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (case, variant, which, e, row["e64"], r)
        moved = [k for k, v in _masters(net).items() if not torch.equal(_bits(before[k]), _bits(v))]
        assert moved and set(moved) <= set(o._keys)
    print("%s %s: largest |e - e64| / r = %.3f" % (case, variant, worst))


# ------------------------------------------------------------------ composition
def _by_hand(net, args, kw):
    """forward_backward(encoder=True)'s seven calls through the PUBLIC methods, with contiguous NCHW tensors handed between them."""
    images_lr, images_hr, points_lr, points_hr, calibs = args
    nchw = lambda t: t.detach().clone(memory_format=torch.contiguous_format)
    img_SR, feature_lr, _ = net.super_res_train(images_lr)
    outs = net.filter_lr_train(feature_lr)
    net.im_feat_list_lr = list(outs)
    net.query_mr(points_hr, calibs, labels=kw["labels_hr"])
    net.query_sr(points_lr, calibs, labels=kw["labels_lr"])
    g_mlp, fg = net.classifier_grads(features=True)
    scale = torch.full((), float(net.opt.srweight), dtype=torch.float32, device=img_SR.device) / img_SR.numel()
    d_img = torch.sign(nchw(img_SR) - images_hr) * scale
    d_feature_lr, g_hg = net.filter_lr_backward([nchw(t) for t in fg["lr"]])
    g_sr = net.super_res_backward(nchw(d_img), nchw(d_feature_lr), nchw(fg["hr"]))
    assert nchw(d_feature_lr).is_contiguous() and nchw(fg["hr"]).stride()[-1] == 1
    merged = dict(g_mlp, **g_sr)
    merged.update(g_hg)
    return OrderedDict((k, merged[k]) for k in net.state_dict() if k in merged)


@pytest.mark.parametrize("case,B,outside", [("tiny", 2, None), ("tiny", 1, None), ("tiny", 2, 1), ("d2", 1, None)])
def test_full_gradient_is_the_chain_of_public_calls(case, B, outside):
    variant = "w1111"
    args, kw = _args(_x(case, outside), B)
    net = _net(case, variant)
    res_hr, error, res_lr, grads = net.forward_backward(*args, encoder=True, **kw)
    got = OrderedDict((k, v.clone()) for k, v in grads.items())
    mine = OrderedDict(res_hr=res_hr, error=error, res_lr=res_lr, loss_values=net.loss_values, im_SR=net.im_SR, hr=net.im_feat_list_hr[0])
    mine.update(("lr%d" % i, t) for i, t in enumerate(net.im_feat_list_lr))
    mine = OrderedDict((k, v.detach().clone()) for k, v in mine.items())
    # the keys, shapes and order
    want_keys = [k for k in net.state_dict() if k in set(net.mlp_parameters()) | set(net.sr_parameters()) | set(net.hg_parameters())]
    assert list(got) == want_keys and len(want_keys) == len(net.mlp_parameters()) + len(net.sr_parameters()) + len(net.hg_parameters())
    params = _masters(net)
    for k, g in got.items():
        assert g.dtype == torch.float32 and g.is_cuda and g.numel() == params[k].numel(), k
        assert bool(torch.isfinite(g).all()), k
    for keys in (net.mlp_parameters(), net.sr_parameters(), net.hg_parameters()):      # every set receives something
        assert any(bool(got[k].any()) for k in keys)
    # two calls: the same bits
    again = net.forward_backward(*args, encoder=True, **kw)
    for k in got:
        _same(again[3][k], got[k], "second call " + k)
    _same(again[1], error, "second call error")
    # forward() on a fresh net: the same predictions, loss and maps, bit for bit
    ref = _net(case, variant)
    r_hr, r_err, r_lr = ref.forward(*args, **kw)
    theirs = OrderedDict(res_hr=r_hr, error=r_err, res_lr=r_lr, loss_values=ref.loss_values, im_SR=ref.im_SR, hr=ref.im_feat_list_hr[0])
    theirs.update(("lr%d" % i, t) for i, t in enumerate(ref.im_feat_list_lr))
    assert list(theirs) == list(mine)
    for k in mine:
        _same(mine[k], theirs[k], "forward() " + k)
    # the chain by hand on a third net
    hand = _by_hand(_net(case, variant), args, kw)
    assert list(hand) == list(got)
    for k in got:
        _same(hand[k].reshape(-1), got[k].reshape(-1), "by hand " + k)
    if outside is not None:
        # the image whose points all lie outside contributes through the image term alone: the classifiers' gradients are those of
        # the other image's points (exact zeros from image `outside`), and nothing is NaN
        assert float(res_hr[outside].abs().max()) == 0.0 and float(res_lr[outside].abs().max()) == 0.0


def test_eval_mode_queries_the_last_stack_only():
    case = "tiny"
    args, kw = _args(_x(case))
    net = _net(case, train=False)
    res_hr, error, res_lr, grads = net.forward_backward(*args, encoder=True, **kw)
    assert len(net.im_feat_list_lr) == 1 and len(net.intermediate_preds_list_lr) == 1
    ref = _net(case, train=False)
    r_hr, r_err, r_lr = ref.forward(*args, **kw)
    _same(res_hr, r_hr, "res_hr")
    _same(error, r_err, "error")
    _same(net.loss_values, ref.loss_values, "loss_values")
    assert list(grads) == ts.set_keys(case, "all") and all(bool(torch.isfinite(g).all()) for g in grads.values())


# ------------------------------------------------------------------ the loss head
@pytest.mark.parametrize("shape,S,M", [((1, 3, 5, 7), 1, 77), ((2, 3, 8, 16), 2, 600), ((3, 3, 40, 36), 3, 70001)])
def test_loss_head_bits(shape, S, M):
    """k = 105 (no multiple of 4, fewer elements than threads), the encoder's 768, and 12 960 with more points than one pass of the
    partition (65 536): terms and total against surs_forward_losses on the NCHW-flattened values, d_img_sr against torch."""
    from surs_amd import native
    B, Cc, H, W = shape
    gen = torch.Generator().manual_seed(3)
    sr = torch.randn(shape, generator=gen)
    hr = torch.randn(shape, generator=gen)
    hr.view(-1)[::5] = sr.view(-1)[::5]                                   # exactly equal elements
    pl, ph = torch.rand((S, M), generator=gen), torch.rand((S, M), generator=gen)
    ll, lh = (torch.rand(M, generator=gen) > 0.5).float(), (torch.rand(M, generator=gen) > 0.5).float()
    sr, hr, pl, ph, ll, lh = (t.to(_dev()) for t in (sr, hr, pl, ph, ll, lh))
    sr_nhwc = sr.permute(0, 2, 3, 1).contiguous()
    for w in ((1.0, 1.0, 1.0, 1.0), (0.5, 2.0, 0.25, 1.5), (1.0, 1.0, 3.0, 1.0), (0.0, 0.0, 0.7, 0.0), (1.0, 1.0, 0.0, 1.0)):
        terms, total, d = native.forward_losses_grad(pl, ll, ph, lh, sr_nhwc, hr, w)
        t0, tot0 = native.forward_losses(pred_lr=pl, lab_lr=ll, pred_hr=ph, lab_hr=lh, img_sr=sr.contiguous(), img_hr=hr, weights=w)
        _same(terms, t0, "terms")
        _same(total, tot0, "total")
        scale = torch.full((), float(w[2]), dtype=torch.float32, device=sr.device) / sr.numel()
        want = torch.sign(sr - hr) * scale
        got = d.permute(0, 3, 1, 2)
        bad = int((_bits(got.contiguous()) != _bits(want)).sum())
        print("k %d w_sr %g: scale torch %r, fp32 w / k %r, fp32 w * (1 / k) %r, %d of %d elements differ" % (
            sr.numel(), w[2], float(scale), float(np.float32(w[2]) / np.float32(sr.numel())),
            float(np.float32(w[2]) * (np.float32(1.0) / np.float32(sr.numel()))), bad, sr.numel()))
        assert bad == 0, (shape, w)
        assert bool((got[sr == hr] == 0).all())
        host = native.forward_losses_grad_host(sr_nhwc.cpu().numpy(), hr.cpu().numpy(), w[2])
        assert np.array_equal(host.view(np.uint32), d.cpu().numpy().view(np.uint32))
    # without the gradient: the same terms; a NaN pixel: NaN in its gradient and in the image term, nowhere else
    terms2, total2, none = native.forward_losses_grad(pl, ll, ph, lh, sr_nhwc, hr, (1, 1, 1, 1), want_grad=False)
    assert none is None
    _same(terms2, native.forward_losses(pred_lr=pl, lab_lr=ll, pred_hr=ph, lab_hr=lh, img_sr=sr.contiguous(), img_hr=hr, weights=(1, 1, 1, 1))[0], "terms")
    sr_nhwc[0, 1, 2, 0] = float("nan")
    terms3, _, d3 = native.forward_losses_grad(pl, ll, ph, lh, sr_nhwc, hr, (1, 1, 1, 1))
    assert bool(torch.isnan(d3[0, 1, 2, 0])) and int(torch.isnan(d3).sum()) == 1 and bool(torch.isnan(terms3[2]))
    assert bool(torch.isfinite(terms3[[0, 1, 3]]).all())


# ------------------------------------------------------------------ the guard
def _up(a, off=0):
    buf = torch.zeros(a.size + 4 + off, dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    return t


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name", list(ts.GUARD_POISON))
def test_guard_on_the_device_equals_the_host_twin(name, off):
    """off = 1: every tensor 4 bytes beyond 16-byte alignment (the scalar path)."""
    from surs_amd import native
    arrays, want = ts.guard_table(name)
    tensors = [_up(a, off) for a in arrays]
    assert all(t.data_ptr() % 16 == 4 * off for t in tensors)
    got = int(native.tensors_nonfinite_device(tensors).item())
    assert got == want == native.tensors_nonfinite_host(arrays)


def test_guard_beyond_the_grid():
    """One tensor of 2049 chunks and three elements - more chunks than the launch has workgroups - behind 300 small ones: a NaN in its
    last element, then an infinity in chunk 2048 (the first a workgroup reaches on its second visit), then a clean table."""
    from surs_amd import native
    big = torch.zeros(2049 * 4096 + 3, dtype=torch.float32, device=_dev())
    small = [torch.ones(1 + i % 7, dtype=torch.float32, device=_dev()) for i in range(300)]
    tensors = small + [big]
    assert int(native.tensors_nonfinite_device(tensors).item()) == -1
    big[-1] = float("nan")
    assert int(native.tensors_nonfinite_device(tensors).item()) == 300
    big[-1] = 0.0
    big[2048 * 4096 + 17] = float("-inf")
    assert int(native.tensors_nonfinite_device(tensors).item()) == 300
    small[123][0] = float("inf")
    assert int(native.tensors_nonfinite_device(tensors).item()) == 123


def _optim_state(net, o):
    out = _masters(net)
    out.update(("state." + n, s.detach().clone()) for n, s in o._slabs.items())
    out["blob"] = net._mlp_blob().detach().clone()
    for i, t in enumerate(net.im_feat_list_lr):
        out["lr%d" % i] = t.detach().clone()
    return out


def test_guarded_step_skips_a_poisoned_gradient():
    from surs_amd import optim
    case = "tiny"
    args, kw = _args(_x(case))
    net = _net(case)
    _, _, _, grads = net.forward_backward(*args, encoder=True, **kw)
    grads = OrderedDict((k, v.clone()) for k, v in grads.items())
    o = optim.Optimizer(net, "ADAM", lr=1e-3)
    assert o.step(grads, guard=True) is True and o._t == 1 and o.skipped == 0 and o.last_skipped_key is None
    net.forward(*args, **kw)
    before = _optim_state(net, o)
    keys = list(o._keys)                 # the optimiser's parameter order: the sets' key orders one after the other
    victim = keys[len(keys) // 2]
    grads[victim].view(-1)[-1] = float("nan")
    grads[keys[-1]].view(-1)[0] = float("inf")
    assert o.step(grads, guard=True) is False
    assert o.skipped == 1 and o.last_skipped_key == victim and o._t == 1
    net.forward(*args, **kw)
    after = _optim_state(net, o)
    assert list(before) == list(after)
    for k in before:
        _same(after[k], before[k], "after the refused step: " + k)
    # guard=False takes the poison, as before
    o.step(grads)
    assert o._t == 2 and bool(torch.isnan(_masters(net)[victim]).any())


def test_guarded_step_on_clean_gradients_has_the_plain_step_bits():
    from surs_amd import optim
    case = "tiny"
    args, kw = _args(_x(case))
    results = []
    for guard in (False, True):
        net = _net(case)
        o = optim.Optimizer(net, "AMSgrad", lr=1e-3, weight_decay=1e-2)
        for _ in range(2):
            _, _, _, grads = net.forward_backward(*args, encoder=True, **kw)
            ret = o.step(grads, guard=guard)
            assert ret is (True if guard else None)
        net.forward(*args, **kw)
        results.append(_optim_state(net, o))
        assert o.skipped == 0
    for k in results[0]:
        _same(results[0][k], results[1][k], k)
