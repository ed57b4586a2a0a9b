"""GPU checks of the validation forward: every stack's predictions bit for bit against the single-map entries, SuRSNet.forward
against the reference's own outputs (tests/golden/forward_h64.npz, tools/gen_golden_forward.py), the deterministic loss reduction.
fp32-grade: 1e-4 on every stack's occupancies (the standing bound, end to end through the encoder); the loss bounds follow from
it - |p - label| <= 1 gives |d MSE| <= 2e-4 + 1e-8 < 2.1e-4 per MSE term, |disp| <= 2 with two predictions gives 8e-4 + 4e-8 < 8.1e-4,
the L1 term moves by at most the encoder's 1e-4 of img_SR's range; the total by the weighted sum of those."""
import os
import signal

import numpy as np
import pytest
import torch

import common
import forward_common as fc

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 1024 // 2, 200.0
D128 = ["--hg_dim", "128", "--mlp_dim_lr", "193", "512", "256", "128", "1", "--mlp_dim_hr", "194", "512", "256", "128", "1",
        "--mlp_res_layers_lr", "1", "2", "3", "--mlp_res_layers_hr", "1", "2", "3"]
EXTRA = {"released": fc.SHAPES["released"], "s1": fc.SHAPES["s1"], "d128": D128}


@pytest.fixture(autouse=True)
def _time_limit():
    """Every test of this file under its own time limit."""
    def expired(signum, frame):
        raise TimeoutError("test exceeded its 600 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(600)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "forward_h64.npz"))


def _net(name, more=()):
    import gpu_common as g
    from surs_amd import model, options, weights
    base = fc.flags(name) if name in fc.SHAPES else common.FLAGS + EXTRA[name]
    opt = options.BaseOptions().parse(base + list(more))
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    return net


def _dev(x):
    import gpu_common as g
    return {k: torch.from_numpy(v).to(g.dev()) for k, v in x.items()}


_encoded = {}


def _encoded_train(name):
    """A model of the given shape with the fixture's two H = 64 images encoded in training mode: three lr maps."""
    if name not in _encoded:
        net = _net(name)
        net.train()
        x = _dev(fc.inputs())
        _, f_lr, f_hr = net.super_res(x["images_lr"])
        net.filter_lr(f_lr)
        net.filter_hr(f_hr)
        assert len(net.im_feat_list_lr) == 3 and len(net.im_feat_list_hr) == 1
        _encoded[name] = (net, x)
    return _encoded[name]


class _split:
    def __init__(self, parts):
        self.parts = parts

    def __enter__(self):
        from surs_amd import native
        native.check(native.lib().surs_set_operand_split_local(self.parts))

    def __exit__(self, *a):
        from surs_amd import native
        native.check(native.lib().surs_set_operand_split_local(0))


@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("name", ["released", "s1", "d128"])
def test_every_stack_bit_for_bit(name, parts):
    """Rows [s] of the stacks entry = the single-map entry on map s, in the three forms (both classifiers, lr only, hr only), for each
    operand split; one map through the stacks entry = the single-map entry."""
    from surs_amd import native
    net, x = _encoded_train(name)
    gm = net.generic_mlp()
    assert (gm is None) == (name == "released")
    cal = common.CALIB.reshape(-1)[:12]
    for b in range(fc.B):
        feats, fh = net.stack_features(b)
        assert len(feats) == 3 and len({f.ptr().value for f in feats}) == 3
        pts, pts2 = x["points_hr"][b].contiguous(), x["points_lr"][b].contiguous()
        given = torch.rand((3, fc.N), generator=torch.Generator().manual_seed(5 + b)).to(pts.device)
        if gm is None:
            blob, ws = net._mlp_blob(), net._workspace()
            stacks = lambda fl, **k: native.query_points_stacks(pts if "p_lr" not in k else pts2, cal, ZMUL, ZDIV, fl, fh, blob, ws, **k)
            single = lambda f: native.query_points(pts, cal, ZMUL, ZDIV, f, fh, blob, ws)
            single_hr = lambda f, pl: native.query_points_hr(pts2, cal, ZMUL, ZDIV, f, fh, blob, ws, pl)
        else:
            stacks = lambda fl, **k: native.query_points_generic_stacks(pts if "p_lr" not in k else pts2, cal, ZMUL, ZDIV, fl, fh, gm, **k)
            single = lambda f: native.query_points_generic(pts, cal, ZMUL, ZDIV, f, fh, gm)
            single_hr = lambda f, pl: native.query_points_generic(pts2, cal, ZMUL, ZDIV, f, fh, gm, p_lr=pl)[0]
        with _split(parts):
            phr, plr = stacks(feats)
            none, plr_only = stacks(feats, lr_only=True)
            phr_given, back = stacks(feats, p_lr=given)
            assert none is None and back.data_ptr() == given.data_ptr()
            for s in range(3):
                one_hr, one_lr = [t.clone() for t in single(feats[s])]
                assert torch.equal(phr[s], one_hr) and torch.equal(plr[s], one_lr), (name, parts, b, s)
                assert torch.equal(plr_only[s], one_lr), (name, parts, b, s)
                assert torch.equal(phr_given[s], single_hr(feats[s], given[s].contiguous())), (name, parts, b, s)
            assert not torch.equal(plr[0], plr[2]) and not torch.equal(phr[0], phr[2])
            # S = 1 through the new entry
            p1h, p1l = stacks(feats[2:])
            one_hr, one_lr = single(feats[2])
            assert tuple(p1h.shape) == (1, fc.N) and torch.equal(p1h[0], one_hr) and torch.equal(p1l[0], one_lr)
            assert torch.equal(stacks(feats[2:], lr_only=True)[1][0], one_lr)
            assert torch.equal(stacks(feats[2:], p_lr=given[:1].contiguous())[0][0], single_hr(feats[2], given[0].contiguous()))
        assert float((plr[2] == 0).float().mean()) > 0.05    # (the mask takes part)


def _forward(net, x):
    return net.forward(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"], labels_lr=x["labels_lr"],
                       labels_hr=x["labels_hr"])


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_forward_vs_reference(gold, name, mode):
    net = _net(name)
    net.train(mode == "train")
    x = _dev(fc.inputs())
    res_hr, error, res_lr = _forward(net, x)
    tag = "%s_%s_" % (name, mode)
    S = gold[tag + "pred_lr"].shape[0]
    assert S == (3 if mode == "train" else 1)
    # list lengths and aliases as in the reference
    assert len(net.intermediate_preds_list_lr) == S and len(net.intermediate_preds_list_hr) == S == len(net.im_feat_list_lr)
    assert net.preds_lr is net.intermediate_preds_list_lr[-1] and net.preds_hr is net.intermediate_preds_list_hr[-1]
    assert res_hr is net.preds_hr and res_lr is net.preds_lr
    assert net.labels_lr is x["labels_hr"] and net.labels_hr is x["labels_lr"]      # (SuRSNet.py:249-250)
    for s in range(S):
        for key, lst in (("pred_lr", net.intermediate_preds_list_lr), ("pred_hr", net.intermediate_preds_list_hr)):
            assert tuple(lst[s].shape) == (fc.B, 1, fc.N)
            got, ref = lst[s][:, 0].cpu().numpy(), gold[tag + key][s]
            d = float(np.abs(got - ref).max())
            print(tag, key, "stack", s, "max difference", d)
            assert d < 1e-4
            assert ((got == 0) == (ref == 0)).all()
    # the loss: a 0-dim float32 device tensor outside any autograd graph
    assert error.dim() == 0 and error.dtype == torch.float32 and error.is_cuda and error.grad_fn is None and not error.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        error.backward()
    sr_range = float(gold["img_sr"].max() - gold["img_sr"].min())
    bounds = np.array([2.1e-4, 2.1e-4, 1e-4 * sr_range, 8.1e-4])
    terms = net.loss_values.cpu().numpy().astype(np.float64)
    d = np.abs(terms - gold[tag + "terms"].astype(np.float64))
    dt = abs(float(error) - float(gold[tag + "total"]))
    print(tag, "terms", terms, "differences", d, "bounds", bounds, "total", float(error), "difference", dt,
          "bound", float(np.dot(fc.LOSS_WEIGHTS, bounds)))
    assert (d < bounds).all()
    assert dt < float(np.dot(fc.LOSS_WEIGHTS, bounds))
    # img_SR itself (what the SR term's bound rests on)
    assert float(np.abs(net.im_SR.cpu().numpy() - gold["img_sr"]).max()) < 1e-4 * sr_range
    # the four methods on their own: the same reduction, the same bits
    one = [net.get_error_lr(), net.get_error_hr(), net.get_errorSR(net.im_SR, x["images_hr"]), net.get_error_disp_1()]
    for i, t in enumerate(one):
        assert t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda
        assert torch.equal(t, net.loss_values[i]), i
    w = np.asarray(fc.LOSS_WEIGHTS, np.float32)
    assert float(error) == float(((w[0] * terms[0].astype(np.float32) + w[1] * np.float32(terms[1])) + w[2] * np.float32(terms[2]))
                                 + w[3] * np.float32(terms[3]))
    # forward twice: the same bits
    _, again, _ = _forward(net, x)
    assert torch.equal(again, error)


@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_train_mode_queries_return_every_stack(gold, name):
    """query_mr + query_sr on ONE point set in training mode (the fused both-classifier pass per stack): list lengths of the
    reference, every stack against the single-map query of a model that holds that map alone."""
    net, x = _encoded_train(name)
    cal = x["calibs"]
    net.query_mr(x["points_hr"], cal)
    net.query_sr(x["points_hr"], cal)
    assert len(net.intermediate_preds_list_lr) == 3 and len(net.intermediate_preds_list_hr) == 3
    assert net.get_preds()[0] is net.intermediate_preds_list_hr[-1] and net.get_preds()[1] is net.intermediate_preds_list_lr[-1]
    got_lr = [t.clone() for t in net.intermediate_preds_list_lr]
    got_hr = [t.clone() for t in net.intermediate_preds_list_hr]
    one = _net(name)
    one.eval()
    for s in range(3):
        one.im_feat_list_lr, one.im_feat_list_hr = [net.im_feat_list_lr[s]], net.im_feat_list_hr
        one.query_mr(x["points_hr"], cal)
        one.query_sr(x["points_hr"], cal)
        phr, plr = one.get_preds()
        assert torch.equal(plr, got_lr[s]) and torch.equal(phr, got_hr[s]), s
        # the lr predictions on points_hr are what the fixture's train-mode forward made there
        assert float(np.abs(plr[:, 0].cpu().numpy() - gold[name + "_train_pred_lr"][s]).max()) < 1e-4


@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_eval_mode_get_preds_keeps_its_bits(name):
    """One map: query_mr + query_sr + get_preds are the single-map entries' bits, as before."""
    from surs_amd import native
    net = _net(name)
    net.eval()
    x = _dev(fc.inputs())
    _, f_lr, f_hr = net.super_res(x["images_lr"])
    net.filter_lr(f_lr)
    net.filter_hr(f_hr)
    assert len(net.im_feat_list_lr) == 1
    net.query_mr(x["points_hr"], x["calibs"])
    net.query_sr(x["points_hr"], x["calibs"])
    phr, plr = net.get_preds()
    assert len(net.intermediate_preds_list_lr) == 1 and len(net.intermediate_preds_list_hr) == 1
    cal = common.CALIB.reshape(-1)[:12]
    for b in range(fc.B):
        fl, fh = net.features(b)
        pts = x["points_hr"][b].contiguous()
        if net.generic_mlp() is None:
            rh, rl = native.query_points(pts, cal, ZMUL, ZDIV, fl, fh, net._mlp_blob(), native.Workspace(pts.device))
        else:
            rh, rl = native.query_points_generic(pts, cal, ZMUL, ZDIV, fl, fh, net.generic_mlp())
        assert torch.equal(phr[b, 0], rh) and torch.equal(plr[b, 0], rl)


def test_forward_losses_deterministic_and_against_numpy():
    import gpu_common as g
    from surs_amd import native
    gen = torch.Generator().manual_seed(11)
    S, M, K = 3, 6001, 98307
    pl, ph = torch.rand((S, M), generator=gen).to(g.dev()), torch.rand((S, M), generator=gen).to(g.dev())
    ll, lh = (torch.rand(M, generator=gen) > 0.5).float().to(g.dev()), (torch.rand(M, generator=gen) > 0.5).float().to(g.dev())
    a, b = (torch.rand(K, generator=gen) * 2 - 1).to(g.dev()), (torch.rand(K, generator=gen) * 2 - 1).to(g.dev())
    w = (0.5, 2.0, 0.25, 1.5)
    run = lambda: native.forward_losses(pred_lr=pl, lab_lr=ll, pred_hr=ph, lab_hr=lh, img_sr=a, img_hr=b, weights=w)
    t1, e1 = run()
    t2, e2 = run()
    assert torch.equal(t1, t2) and torch.equal(e1, e2)
    n = lambda t: t.cpu().numpy().astype(np.float64)
    ref = np.array([np.mean((n(pl) - n(ll)) ** 2), np.mean((n(ph) - n(lh)) ** 2), np.mean(np.abs(n(a) - n(b))),
                    np.mean(((n(lh) - n(ll)) - (n(ph)[-1] - n(pl)[-1])) ** 2)])
    rel = np.abs(n(t1) - ref) / ref
    print("terms", n(t1), "relative differences", rel, "total", float(e1), "relative", abs(float(e1) - np.dot(w, ref)) / np.dot(w, ref))
    assert rel.max() < 1e-6
    assert abs(float(e1) - np.dot(w, ref)) / np.dot(w, ref) < 1e-6
    # a group left out: a zero term, the others' bits unchanged
    t3, none = native.forward_losses(pred_lr=pl, lab_lr=ll)
    assert none is None and torch.equal(t3[0], t1[0]) and float(t3[1]) == float(t3[2]) == float(t3[3]) == 0.0


@pytest.mark.parametrize("name", list(fc.SHAPES))
def test_forward_bf16(name):
    """--precision bf16: a finite loss; every stack's predictions are the bits of the single-map query of that precision."""
    net = _net(name, ["--precision", "bf16"])
    net.train()
    x = _dev(fc.inputs())
    _, error, _ = _forward(net, x)
    assert bool(torch.isfinite(error)) and bool(torch.isfinite(net.loss_values).all())
    assert len(net.intermediate_preds_list_lr) == 3 and len(net.intermediate_preds_list_hr) == 3
    got_lr = [t.clone() for t in net.intermediate_preds_list_lr]
    got_hr = [t.clone() for t in net.intermediate_preds_list_hr]
    one = _net(name, ["--precision", "bf16"])
    one.eval()
    fp32 = _net(name)
    fp32.train()
    _forward(fp32, x)
    for s in range(3):
        one.im_feat_list_lr, one.im_feat_list_hr = [net.im_feat_list_lr[s]], net.im_feat_list_hr
        one.query_mr(x["points_hr"], x["calibs"])
        one.query_sr(x["points_lr"], x["calibs"])
        phr, plr = one.get_preds()
        assert torch.equal(plr, got_lr[s]) and torch.equal(phr, got_hr[s]), s
        # ... and it is the reduced arithmetic, not the fp32-grade one
        assert not torch.equal(got_lr[s], fp32.intermediate_preds_list_lr[s])
    print(name, "bf16 loss", float(error), "fp32 loss", float(fp32.loss_values @ torch.tensor(fc.LOSS_WEIGHTS, device=error.device)))
