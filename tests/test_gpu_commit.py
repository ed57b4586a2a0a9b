"""GPU checks of SuRSNet.commit(): the forward after an in-place device repack of the packed weights equals, bit for bit, the forward
of a net that LOADED the same values (the host packers); state_dict() after a commit; partial commits; stable addresses; the wide
image; the other operand settings; a side stream; to()'s write-back; the refusals.  The `s1` options and the 64 x 64 images of
tests/forward_common.py."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import forward_common as fc

pytestmark = pytest.mark.gpu

_cache = {}


def _opt(more=()):
    from surs_amd import options
    return options.BaseOptions().parse(fc.flags("s1", more))


def _sd0(more=()):
    from surs_amd import weights
    key = ("sd0",) + tuple(more)
    if key not in _cache:
        _cache[key] = OrderedDict((k, torch.from_numpy(np.asarray(v)))
                                  for k, v in weights.synthetic_state_dict(_opt(more), seed=0).items())
    return _cache[key]


def _net(sd, more=()):
    import gpu_common as g
    from surs_amd import model
    net = model.SuRSNet(_opt(more)).to(device=g.dev())
    net.load_state_dict(sd)
    net.train()
    return net


def _x():
    import gpu_common as g
    if "x" not in _cache:
        _cache["x"] = {k: torch.from_numpy(v).to(g.dev()) for k, v in fc.inputs().items()}
    return _cache["x"]


def _forward(net):
    """forward() in training mode: everything the issue compares, as clones."""
    x = _x()
    res_hr, error, res_lr = net.forward(x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"],
                                        labels_lr=x["labels_lr"], labels_hr=x["labels_hr"])
    out = OrderedDict(img_SR=net.im_SR, hr=net.im_feat_list_hr[0], res_hr=res_hr, res_lr=res_lr, error=error)
    for i, t in enumerate(net.im_feat_list_lr):
        out["lr%d" % i] = t
    assert len(net.im_feat_list_lr) == 3
    return OrderedDict((k, v.detach().clone()) for k, v in out.items())


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k


def _masters(net, sets=("mlp", "sr", "hg")):
    out = OrderedDict()
    for s in sets:
        out.update(getattr(net, s + "_parameters")())
    return out


def _perturb(masters, seed=11):
    """A seeded perturbation added to every master IN PLACE: relative 2^-7 noise plus a small absolute one (zero biases move too)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in masters.values():
            n = torch.rand(p.shape, generator=gen) - 0.5
            p.add_((n * (2.0 ** -6)).to(p.device) * p.abs() + (n * 1e-3).to(p.device))


def _as_state_dict(sd0, masters):
    """sd0 with the masters' current values at their keys (the state dict's shapes)."""
    sd = OrderedDict(sd0)
    for k, p in masters.items():
        sd[k] = p.detach().cpu().reshape(sd0[k].shape).clone()
    return sd


def _encoder_tensors(W):
    out = OrderedDict()
    for name, cw in W.conv.items():
        out[name + "/w"] = cw.w
        if cw.w3 is not None:
            out[name + "/w3"] = cw.w3
        if cw.b is not None:
            out[name + "/b"] = cw.b
    for name, (gamma, beta) in W.gn.items():
        out[name + "/gamma"], out[name + "/beta"] = gamma, beta
    return out


@pytest.fixture(scope="module")
def committed():
    """Net A: loads sd0, runs a forward (everything packed), every master perturbed in place, commit(), forward.  Net B: loads the
    perturbed values.  Shared by the tests that only look."""
    sd0 = _sd0()
    net = _net(sd0)
    before = _forward(net)
    masters = _masters(net)
    W, native_net = net._enc, getattr(net._enc, "_native", None)
    assert native_net is not None     # (the library's own sequencing ran: its struct holds the raw pointers)
    ptrs = {k: t.data_ptr() for k, t in _encoder_tensors(W).items()}
    ptrs["blob"] = net._blob.data_ptr()
    _perturb(masters)
    net.commit()
    after = _forward(net)
    sd_b = _as_state_dict(sd0, masters)
    ref = _forward(_net(sd_b))
    return dict(net=net, sd0=sd0, sd_b=sd_b, before=before, after=after, ref=ref, masters=masters, ptrs=ptrs, W=W, native_net=native_net)


def test_commit_equals_reload(committed):
    _same(committed["after"], committed["ref"])
    for k in ("img_SR", "lr2", "hr", "res_hr", "error"):
        assert not torch.equal(committed["after"][k], committed["before"][k]), k     # (the perturbation reaches every output)


def test_stable_addresses(committed):
    net = committed["net"]
    assert net._enc is committed["W"] and net._enc._native is committed["native_net"]
    now = {k: t.data_ptr() for k, t in _encoder_tensors(net._enc).items()}
    now["blob"] = net._blob.data_ptr()
    assert now == committed["ptrs"]
    assert net.generic_mlp() is not None and net.generic_mlp().blob.data_ptr() == committed["ptrs"]["blob"]


def test_state_dict_after_commit(committed):
    net, sd0, masters = committed["net"], committed["sd0"], committed["masters"]
    sd = net.state_dict()
    assert list(sd) == [k for k, _, _ in net._spec] == list(sd0)
    for k, v in sd.items():
        want = masters[k].detach().cpu().reshape(sd0[k].shape) if k in masters else sd0[k]
        assert v.dtype == sd0[k].dtype and v.shape == sd0[k].shape and torch.equal(v, want), k
    assert any(not torch.equal(sd[k], sd0[k]) for k in masters)
    assert [tuple(p.shape) for p in net.parameters()] == [tuple(v.shape) for v in sd0.values()]


def test_two_adam_steps_on_the_classifiers():
    """forward_backward + commit against the load_state_dict route INTEGRATION.md used to end with: the same error bits after each step."""
    import gpu_common as g
    x = _x()
    args = (x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"])
    kw = dict(labels_lr=x["labels_lr"], labels_hr=x["labels_hr"])
    a, b = _net(_sd0()), _net(_sd0())
    params_a = a.mlp_parameters()
    opt_a = torch.optim.Adam(params_a.values(), lr=1e-3)
    sd = b.state_dict()
    params_b = {k: torch.nn.Parameter(sd[k].to(g.dev())) for k in sd if k.startswith("mlp_")}
    opt_b = torch.optim.Adam(params_b.values(), lr=1e-3)
    errors = []
    for step in range(2):
        _, err_a, _, grads = a.forward_backward(*args, **kw)
        for k, p in params_a.items():
            p.grad = grads[k].reshape(p.shape)
        opt_a.step()
        a.commit(("mlp",))
        _, err_b, _, grads = b.forward_backward(*args, **kw)
        for k, p in params_b.items():
            p.grad = grads[k]
        opt_b.step()
        sd.update({k: p.detach().cpu() for k, p in params_b.items()})
        b.load_state_dict(sd)
        assert torch.equal(err_a, err_b), step
        errors.append(float(err_a))
    err_a, err_b = a.forward(*args, **kw)[1], b.forward(*args, **kw)[1]
    assert torch.equal(err_a, err_b)
    assert float(err_a) != errors[0] and a.mlp_parameters() is params_a


def test_partial_commit_leaves_the_encoder_images():
    net = _net(_sd0())
    _forward(net)
    masters = _masters(net)
    _perturb(masters, seed=12)
    enc = _encoder_tensors(net._enc)
    kept = {k: t.clone() for k, t in enc.items()}
    blob = net._blob.clone()
    net.commit(("mlp",))
    for k, t in enc.items():
        assert torch.equal(t.view(torch.uint8), kept[k].view(torch.uint8)), k
    assert not torch.equal(net._blob, blob)
    sd = net.state_dict()
    assert all(torch.equal(sd[k], _sd0()[k]) for k in sd if not k.startswith("mlp_"))   # (uncommitted masters are not written back)


@pytest.mark.parametrize("wide_first", [True, False])
def test_wide_operands_after_a_commit(wide_first):
    """A 3x3 convolution inside wide_operands() after repack(): the wide image is refreshed where it existed and packed from the device
    master where it did not - never from the stale host copy."""
    import gpu_common as g
    from surs_amd import native
    rng = np.random.default_rng(3)
    w0, w1 = (rng.normal(0, 0.05, (48, 32, 3, 3)).astype(np.float32) for _ in range(2))
    b0, b1 = (rng.normal(0, 0.05, 48).astype(np.float32) for _ in range(2))
    x = native.Img.from_nchw(torch.from_numpy(rng.uniform(-1, 1, (1, 32, 24, 20)).astype(np.float32)).to(g.dev()))
    cw = native.ConvWeights(w0, b0, g.dev())
    if wide_first:
        with native.wide_operands():
            old = native.conv2d(x, cw).buf.clone()
        assert cw._w3_wide is not None
    ptr = (cw.w.data_ptr(), cw.w3.data_ptr(), cw.b.data_ptr(), cw._w3_wide.data_ptr() if wide_first else 0)
    cw.repack(torch.from_numpy(w1).to(g.dev()), torch.from_numpy(b1).to(g.dev()))
    fresh = native.ConvWeights(w1, b1, g.dev())
    with native.wide_operands():
        got, want = native.conv2d(x, cw).buf, native.conv2d(x, fresh).buf
    assert torch.equal(got, want) and (not wide_first or not torch.equal(got, old))
    assert torch.equal(cw._w3_wide, fresh._w3_wide) and torch.equal(cw.w3, fresh.w3) and torch.equal(cw.w, fresh.w)
    assert ptr == (cw.w.data_ptr(), cw.w3.data_ptr(), cw.b.data_ptr(), cw._w3_wide.data_ptr() if wide_first else 0)
    assert torch.equal(native.conv2d(x, cw).buf, native.conv2d(x, fresh).buf)


@pytest.fixture
def conv_split_bf16x3():
    from surs_amd import settings
    settings.set("SURS_CONV_SPLIT", "bf16x3")
    yield
    settings.set("SURS_CONV_SPLIT", None)


def _commit_against_fresh(more=()):
    sd0 = _sd0(more)
    net = _net(sd0, more)
    before = _forward(net)
    masters = _masters(net)
    _perturb(masters, seed=13)
    net.commit()
    after = _forward(net)
    _same(after, _forward(_net(_as_state_dict(sd0, masters), more)))
    assert not torch.equal(after["lr2"], before["lr2"])
    return net


def test_commit_with_three_bf16_parts(conv_split_bf16x3):
    net = _commit_against_fresh()
    assert all(cw.parts == 3 for cw in net._enc.conv.values())


def test_commit_with_encoder_precision_f16():
    net = _commit_against_fresh(("--encoder_precision", "f16"))
    assert net._enc.reduced


def test_commit_on_a_side_stream(committed):
    import gpu_common as g
    net = _net(committed["sd0"])
    _forward(net)
    masters = _masters(net)
    with torch.no_grad():
        for k, p in masters.items():
            p.copy_(committed["masters"][k])
    side, cur = torch.cuda.Stream(g.dev()), torch.cuda.current_stream(g.dev())
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        net.commit()
    cur.wait_stream(side)
    _same(_forward(net), committed["ref"])


def test_to_writes_the_committed_values_back():
    import gpu_common as g
    net = _net(_sd0())
    net._mlp_blob()
    masters = _masters(net, ("mlp", "sr"))
    _perturb(masters, seed=14)
    net.commit()
    want = {k: p.detach().cpu().reshape(_sd0()[k].shape).clone() for k, p in masters.items()}
    net.to(g.dev())
    assert not net._masters()
    sd = net.state_dict()
    for k, v in sd.items():
        assert torch.equal(v, want[k] if k in want else _sd0()[k]), k
    # and the masters made afterwards start from the committed values
    assert all(torch.equal(p.detach().cpu(), want[k].reshape(p.shape)) for k, p in net.mlp_parameters().items())


def test_partial_load_after_commit_keeps_the_committed_values():
    """load_state_dict(strict=False) of the classifiers alone after a commit of everything: the keys it does not name keep their
    COMMITTED values (they lived in device masters the load drops), in state_dict() and in the forward."""
    sd0 = _sd0()
    net = _net(sd0)
    _forward(net)
    masters = _masters(net)
    _perturb(masters, seed=16)
    net.commit()
    want = _as_state_dict(sd0, {k: p for k, p in masters.items() if not k.startswith("mlp_")})
    net.load_state_dict(OrderedDict((k, v) for k, v in sd0.items() if k.startswith("mlp_")), strict=False)
    assert net._stale == set() and not net._masters()
    sd = net.state_dict()
    for k, v in sd.items():
        assert torch.equal(v, want[k]), k
    assert any(not torch.equal(sd[k], sd0[k]) for k in masters if not k.startswith("mlp_"))
    _same(_forward(net), _forward(_net(want)))


def test_refresh_takes_in_a_wide_image_packed_after_the_first_commit():
    """wide_operands() after a commit packs the wide images from the device masters; the next commit makes its table again, once, with
    them in it - and the wide forward then equals a fresh net's."""
    from surs_amd import native
    sd0 = _sd0()
    net = _net(sd0)
    _forward(net)
    masters = _masters(net)
    _perturb(masters, seed=17)
    net.commit()
    W = net._enc
    (plan,) = W._refresh.values()
    assert len(plan[4]) > 0 and all(cw._w3_wide is None for cw in plan[4])
    with native.wide_operands():
        _forward(net)
    assert any(cw._w3_wide is not None for cw in plan[4])
    ptrs = {n: cw._w3_wide.data_ptr() for n, cw in W.conv.items() if cw._w3_wide is not None}
    _perturb(masters, seed=18)
    net.commit()
    (plan2,) = W._refresh.values()
    assert plan2 is not plan and all(cw._w3_wide is None for cw in plan2[4])
    net.commit()
    assert next(iter(W._refresh.values())) is plan2        # (made again once, not per call)
    assert ptrs == {n: cw._w3_wide.data_ptr() for n, cw in W.conv.items() if cw._w3_wide is not None}
    fresh = _net(_as_state_dict(sd0, masters))
    with native.wide_operands():
        _same(_forward(net), _forward(fresh))


def test_a_refused_refresh_changes_nothing():
    """EncoderWeights.refresh checks everything before it touches a convolution: after a refusal no ConvWeights has lost its host copy
    or taken a master."""
    net = _net(_sd0())
    _forward(net)
    sr = net.sr_parameters()
    bad = OrderedDict(sr)
    bad["image_filter_lr.bl0.weight"] = net.hg_parameters()["image_filter_lr.bl0.weight"]     # a stack joint without al and l
    with pytest.raises(ValueError, match="stack joint 0"):
        net._enc.refresh(bad)
    wrong = OrderedDict(sr)
    last = list(sr)[-2 if list(sr)[-1].endswith("bias") else -1]
    assert last.endswith(".weight")
    wrong[last] = sr[last].new_zeros((2, 2, 3, 3))                                             # not that convolution's shape
    with pytest.raises(ValueError, match="repack"):
        net._enc.refresh(wrong)
    assert all(cw._master is None and cw._host_w is not None for cw in net._enc.conv.values())
    assert net._enc._refresh == {}


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_commit_rewrites_the_released_blob(precision):
    """The released classifier shape: commit() rewrites the surs_mlp_pack blob in its own dtype, in place."""
    import common
    import gpu_common as g
    from surs_amd import model, native, options
    net = model.SuRSNet(options.BaseOptions().parse(common.FLAGS + ["--precision", precision])).to(device=g.dev())
    net.load_state_dict(common.state_dict())
    blob = net._mlp_blob()
    assert net.generic_mlp() is None
    ptr, old = blob.data_ptr(), blob.clone()
    masters = _masters(net, ("mlp",))
    _perturb(masters, seed=15)
    net.commit()
    sd = {k: p.detach().cpu().numpy() for k, p in masters.items()}
    want, core = native.pack_mlp(sd, precision, torch.device("cpu"))
    assert core == net._core_dtype and net._blob.data_ptr() == ptr and not torch.equal(net._blob, old)
    assert torch.equal(net._blob.cpu(), want)


def test_refusals():
    import gpu_common as g
    from surs_amd import model
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.SuRSNet(_opt()).commit()
    net = _net(_sd0())
    with pytest.raises(ValueError, match="unknown parameter set"):
        net.commit(("mlp", "encoder"))
    with pytest.raises(RuntimeError, match="nothing to commit"):
        net.commit(("sr",))
    assert net.commit() is net      # (no master exists: nothing to do)
    batch = model.SuRSNet(_opt(("--norm", "batch"))).to(device=g.dev())
    with pytest.raises(NotImplementedError, match="--norm group only"):
        batch.commit(("hg",))
