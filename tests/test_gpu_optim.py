"""GPU checks of the optimiser step: surs_optim_step against surs_optim_step_host BIT FOR BIT (both compile csrc/surs_optim_update.h) and
against torch.optim's float64 under the bound of tests/optim_common.py; the scalar path of misaligned items; many small items, a chunk
boundary, the grid cap's stride and an index beyond 2^31; equal bits at other addresses; optim.Optimizer on a net (the `s1` options and
64 x 64 images of tests/forward_common.py): step + commit against a net that loaded the stepped values, commit=False, the state round trip
with torch.optim.Adam in both directions, and the .grad route after loss.backward()."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import forward_common as fc
import optim_common as oc

pytestmark = pytest.mark.gpu

_cache = {}


def _dev():
    import gpu_common as g
    return g.dev()


def _up(a, off=0):
    """numpy -> device tensor; off = 1: a view 4 bytes beyond a 16-byte-aligned address."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.zeros(a.size + 4 + off, dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def _device_step(rows, hyper):
    """surs_optim_step over rows (p, g, s0, s1, s2) of device tensors (None: no such state): table built, checked and uploaded here."""
    from surs_amd import native
    items = native.optim_items([tuple(t.data_ptr() if t is not None else None for t in r) + (r[0].numel(),) for r in rows])
    native.optim_check(items, len(rows), hyper)
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(_dev())
    native.optim_step(table, len(rows), hyper)
    return table


def _hyper(kind, t, wd=0.0, momentum=0.0, lr=oc.LR, eps=oc.EPS):
    from surs_amd import native
    return native.optim_hyper(kind, t, lr, wd, momentum, oc.BETAS, eps, oc.ALPHA, first_step=t == 1)


def _rows(p0, names, off=0):
    p = [_up(x, off) for x in p0]
    st = [[_up(np.zeros_like(x), off) for x in p0] for _ in names]
    g = [_up(np.zeros_like(x), off) for x in p0]
    rows = [(p[i], g[i]) + tuple(s[i] for s in st) + (None,) * (3 - len(names)) for i in range(len(p0))]
    return p, g, st, rows


def _assert_bits(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert oc.same_bits(a.cpu().numpy(), b), (what, i)


@pytest.mark.parametrize("case,wd", [(c, wd) for c in oc.CASES for wd in oc.DECAYS])
def test_table_equals_the_host_entry_bit_for_bit(case, wd):
    """The table of tests/test_optim_host.py on the device: after each of the 5 steps p and every state tensor carry the host entry's
    bits; after the last the float64 bound holds on every tensor."""
    t = oc.table(case, wd)
    kind, momentum, names = t["kind"], t["momentum"], t["names"]
    p, g, st, rows = _rows(t["p0"], names)
    for s in range(oc.STEPS):
        for dst, src in zip(g, t["grads"][s]):
            dst.copy_(torch.from_numpy(src))
        _device_step(rows, _hyper(kind, s + 1, wd, momentum))
        _assert_bits(p, t["host"][s][0], "%s p step %d" % (case, s + 1))
        for n, tensors in zip(names, st):
            _assert_bits(tensors, t["host"][s][1][n], "%s %s step %d" % (case, n, s + 1))
    ours = ([x.cpu().numpy() for x in p], {n: [x.cpu().numpy() for x in tensors] for n, tensors in zip(names, st)})
    oc.check_step(ours, t["f64"][-1], t["f32"][-1], "%s wd=%g device step %d" % (case, wd, oc.STEPS))


@pytest.mark.parametrize("case", ["SGD", "AMSgrad", "RMSprop"])
def test_misaligned_items_take_the_scalar_path(case):
    """Every pointer of every item 4 bytes beyond 16-byte alignment: the bits of the aligned copy (and so of the host entry)."""
    t = oc.table(case, 1e-2)
    kind, momentum, names = t["kind"], t["momentum"], t["names"]
    p, g, st, rows = _rows(t["p0"], names, off=1)
    assert all(x.data_ptr() % 16 == 4 for r in rows for x in r if x is not None)
    for s in range(2):
        for dst, src in zip(g, t["grads"][s]):
            dst.copy_(torch.from_numpy(src))
        _device_step(rows, _hyper(kind, s + 1, 1e-2, momentum))
    _assert_bits(p, t["host"][1][0], case + " p")
    for n, tensors in zip(names, st):
        _assert_bits(tensors, t["host"][1][1][n], case + " " + n)


def _many():
    """600 items of one to seven elements, one of 70 000 (18 chunks: a chunk boundary inside an item) and one of 2049 chunks and three
    elements, which alone is more chunks than the grid has workgroups (2048): the stride."""
    if "many" not in _cache:
        rng = np.random.default_rng(7)
        sizes = [1 + i % 7 for i in range(600)]
        sizes[300:300] = [70000]
        sizes.append(2049 * 4096 + 3)
        p0 = [rng.normal(0, 1, n).astype(np.float32) for n in sizes]
        gs = [rng.normal(0, 1, n).astype(np.float32) for n in sizes]
        names = oc.state_names("AMSgrad", 0.0)
        st0 = [[(rng.uniform(0, 1, n) * (1e-3 if k else 1.0)).astype(np.float32) for n in sizes] for k, _ in enumerate(names)]
        from surs_amd import native
        p = [x.copy() for x in p0]
        st = [[x.copy() for x in s] for s in st0]
        h = _hyper("AMSgrad", 3, 1e-2)
        native.optim_step_host([(p[i], gs[i], st[0][i], st[1][i], st[2][i]) for i in range(len(p))], h)
        _cache["many"] = dict(sizes=sizes, p0=p0, gs=gs, st0=st0, p=p, st=st, h=h)
    return _cache["many"]


def _run_many(pad):
    m = _many()
    filler = torch.empty(pad, dtype=torch.uint8, device=_dev()) if pad else None    # (moves every later allocation)
    p = [_up(x) for x in m["p0"]]
    g = [_up(x) for x in m["gs"]]
    st = [[_up(x) for x in s] for s in m["st0"]]
    _device_step([(p[i], g[i], st[0][i], st[1][i], st[2][i]) for i in range(len(p))], m["h"])
    del filler
    return p, st


def test_many_small_items_a_chunk_boundary_and_the_grid_stride():
    m = _many()
    assert sum(-(-n // 4096) for n in m["sizes"]) > 2048
    p, st = _run_many(0)
    _assert_bits(p, m["p"], "p")
    for k in range(3):
        _assert_bits(st[k], m["st"][k], "state %d" % k)
    _cache["many_dev"] = (p, st)


def test_equal_inputs_at_other_addresses_give_equal_bits():
    first = _cache.get("many_dev") or _run_many(0)
    p, st = _run_many(12345 * 16 + 4096)
    assert {x.data_ptr() for x in p} != {x.data_ptr() for x in first[0]}
    for a, b in zip(p + [x for s in st for x in s], first[0] + [x for s in first[1] for x in s]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_an_item_beyond_two_to_the_31_elements():
    """SGD without momentum at lr = 1 on zeros: p = -g exactly.  Gradients planted at both ends, on both sides of element 2^31 and in
    the scalar tail; every other element must stay zero."""
    n = (1 << 31) + 4099
    p = torch.zeros(n, dtype=torch.float32, device=_dev())
    g = torch.zeros(n, dtype=torch.float32, device=_dev())
    where = [0, 5, (1 << 31) - 1, 1 << 31, (1 << 31) + 4095, n - 2, n - 1]
    vals = torch.arange(1, len(where) + 1, dtype=torch.float32, device=_dev())
    g[torch.tensor(where, device=_dev())] = vals
    _device_step([(p, g, None, None, None)], _hyper("SGD", 1, lr=1.0))
    assert torch.equal(p[torch.tensor(where, device=_dev())], -vals)
    assert int(torch.count_nonzero(p)) == len(where)


def test_the_kernel_entry_launches_nothing_it_refuses():
    from surs_amd import _lib, native
    p, g = _up(np.ones(8, np.float32)), _up(np.ones(8, np.float32))
    items = native.optim_items([(p.data_ptr(), g.data_ptr(), None, None, None, 8)])
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(_dev())
    with pytest.raises(_lib.SursError, match="kind 9"):
        native.optim_step(table, 1, native.optim_hyper(9, 1, 1e-2))
    with pytest.raises(_lib.SursError, match="misses a state tensor"):       # (the table's check, before any upload)
        native.optim_check(items, 1, native.optim_hyper("ADAM", 1, 1e-2))
    native.optim_step(table, 0, native.optim_hyper("SGD", 1, 1e-2))          # an empty table: nothing to do
    torch.cuda.synchronize()
    assert bool((p == 1).all())


# ------------------------------------------------------------------ optim.Optimizer on a net

def _opt():
    from surs_amd import options
    return options.BaseOptions().parse(fc.flags("s1"))


def _sd0():
    from surs_amd import weights
    if "sd0" not in _cache:
        _cache["sd0"] = OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in weights.synthetic_state_dict(_opt(), seed=0).items())
    return _cache["sd0"]


def _net(sd):
    from surs_amd import model
    net = model.SuRSNet(_opt()).to(device=_dev())
    net.load_state_dict(sd)
    net.train()
    return net


def _x():
    if "x" not in _cache:
        _cache["x"] = {k: torch.from_numpy(v).to(_dev()) for k, v in fc.inputs().items()}
    return _cache["x"]


def _args():
    x = _x()
    return (x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"]), dict(labels_lr=x["labels_lr"], labels_hr=x["labels_hr"])


def _forward(net):
    args, kw = _args()
    res_hr, error, res_lr = net.forward(*args, **kw)
    out = OrderedDict(img_SR=net.im_SR, hr=net.im_feat_list_hr[0], res_hr=res_hr, res_lr=res_lr, error=error)
    for i, t in enumerate(net.im_feat_list_lr):
        out["lr%d" % i] = t
    return OrderedDict((k, v.detach().clone()) for k, v in out.items())


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k


def _masters_of(net, sets):
    out = OrderedDict()
    for s in sets:
        out.update(getattr(net, s + "_parameters")())
    return out


def _cpu(tensors):
    return OrderedDict((k, t.detach().cpu().numpy().copy()) for k, t in tensors.items())


def _check_against_torch(kind, p0, grads_per_step, got, what, **hyper):
    """The bound on the parameters `got` (key -> array) after torch.optim's steps on the CPU over p0 with the given gradients."""
    keys = list(p0)
    gs = [[g[k].reshape(p0[k].shape) for k in keys] for g in grads_per_step]
    f64 = oc.run_torch(kind, [p0[k] for k in keys], gs, torch.float64, (), **hyper)[-1]
    f32 = oc.run_torch(kind, [p0[k] for k in keys], gs, torch.float32, (), **hyper)[-1]
    return oc.check_step(([got[k] for k in keys], {}), f64, f32, what)


def test_step_on_a_net_commits_what_it_stepped():
    """forward_backward, Optimizer(net).step(grads): the stepped masters within the bound of torch.optim's, every key without a
    gradient untouched, and the next forward bit for bit the forward of a net that load_state_dict-ed net.state_dict() - commit's
    contract, reached through step.  step(commit=False) then moves the masters and leaves the packed forward where it was."""
    from surs_amd import optim
    args, kw = _args()
    a = _net(_sd0())
    _, _, _, grads = a.forward_backward(*args, **kw)
    o = optim.Optimizer(a, "ADAM", lr=1e-3, weight_decay=1e-2)
    assert o.which == a.SETS and len(o._keys) == len(_masters_of(a, a.SETS))
    masters = _masters_of(a, a.SETS)
    before = _cpu(masters)
    assert o.step(grads) is None
    after = _cpu(masters)
    stepped = [k for k in before if k in grads]
    assert stepped == [k for k in before if k.startswith("mlp_")]
    _check_against_torch("ADAM", OrderedDict((k, before[k]) for k in stepped), [_cpu(grads)], after, "net ADAM", lr=1e-3, wd=1e-2)
    assert all(np.array_equal(before[k], after[k]) for k in before if k not in grads)
    assert all(not np.array_equal(before[k], after[k]) for k in stepped)
    # a second net under torch.optim itself, on the device, for the record
    b = _net(_sd0())
    pb = b.mlp_parameters()
    tb = oc.torch_optimizer("ADAM", list(pb.values()), lr=1e-3, wd=1e-2)
    for k, p in pb.items():
        p.grad = grads[k].reshape(p.shape)
    tb.step()
    print("largest |ours - torch.optim on the device|: %.3e" % max(float(np.abs(after[k] - pb[k].detach().cpu().numpy()).max()) for k in pb))
    # commit's contract through step()
    got = _forward(a)
    ref = _forward(_net(a.state_dict()))
    _same(got, ref)
    sd = a.state_dict()
    assert all(np.array_equal(sd[k].numpy().reshape(-1), after[k].reshape(-1)) for k in stepped)
    # commit=False: the masters move, the packed forward does not
    o.step(grads, commit=False)
    assert all(not np.array_equal(after[k], v) for k, v in _cpu(masters).items() if k in grads)
    _same(_forward(a), got)
    a.commit()
    assert not torch.equal(_forward(a)["res_hr"], got["res_hr"])


def test_step_refuses_before_it_writes():
    from surs_amd import optim
    a = _net(_sd0())
    o = optim.Optimizer(a, "SGD", which=("mlp",), lr=1e-2)
    params = a.mlp_parameters()
    keys = list(params)
    good = OrderedDict((k, torch.ones(p.numel(), device=_dev())) for k, p in params.items())
    before = _cpu(params)
    for bad in (torch.ones(params[keys[-1]].numel() + 1, device=_dev()), torch.ones(params[keys[-1]].numel(), device=_dev(), dtype=torch.float64),
                torch.ones(params[keys[-1]].numel())):
        with pytest.raises(ValueError, match="gradient of " + keys[-1]):
            o.step(OrderedDict(good, **{keys[-1]: bad}))
    torch.cuda.synchronize()
    assert all(np.array_equal(before[k], v) for k, v in _cpu(params).items()) and o._t == 0
    assert o.step({}) is None and o._t == 0                       # nothing has a gradient: nothing happens
    o.step(good)                                                  # ([out,in] masters, flat gradients: any shape with the element count)
    assert o._t == 1 and all(not np.array_equal(before[k], v) for k, v in _cpu(params).items())
    table = o._table
    o.step(good)
    assert o._table is table                                      # the same pointers: the table is not rebuilt
    o.step(OrderedDict((k, v.clone()) for k, v in good.items()))
    assert o._table is not table
    a.load_state_dict(_sd0())
    with pytest.raises(RuntimeError, match="masters were replaced"):
        o.step(good)


def _synthetic_grads(params, step):
    gen = torch.Generator().manual_seed(100 + step)
    return OrderedDict((k, torch.randn(p.shape, generator=gen).to(_dev())) for k, p in params.items())


def test_state_round_trip_with_torch_adam():
    """Three steps of torch.optim.Adam, its state_dict() loaded here, two more steps: against five torch steps under the bound.  Then
    three steps here, state_dict() loaded into torch.optim.Adam, two steps there."""
    from surs_amd import optim
    hyper = dict(lr=1e-3, wd=1e-2)
    net = _net(_sd0())
    for direction in ("torch -> here", "here -> torch"):
        net.load_state_dict(_sd0())
        params = net.mlp_parameters()
        p0 = _cpu(params)
        gs = [_synthetic_grads(params, s) for s in range(5)]
        t = oc.torch_optimizer("ADAM", list(params.values()), **hyper)
        o = optim.Optimizer(net, "ADAM", which=("mlp",), lr=hyper["lr"], weight_decay=hyper["wd"])

        def torch_step(g):
            for k, p in params.items():
                p.grad = g[k]
            t.step()

        if direction == "torch -> here":
            for s in range(3):
                torch_step(gs[s])
            o.load_state_dict(t.state_dict())
            assert o._t == 3
            for s in range(3, 5):
                o.step(gs[s], commit=False)
        else:
            for s in range(3):
                o.step(gs[s], commit=False)
            t.load_state_dict(o.state_dict())
            for s in range(3, 5):
                torch_step(gs[s])
        _check_against_torch("ADAM", p0, [_cpu(g) for g in gs], _cpu(params), "round trip " + direction, **hyper)


def test_the_grad_route_after_loss_backward():
    """INTEGRATION.md's whole-encoder example: loss.backward() through autograd.point_loss leaves .grad on sr_parameters() and
    hg_parameters(); the classifiers' come from last_classifier_grads; step() with grads=None reads them all; zero_grad() clears them."""
    import torch.nn.functional as F
    from surs_amd import autograd, optim
    x = _x()
    net = _net(_sd0())
    o = optim.Optimizer(net, "RMSprop", lr=1e-5)      # (RMSprop's first step moves every element by about 10 lr)
    masters = _masters_of(net, net.SETS)
    img_SR, feature_lr, feat_hr = autograd.super_res_features(net, x["images_lr"])
    loss = autograd.point_loss(net, autograd.filter_lr(net, feature_lr), feat_hr, x["points_hr"], x["points_lr"], x["calibs"],
                               x["labels_hr"], x["labels_lr"]) + net.opt.srweight * F.l1_loss(img_SR, x["images_hr"])
    o.zero_grad()
    loss.backward()
    for k, p in net.mlp_parameters().items():
        p.grad = net.last_classifier_grads[k].reshape(p.shape)
    with_grad = [k for k, p in masters.items() if p.grad is not None]
    assert set(net.mlp_parameters()) <= set(with_grad) and any(k.startswith("super_resolution.") for k in with_grad) \
        and any(k.startswith("image_filter_lr.") for k in with_grad)
    before = _cpu(masters)
    grads = OrderedDict((k, masters[k].grad.detach().cpu().numpy().copy()) for k in with_grad)
    o.step()
    after = _cpu(masters)
    _check_against_torch("RMSprop", OrderedDict((k, before[k]) for k in with_grad), [grads], after, "grad route RMSprop", lr=1e-5)
    assert all(np.array_equal(before[k], after[k]) for k in before if k not in grads)
    _same(_forward(net), _forward(_net(net.state_dict())))
    o.zero_grad()
    assert all(p.grad is None for p in masters.values())
