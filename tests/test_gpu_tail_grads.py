"""GPU checks of the stack-tail and whole-filter gradients: the fused joint kernel of csrc/surs_tail_grad.hip against torch-CPU float64
and against the three-call chain of surs_conv_grad_input it replaces; the tail module (SuRSNet.stack_tail_train / stack_tail_backward)
against the reference's own float64 gradients on kink-safe inputs (tests/golden/tail_grads_*.npz, tools/gen_golden_tail_grads.py,
tests/tail_grad_common.py); the whole filter (filter_lr_train / filter_lr_backward) bit for bit against the inference forward and
against the chain of the module calls; the autograd hand-off; one optimiser step through commit().

Bounds, in the metric  max |t - t64| / max |t64|  per tensor.  The joint kernel: e <= 4 max(e_chain, 2^-20) with e_chain the same
quantity for the chain on the same inputs (a factor 2 for one accumulator summing 256 + D terms where the chain rounds two sums
separately, times 2 for seed spread).  The module, per stored quantity: 8 max(e_ref, 2^-20) (sr_grad_common.compare's rule).  Every
parity test prints its worst ratio before it asserts."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import tail_grad_common as tg
from surs_amd import prng

pytestmark = pytest.mark.gpu

JOINT_FLOOR = 2.0 ** -20
SENTINEL = 12345.0


def _dev():
    import gpu_common as g
    return g.dev()


def _u(tag, seed, shape, lo=-1.0, hi=1.0):
    return prng.uniform("tail_grad_prim_" + tag, seed, shape, lo, hi)


# ------------------------------------------------------------------ 1. the fused kernel
# (pixels, D, G_out present, G_next present); 1056 = 33 x 32: sixteen whole 64-pixel tiles and a ragged one (thirty-three 32-pixel
# tiles at D = 384: the other instantiation); 35: below one tile.  D = 48, 1: ragged column blocks and k steps.
JOINT_CASES = [
    (1056, 256, True, True), (1056, 128, True, True), (1056, 48, True, True), (1056, 1, True, True),
    (35, 256, True, True), (35, 48, True, True), (35, 1, True, True), (35, 128, True, True),
    (1056, 256, True, False), (35, 48, True, False),        # G_next absent: the last stack's case
    (1056, 256, False, True), (35, 48, False, True),        # G_out absent
    (97, 384, True, True),                                  # D > 256: 32-pixel tiles
]
_joint_ref = {}


def _joint_inputs(p, D):
    """Seeded inputs and the float64 results, once per (p, D): weights of the tail's magnitude are not needed here - nothing has a kink."""
    key = (p, D)
    if key not in _joint_ref:
        r = dict(g_out=_u("go", p + D, (p, D)), g_next=_u("gn", p + D + 1, (p, 256)), w_al=_u("al", D, (256, D), -0.1, 0.1),
                 w_l=_u("l", D + 1, (D, 256), -0.1, 0.1), w_bl=_u("bl", D + 2, (256, 256), -0.1, 0.1))
        _joint_ref[key] = r
    return _joint_ref[key]


def _f64(r, has_out, has_next):
    d = lambda a: a.astype(np.float64)
    dout = (d(r["g_out"]) if has_out else 0.0) + (d(r["g_next"]) @ d(r["w_al"]) if has_next else 0.0)
    da = dout @ d(r["w_l"]) + (d(r["g_next"]) @ d(r["w_bl"]) if has_next else 0.0)
    return dout, da


def _rows(a, ld):
    """numpy [p][c] -> native.Img [1,p,c] with channel pitch ld, SENTINEL behind every row, and the fenced buffer it lives in."""
    from surs_amd import native
    p, c = a.shape
    buf = torch.full((64 + p * ld + 64,), SENTINEL, dtype=torch.float32)
    buf[64:64 + p * ld].reshape(p, ld)[:, :c] = torch.from_numpy(a)
    buf = buf.to(_dev())
    return native.Img(1, p, c, ld, buf, off=64), buf


def _out(p, c, ld):
    from surs_amd import native
    buf = torch.full((64 + p * ld + 64,), SENTINEL, dtype=torch.float32, device=_dev())
    return native.Img(1, p, c, ld, buf, off=64), buf


def _read(img, buf):
    """(the Img's values [p][c] as numpy, True where everything else of the buffer still holds SENTINEL)."""
    t = buf.cpu()
    body = t[64:64 + img.w * img.ld].reshape(img.w, img.ld)
    clean = bool((t[:64] == SENTINEL).all()) and bool((t[64 + img.w * img.ld:] == SENTINEL).all()) and bool((body[:, img.c:] == SENTINEL).all())
    return body[:, :img.c].numpy().copy(), clean


def _err(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) / float(np.abs(ref).max())


@pytest.mark.parametrize("p,D,has_out,has_next", JOINT_CASES)
def test_joint_kernel_against_float64_and_the_chain(p, D, has_out, has_next):
    from surs_amd import native
    r = _joint_inputs(p, D)
    ref_out, ref_a = _f64(r, has_out, has_next)
    dev = _dev()
    w = {k: torch.from_numpy(r[k]).to(dev) for k in ("w_al", "w_l", "w_bl")}
    w4 = dict(w_al=w["w_al"].reshape(256, D, 1, 1), w_l=w["w_l"].reshape(D, 256, 1, 1), w_bl=w["w_bl"].reshape(256, 256, 1, 1))
    runs = []
    for rep, (ld_o, ld_n, ld_do, ld_da) in enumerate(((D + 3, 260, D + 5, 264), (D, 256, D + 1, 256))):   # pitches above the channel count
        go, go_buf = _rows(r["g_out"], ld_o) if has_out else (None, None)
        gn, gn_buf = _rows(r["g_next"], ld_n) if has_next else (None, None)
        d_out, do_buf = _out(p, D, ld_do)
        d_a, da_buf = _out(p, 256, ld_da)
        native.tail_joint_grad(go, gn, w4["w_al"], w4["w_l"], w4["w_bl"], d_out=d_out, d_a=d_a)
        got_out, clean_out = _read(d_out, do_buf)
        got_a, clean_a = _read(d_a, da_buf)
        assert clean_out and clean_a, "a sentinel behind a row or a buffer was overwritten"
        for t, b in ((go, go_buf), (gn, gn_buf)):
            if t is not None:
                back, clean = _read(t, b)
                assert clean and np.array_equal(back, r["g_out"] if t is go else r["g_next"])
        runs.append((got_out, got_a))
    # two calls, buffers at other addresses and pitches: the same bits
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    got_out, got_a = runs[0]
    assert np.isfinite(got_out).all() and np.isfinite(got_a).all()
    if not has_next:
        assert np.array_equal(got_out, r["g_out"])             # dOut = G_out, a copy
    # the chain: three surs_conv_grad_input calls (k = 1), the second and third adding into their target
    go, _ = _rows(r["g_out"], D) if has_out else (None, None)
    gn, _ = _rows(r["g_next"], 256) if has_next else (None, None)
    c_out = native.Img(1, p, D, D, go.buf[64:64 + p * D].clone()) if has_out else None
    if has_next:
        c_out = native.conv_grad_input(gn, w4["w_al"], 1, p, dx=c_out, add=has_out)
    c_a = native.conv_grad_input(c_out, w4["w_l"], 1, p)
    if has_next:
        native.conv_grad_input(gn, w4["w_bl"], 1, p, dx=c_a, add=True)
    chain_out, chain_a = c_out.buf.reshape(p, D).cpu().numpy(), c_a.buf.reshape(p, 256).cpu().numpy()
    worst = 0.0
    for name, got, chain, ref in (("dOut", got_out, chain_out, ref_out), ("dA", got_a, chain_a, ref_a)):
        e, e_chain = _err(got, ref), _err(chain, ref)
        bound = 4.0 * max(e_chain, JOINT_FLOOR)
        worst = max(worst, e / bound)
        print("joint p=%d D=%d out=%d next=%d %s: e %.3g, chain %.3g, e / bound %.3f" % (p, D, has_out, has_next, name, e, e_chain, e / bound))
        assert e <= bound, (name, e, e_chain)
    print("joint p=%d D=%d out=%d next=%d: worst e / (4 max(e_chain, 2^-20)) = %.3f" % (p, D, has_out, has_next, worst))


# ------------------------------------------------------------------ 2. the module against the reference
_cases = {}


class _Case:
    def __init__(self, golden_dir, name):
        from surs_amd import model
        self.name, self.stack, self.last = name, tg.stack(name), tg.is_last(name)
        self.gold = tg.load_fixture(golden_dir, name)
        self.opt = tg.opt(name)
        self.net = model.SuRSNet(self.opt).to(device=_dev())
        self.net.load_state_dict(tg.state_dict(name))
        T = lambda a: None if a is None else torch.from_numpy(a).to(_dev())
        self.ll = T(tg.inputs(name, int(self.gold["seed"])))
        self.prev = T(tg.previous(name))
        self.g_out, self.g_next = [T(a) for a in tg.upstream(name)]


def _case(golden_dir, name):
    if name not in _cases:
        _cases[name] = _Case(golden_dir, name)
    return _cases[name]


def _check(c, grads, d_ll, d_prev, tag=""):
    assert sorted(grads) == sorted(tg.param_keys(c.name))
    sd = tg.state_dict(c.name)
    for k, v in grads.items():
        assert tuple(v.shape) == tuple(sd[k].shape) and v.dtype == torch.float32 and v.is_cuda, k
    both = OrderedDict((k, grads[k].detach().cpu().numpy()) for k in tg.param_keys(c.name))
    both[tg.INPUT_KEY] = d_ll.detach().cpu().numpy()
    if not c.last:
        both[tg.PREVIOUS_KEY] = d_prev.detach().cpu().numpy()
    rows = tg.compare(c.gold, both)
    name, ratio = tg.worst(rows)
    print("%s%s: %d quantities, worst deviation / bound = %.3f at %s; worst deviation / max(e_ref, 2^-20) = %.3f (bound 8)"
          % (c.name, tag, len(rows), ratio, name, max(d / (b / 8.0) for _, d, b in rows)))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", list(tg.CASES))
def test_module_parity_with_the_reference(golden_dir, name):
    from surs_amd import native
    c = _case(golden_dir, name)
    out, nxt = c.net.stack_tail_train(c.stack, c.ll, c.prev)
    assert tuple(out.shape) == tuple(tg.shapes(name)[1]) and (nxt is None) == c.last
    d_ll, d_prev, grads = c.net.stack_tail_backward(c.stack, c.g_out, c.g_next)
    assert list(grads) == native.hg_tail_keys(c.stack, c.opt.num_stack_lr)
    if c.last:
        assert d_prev is None
    else:
        assert torch.equal(d_prev, c.g_next)                    # d previous is grad_next itself, bit for bit
    _check(c, grads, d_ll, d_prev, tag=" model")
    # the same bits again
    d_ll2, _, grads2 = c.net.stack_tail_backward(c.stack, c.g_out, c.g_next)
    assert torch.equal(d_ll, d_ll2) and all(torch.equal(grads[k], grads2[k]) and grads[k].data_ptr() != grads2[k].data_ptr() for k in grads)


def test_tail_forward_is_the_inference_tail(golden_dir):
    """stack_tail_train's out and next on (ll, previous) equal the host mirror's launches on the same maps: conv_last leaving bn_end's
    statistics, l, and the merged next with the residual."""
    from surs_amd import native
    from surs_amd.model import _as_img, _as_nchw_view
    c = _case(golden_dir, "joint57")
    out, nxt = c.net.stack_tail_train(0, c.ll, c.prev)
    W = c.net._encoder_weights()
    for b in range(c.ll.shape[0]):
        t = native.conv2d_gn(_as_img(c.ll[b:b + 1]), W.conv[tg.P + "conv_last0"], want_stats=True)
        o = native.conv2d_gn(t, W.conv[tg.P + "l0"], gn=W.gn[tg.P + "bn_end0"])
        n = native.conv2d_gn(t, W.conv[tg.P + "next0"], gn=W.gn[tg.P + "bn_end0"], residual=_as_img(c.prev[b:b + 1]), want_stats=True)
        assert torch.equal(out[b:b + 1], _as_nchw_view(o)) and torch.equal(nxt[b:b + 1], _as_nchw_view(n)), b
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(nxt).all())


def test_missing_gradients_are_zeros(golden_dir):
    """grad_out alone: bl and al get exact zeros and previous no gradient; grad_next alone: previous gets grad_next itself."""
    c = _case(golden_dir, "joint57")
    c.net.stack_tail_train(0, c.ll, c.prev)
    d_o, p_o, g_o = c.net.stack_tail_backward(0, c.g_out, None)
    d_n, p_n, g_n = c.net.stack_tail_backward(0, None, c.g_next)
    assert p_o is None and torch.equal(p_n, c.g_next)
    for k in g_o:
        zero = ".bl0." in k or ".al0." in k
        assert (float(g_o[k].abs().max()) == 0.0) == zero, k
        assert float(g_n[k].abs().max()) > 0.0 and bool(torch.isfinite(g_n[k]).all()), k
    assert float(d_o.abs().max()) > 0.0 and float(d_n.abs().max()) > 0.0


# ------------------------------------------------------------------ 3. / 4. the whole filter
FILTER_CASES = OrderedDict([
    ("s2d1", (["--num_stack_lr", "2", "--hg_depth", "1"], (8, 8), 2, (0,))),       # flags, map, B, stacks with a gradient
    ("s3d2", (["--num_stack_lr", "3", "--hg_depth", "2"], (8, 12), 1, (0, 2))),
])
_filters = {}


class _Filter:
    def __init__(self, name):
        import common
        from surs_amd import model, options, weights
        fl, (h, w), B, with_g = FILTER_CASES[name]
        self.opt = options.BaseOptions().parse(common.FLAGS + fl)
        self.sd = weights.synthetic_state_dict(self.opt, seed=0)
        self.net = model.SuRSNet(self.opt).to(device=_dev())
        self.net.load_state_dict(self.sd)
        S = self.opt.num_stack_lr
        self.x = torch.from_numpy(_u("flt_x_" + name, 1, (B, 256, h, w))).to(_dev())
        self.G = [torch.from_numpy(_u("flt_G_%s_%d" % (name, s), 2 + s, (B, self.opt.hg_dim, h, w))).to(_dev()) if s in with_g else None
                  for s in range(S)]
        self.outs = self.net.filter_lr_train(self.x)
        self.dx, self.grads = self.net.filter_lr_backward(self.G)


def _filter(name):
    if name not in _filters:
        _filters[name] = _Filter(name)
    return _filters[name]


def test_train_forward_is_the_inference_forward():
    """filter_lr_train(x) against encoder.filter_lr - the host mirror's sequencing: ONE stream (SURS_ENC_STREAMS = 0), a ConvBlock's sum as
    a launch of its own, statistics handed from kernel to kernel - and against surs_encoder_filter_lr, which at 8 x 8 takes the same
    separate-sum form (the sum inside the convolutions needs whole 8 x 32 tiles).  Every stack's output, bit for bit."""
    from surs_amd import encoder, settings
    from surs_amd.model import _as_img, _as_nchw_view
    f = _filter("s2d1")
    W = f.net._encoder_weights()
    settings.set("SURS_ENC_STREAMS", "0")
    try:
        for b in range(f.x.shape[0]):
            x = _as_img(f.x[b:b + 1])
            for tag, outs in (("mirror", encoder.filter_lr(W, x, keep_all=True)), ("library", encoder.filter_lr_native(W, x, keep_all=True))):
                assert len(outs) == len(f.outs)
                for s, o in enumerate(outs):
                    assert torch.equal(f.outs[s][b:b + 1], _as_nchw_view(o)), (tag, b, s)
    finally:
        settings.set("SURS_ENC_STREAMS", None)
    assert all(bool(torch.isfinite(o).all()) and float(o.abs().max()) > 0 for o in f.outs)


def _chain(f):
    """The filter as the Python chain of the pinned module calls, walked in reverse; the two-term sums as fp32 +."""
    net, S = f.net, f.opt.num_stack_lr
    prev = [net.conv_block_train("conv2", f.x)]
    outs = []
    for s in range(S):
        ll = net.conv_block_train("top_m_%d" % s, net.hourglass_train(s, prev[s]))
        out, nxt = net.stack_tail_train(s, ll, prev[s] if s < S - 1 else None)
        outs.append(out)
        prev.append(nxt)
    grads, g_next = OrderedDict(), None
    for s in range(S - 1, -1, -1):
        if f.G[s] is None and g_next is None:
            continue
        d_ll, d_prev, g = net.stack_tail_backward(s, f.G[s], g_next)
        grads.update(g)
        d_hg, g = net.conv_block_backward("top_m_%d" % s, d_ll)
        grads.update(g)
        d_in, g = net.hourglass_backward(s, d_hg)
        grads.update(g)
        g_next = d_in if d_prev is None else d_in + d_prev
    dx, g = net.conv_block_backward("conv2", g_next)
    grads.update(g)
    return outs, dx, grads


@pytest.mark.parametrize("name", list(FILTER_CASES))
def test_whole_filter_equals_the_chain_of_modules(name):
    f = _filter(name)
    outs, dx, grads = _chain(f)
    for s, o in enumerate(outs):
        assert torch.equal(o, f.outs[s]), s
    assert torch.equal(dx, f.dx)
    keys = list(f.net.hg_parameters())
    assert list(f.grads) == keys
    reached = 0
    for k in keys:
        if k in grads:
            assert torch.equal(f.grads[k], grads[k]), k
            reached += 1
        else:   # a stack no gradient reaches (its G is None and so is everything behind it)
            assert float(f.grads[k].abs().max()) == 0.0, k
    assert reached > 0 and (reached < len(keys)) == (f.G[-1] is None)
    # a second call: the same bits in other buffers
    dx2, grads2 = f.net.filter_lr_backward(f.G)
    assert torch.equal(dx2, f.dx) and all(torch.equal(grads2[k], f.grads[k]) and grads2[k].data_ptr() != f.grads[k].data_ptr() for k in keys)


# ------------------------------------------------------------------ 5. the autograd hand-off
def test_autograd_filter_lr_and_stack_tail(golden_dir):
    from surs_amd import autograd
    f = _filter("s2d1")
    net, p = f.net, f.net.hg_parameters()
    x = f.x.clone().requires_grad_()
    outs = autograd.filter_lr(net, x)
    assert all(o.grad_fn is not None and torch.equal(o, w) for o, w in zip(outs, f.outs))
    L = sum((g * o).sum() for g, o in zip(f.G, outs) if g is not None)
    others = [v for k, v in net.sr_parameters().items()][:2]
    keys = list(p)
    got = torch.autograd.grad(L, [x] + [p[k] for k in keys] + others, allow_unused=True)
    assert torch.equal(got[0], f.dx)
    for k, g in zip(keys, got[1:1 + len(keys)]):
        assert torch.equal(g, f.grads[k]), k
    assert all(g is None for g in got[1 + len(keys):])          # parameters outside image_filter_lr.* get no gradient
    # the tail alone
    c = _case(golden_dir, "joint57")
    c.net.stack_tail_train(0, c.ll, c.prev)
    d_ll, d_prev, want = c.net.stack_tail_backward(0, c.g_out, c.g_next)
    ll, prev = c.ll.clone().requires_grad_(), c.prev.clone().requires_grad_()
    out, nxt = autograd.stack_tail(c.net, 0, ll, prev)
    cp = c.net.hg_parameters()
    got = torch.autograd.grad((c.g_out * out).sum() + (c.g_next * nxt).sum(), [ll, prev] + [cp[k] for k in want])
    assert torch.equal(got[0], d_ll) and torch.equal(got[1], d_prev)
    assert all(torch.equal(g, want[k]) for k, g in zip(want, got[2:]))
    untouched = [k for k in cp if k not in want]
    got = torch.autograd.grad((c.g_out * autograd.stack_tail(c.net, 0, ll, prev)[0]).sum(), [cp[k] for k in untouched[:4]], allow_unused=True)
    assert all(g is None for g in got)


def _same_grads(got, want):
    assert list(got) == list(want)
    for k in got:
        assert torch.equal(got[k], want[k]), k


def test_autograd_backward_leaves_the_models_tape_alone(golden_dir):
    """The Functions own the tapes of their forwards: a backward run after the model's *_train() on ONE other image has filed its own
    latest tape gives the first forward's gradients, and the model's *_backward() then gives what it gives on a fresh net after that
    *_train() alone - the model's tape, its key and its image count are as the train call left them."""
    from surs_amd import autograd, model
    # the stack tail
    c = _case(golden_dir, "joint57")
    net, p = c.net, c.net.hg_parameters()
    net.stack_tail_train(0, c.ll, c.prev)
    d_ll, d_prev, want = net.stack_tail_backward(0, c.g_out, c.g_next)
    ll, prev = c.ll.clone().requires_grad_(), c.prev.clone().requires_grad_()
    out, nxt = autograd.stack_tail(net, 0, ll, prev)
    net.stack_tail_train(0, c.ll[:1] * 0.5, c.prev[:1])
    kept, filed = net._tapes[("tail", 0)], set(net._tapes)
    got = torch.autograd.grad((c.g_out * out).sum() + (c.g_next * nxt).sum(), [ll, prev] + [p[k] for k in want])
    assert torch.equal(got[0], d_ll) and torch.equal(got[1], d_prev)
    assert all(torch.equal(g, want[k]) for k, g in zip(want, got[2:]))
    assert net._tapes[("tail", 0)] is kept and len(kept[2]) == 1 and set(net._tapes) == filed
    one, _, grads = net.stack_tail_backward(0, c.g_out[:1], c.g_next[:1])
    fresh = model.SuRSNet(c.opt).to(device=_dev())
    fresh.load_state_dict(tg.state_dict("joint57"))
    fresh.stack_tail_train(0, c.ll[:1] * 0.5, c.prev[:1])
    fresh_one, _, fresh_grads = fresh.stack_tail_backward(0, c.g_out[:1], c.g_next[:1])
    assert torch.equal(one, fresh_one)
    _same_grads(grads, fresh_grads)
    # the whole filter
    f = _filter("s2d1")
    net, p = f.net, f.net.hg_parameters()
    G1 = [None if g is None else g[:1] for g in f.G]
    x = f.x.clone().requires_grad_()
    outs = autograd.filter_lr(net, x)
    net.filter_lr_train(f.x[:1] * 0.5)
    kept, filed = net._tapes["filter_lr"], set(net._tapes)
    got = torch.autograd.grad(sum((g * o).sum() for g, o in zip(f.G, outs) if g is not None), [x] + list(p.values()))
    assert torch.equal(got[0], f.dx)
    assert all(torch.equal(g, f.grads[k]) for k, g in zip(p, got[1:]))
    assert net._tapes["filter_lr"] is kept and len(kept[2]) == 1 and set(net._tapes) == filed
    one, grads = net.filter_lr_backward(G1)
    fresh = model.SuRSNet(f.opt).to(device=_dev())
    fresh.load_state_dict(f.sd)
    fresh.filter_lr_train(f.x[:1] * 0.5)
    fresh_one, fresh_grads = fresh.filter_lr_backward(G1)
    assert torch.equal(one, fresh_one)
    _same_grads(grads, fresh_grads)
    net.filter_lr_train(f.x)     # (the shared case's own tape again, for the tests that go back through it)


def test_explicit_tapes_serve_their_own_forward(golden_dir):
    """stack_tail_backward(tapes=) and filter_lr_backward(tapes=): the tapes of a first forward, passed after the same module ran on
    another input, give the first forward's backward bit for bit, and the model's own entry is neither used nor changed."""
    c = _case(golden_dir, "joint57")
    net = c.net
    net.stack_tail_train(0, c.ll, c.prev)
    first = net._tapes[("tail", 0)]
    d_ll, d_prev, want = net.stack_tail_backward(0, c.g_out, c.g_next)
    net.stack_tail_train(0, c.ll[:1] * 0.5, c.prev[:1])
    latest = net._tapes[("tail", 0)]
    assert latest is not first and len(first[2]) == c.ll.shape[0] and len(latest[2]) == 1
    got_ll, got_prev, grads = net.stack_tail_backward(0, c.g_out, c.g_next, tapes=first)
    assert torch.equal(got_ll, d_ll) and torch.equal(got_prev, d_prev)
    _same_grads(grads, want)
    assert net._tapes[("tail", 0)] is latest
    f = _filter("s2d1")
    net = f.net
    net.filter_lr_train(f.x)
    first = net._tapes["filter_lr"]
    net.filter_lr_train(f.x[:1] * 0.5)
    latest = net._tapes["filter_lr"]
    assert latest is not first and len(first[2]) == f.x.shape[0] and len(latest[2]) == 1
    dx, grads = net.filter_lr_backward(f.G, tapes=first)
    assert torch.equal(dx, f.dx)
    _same_grads(grads, f.grads)
    assert net._tapes["filter_lr"] is latest
    net.filter_lr_train(f.x)     # (the shared case's own tape again)


# ------------------------------------------------------------------ 6. train, commit, agree
def test_step_commit_and_a_fresh_net_agree():
    """One SGD step on hg_parameters() from filter_lr_backward's gradients, commit(): filter_lr_train then equals a fresh net loaded from
    the stepped state_dict() bit for bit - the un-merged gradients of bl, al, l and the re-merged next{s} meet."""
    from surs_amd import model
    opt = tg.opt("joint57")
    net = model.SuRSNet(opt).to(device=_dev())
    net.load_state_dict(tg.state_dict("joint57"))
    x = torch.from_numpy(_u("step_x", 4, (1, 256, 8, 8))).to(_dev())
    G = [torch.from_numpy(_u("step_G%d" % s, 5 + s, (1, opt.hg_dim, 8, 8))).to(_dev()) for s in range(2)]
    before = net.filter_lr_train(x)
    before = [o.clone() for o in before]
    _, grads = net.filter_lr_backward(G)
    p = net.hg_parameters()
    with torch.no_grad():
        for k, v in p.items():
            v -= 1e-3 * grads[k]
    net.commit()
    after = net.filter_lr_train(x)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
    fresh = model.SuRSNet(opt).to(device=_dev())
    fresh.load_state_dict(net.state_dict())
    want = fresh.filter_lr_train(x)
    for s in range(2):
        assert torch.equal(after[s], want[s]), s
