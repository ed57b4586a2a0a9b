"""GPU checks of the hourglass gradients: the primitives of csrc/surs_hg_grad.hip against torch-CPU float64, and the modules
(native.hg_train_forward / hg_backward, SuRSNet.conv_block_* / hourglass_*, autograd.conv_block / autograd.hourglass) against the
reference's own float64 gradients on kink-safe inputs (tests/golden/hg_grads_*.npz, tools/gen_golden_hg_grads.py,
tests/hg_grad_common.py).

Bounds, all in the metric  max |t - t64| / max |t64|  per tensor.  Primitives: 8 max(e32, 2^-22) with e32 torch's own float32 distance
from its float64 value in that test.  Modules, per stored quantity: 8 max(e_ref, 2^-20) (sr_grad_common.compare's rule).  Every parity
test prints its worst ratio before it asserts."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hg_grad_common as hg
from surs_amd import prng

pytestmark = pytest.mark.gpu

PRIM_FLOOR = 2.0 ** -22


# ------------------------------------------------------------------ helpers
def _dev():
    import gpu_common as g
    return g.dev()


def _img(a, ld=None, c0=0):
    """numpy [C,H,W] -> native.Img with channel pitch ld at channel offset c0, NaN everywhere else."""
    from surs_amd import native
    c, h, w = a.shape
    ld = c if ld is None else ld
    buf = torch.full((h * w, ld), float("nan"), dtype=torch.float32)
    buf[:, c0:c0 + c] = torch.from_numpy(np.ascontiguousarray(a.transpose(1, 2, 0))).reshape(h * w, c)
    return native.Img(h, w, c, ld, buf.reshape(-1).to(_dev()), off=c0)


def _chw(img):
    """native.Img -> numpy [C,H,W] (its channels), and everything else of the rows."""
    t = img.buf.reshape(img.h * img.w, img.ld).cpu()
    own = t[:, img.off:img.off + img.c]
    gap = torch.cat((t[:, :img.off], t[:, img.off + img.c:]), 1)
    return own.reshape(img.h, img.w, img.c).permute(2, 0, 1).numpy(), gap


def _u(tag, seed, shape, lo=-1.0, hi=1.0):
    return prng.uniform("hg_grad_prim_" + tag, seed, shape, lo, hi)


def _close(name, got, ref64, ref32):
    """max |got - ref64| / max |ref64| <= 8 max(torch's own float32 distance, 2^-22)."""
    ref64 = np.asarray(ref64, np.float64)
    top = float(np.abs(ref64).max())
    e32 = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) / top
    bound = 8.0 * max(e32, PRIM_FLOOR)
    dev = float(np.abs(np.asarray(got, np.float64) - ref64).max()) / top
    print("%s: deviation %.3g of max |t64| (%.2f of the bound %.3g; torch float32: %.3g)" % (name, dev, dev / bound, bound, e32))
    assert np.isfinite(np.asarray(got)).all(), name
    assert dev <= bound, (name, dev, bound)


# ------------------------------------------------------------------ GroupNorm + ReLU backward
GN_SHAPES = [  # h, w, c, pitch, channel offset, add
    (2, 3, 64, 64, 0, False),
    (8, 12, 128, 256, 64, True),       # a slice of a 256-pitch map, added to what dx holds
    (28, 40, 256, 256, 0, False),      # 1120 pixels: parts of 64 pixels, the last one partial; every lane's pixel stride
]
_gn_ref = {}


def _gn_case(h, w, c):
    """Seeded inputs and the float64 / float32 torch gradients of <g, relu(group_norm(x))> (computed once per shape).  Channel 3 has
    gamma == 0, channel 5 a g that is zero throughout; g is zeroed within 1e-4 of the kink."""
    key = (h, w, c)
    if key not in _gn_ref:
        x = _u("gx", c + h, (c, h, w), -2.0, 2.0)
        gamma, beta = _u("gamma", c, (c,), 0.5, 1.5), _u("beta", c + 1, (c,), -0.5, 0.5)
        gamma[3] = 0.0
        g = _u("gg", c + w, (c, h, w))
        g[5] = 0.0
        y64 = F.group_norm(torch.from_numpy(x).double()[None], 32, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5)[0]
        near = (y64.abs() < 1e-4 * float(y64.abs().max())).numpy()
        near[3] = False                                    # (gamma == 0: y == beta[3] everywhere, far from zero)
        share = float(near.mean())
        assert share <= 1e-3, share
        g[near] = 0.0
        out = {}
        for dt in (torch.float64, torch.float32):
            xt = torch.from_numpy(x).to(dt)[None].requires_grad_()
            ga, be = torch.from_numpy(gamma).to(dt).requires_grad_(), torch.from_numpy(beta).to(dt).requires_grad_()
            L = (torch.from_numpy(g).to(dt)[None] * F.relu(F.group_norm(xt, 32, ga, be, 1e-5))).sum()
            out[dt] = [t.detach().double().numpy() for t in torch.autograd.grad(L, (xt, ga, be))]
        _gn_ref[key] = dict(x=x, gamma=gamma, beta=beta, g=g, share=share, r64=out[torch.float64], r32=out[torch.float32])
    return _gn_ref[key]


@pytest.mark.parametrize("h,w,c,ld,c0,add", GN_SHAPES)
def test_groupnorm_relu_grad_against_float64(h, w, c, ld, c0, add):
    from surs_amd import native
    p = _gn_case(h, w, c)
    tag = "gn %dpx c%d%s" % (h * w, c, " add" if add else "")
    print("%s: share of g zeroed next to the kink %.2e" % (tag, p["share"]))
    x, g = _img(p["x"], ld, c0), _img(p["g"], ld, c0)
    gamma, beta = torch.from_numpy(p["gamma"]).to(_dev()), torch.from_numpy(p["beta"]).to(_dev())
    coeffs = native.groupnorm_fold(x, gamma, beta)
    # the fold of a map without statistics: the scale / shift of the forward's own two launches, bit for bit
    sc, sh = native.groupnorm_coeffs(x, gamma, beta)
    assert torch.equal(coeffs[2], sc) and torch.equal(coeffs[3], sh)
    assert float(coeffs[2][3]) == 0.0 and float(coeffs[3][3]) == float(p["beta"][3])
    dx0, dga, dbe = native.groupnorm_relu_grad(g, x, coeffs, gamma)
    got, gap = _chw(dx0)
    if add:
        fill = _u("fill", c, p["x"].shape)
        dx, dga2, dbe2 = native.groupnorm_relu_grad(g, x, coeffs, gamma, dx=_img(fill, ld, c0), add=True, dgamma=dga.clone(), dbeta=dbe.clone(),
                                                    accumulate=True)
        got_add, gap = _chw(dx)
        assert np.array_equal(got_add, fill + got)                          # one fp32 addition per element
        assert gap.shape[1] == ld - c and bool(torch.isnan(gap).all())      # nothing outside the slice was written
        assert torch.equal(dga2, dga + dga) and torch.equal(dbe2, dbe + dbe)
    (rx, rg, rb), (fx, fg, fb) = p["r64"], p["r32"]
    _close(tag + " dx", got, rx[0], fx[0])
    _close(tag + " dgamma", dga.cpu().numpy(), rg, fg)
    _close(tag + " dbeta", dbe.cpu().numpy(), rb, fb)
    assert float(dga[5]) == 0.0 and float(dbe[5]) == 0.0                    # g == 0 throughout: exact zeros
    # the same bits again, into other buffers
    dx1, dga1, dbe1 = native.groupnorm_relu_grad(g, x, coeffs, gamma)
    assert np.array_equal(_chw(dx1)[0], got) and torch.equal(dga1, dga) and torch.equal(dbe1, dbe)


def test_groupnorm_fold_restates_the_in_kernel_fold():
    """Statistics handed from kernel to kernel: relu(x * scale + shift) with surs_groupnorm_fold's vectors, convolved, equals the
    convolution that folds the same statistics itself (conv2d_gn) bit for bit - the mask the backward recomputes is the forward's."""
    from surs_amd import native
    c, h, w = 256, 8, 12
    sd = hg.state_dict("cb_tiny")
    cw = native.ConvWeights(sd[hg.P + "conv2.conv1.weight"], None, _dev())
    gamma, beta = (torch.from_numpy(sd[hg.P + "conv2.bn1." + k]).to(_dev()) for k in ("weight", "bias"))
    big = _img(_u("fx", 1, (c, 2 * h, 2 * w), -2.0, 2.0))
    x = native.avgpool2(big, want_stats=True)
    assert x.stats is not None and native.conv_gn_eligible(x, cw)
    mean, rstd, scale, shift = native.groupnorm_fold(x, gamma, beta)
    fused = native.conv2d_gn(x, cw, gn=(gamma, beta))
    plain = native.conv2d(x, cw, in_scale=scale, in_shift=shift)
    assert torch.equal(fused.buf, plain.buf)
    # mean / rstd against float64, and scale / shift consistent with them
    x64 = x.buf.reshape(h * w, 32, c // 32).double().cpu()
    m64, v64 = x64.mean((0, 2)), x64.var((0, 2), unbiased=False)
    assert float((mean.cpu().double() - m64).abs().max()) <= 2.0 ** -22
    assert float((rstd.cpu().double() * torch.sqrt(v64 + 1e-5) - 1).abs().max()) <= 2.0 ** -22


# ------------------------------------------------------------------ pool and bicubic transposes
SOURCES = [(1, 2), (2, 3), (3, 5), (6, 4)]
C_EW = 8


def _transpose_ref(kind, h, w):
    g = _u(kind + "_g", h + 3 * w, (C_EW, 2 * h, 2 * w))
    out = []
    for dt in (torch.float64, torch.float32):
        if kind == "pool":
            x = torch.zeros((1, C_EW, 2 * h, 2 * w), dtype=dt, requires_grad=True)
            y = F.avg_pool2d(x, 2, stride=2)
            gg = torch.from_numpy(_u("pool_g", h + 3 * w, (C_EW, h, w))).to(dt)
        else:
            x = torch.zeros((1, C_EW, h, w), dtype=dt, requires_grad=True)
            y = F.interpolate(x, scale_factor=2, mode="bicubic", align_corners=True)
            gg = torch.from_numpy(g).to(dt)
        out.append(torch.autograd.grad((gg[None] * y).sum(), x)[0][0].double().numpy())
    return gg.double().numpy().astype(np.float32), out[0], out[1]


@pytest.mark.parametrize("h,w", SOURCES)
@pytest.mark.parametrize("kind", ["pool", "bicubic"])
def test_transposes_against_float64(kind, h, w):
    """Replace and add, with pitches above the channel count and NaN in every gap."""
    from surs_amd import native
    g_np, r64, r32 = _transpose_ref(kind, h, w)
    fn = native.avgpool2_grad if kind == "pool" else native.bicubic_up2_grad
    g = _img(g_np, C_EW + 4)
    dx = fn(g)
    got, _ = _chw(dx)
    assert got.shape == r64.shape
    _close("%s %dx%d" % (kind, h, w), got, r64, r32)
    fill = _u(kind + "_fill", h + w, r64.shape)
    acc = fn(g, dx=_img(fill, C_EW + 12, 4), add=True)
    got_add, gap = _chw(acc)
    assert np.array_equal(got_add, fill + got)                              # one fp32 addition per element
    assert gap.shape[1] == 12 and bool(torch.isnan(gap).all())
    assert np.array_equal(_chw(fn(_img(g_np)))[0], got)                     # the bits do not depend on the pitch


@pytest.mark.parametrize("h,w", SOURCES)
def test_bicubic_transpose_is_the_adjoint_of_the_forward(h, w):
    """<up(x), g> == <x, up^T(g)> with the library's forward, both sides summed in float64 on the host.  Each side's fp32 elements carry
    at most ~ 32 roundings of 2^-24 relative to sum |weights| |operand| <= 1.375^2 max |operand| per element (the cubic weights at
    A = -0.75 sum to at most 1.375 in absolute value per axis): |lhs - rhs| <= 32 * 2^-24 * 1.375^2 * (sum |g| max |x| + sum |x| max |g|)."""
    from surs_amd import native
    x_np, g_np = _u("adj_x", h, (C_EW, h, w)), _u("adj_g", w, (C_EW, 2 * h, 2 * w))
    up, _ = _chw(native.bicubic_up2(_img(x_np, C_EW + 4), True))
    upt, _ = _chw(native.bicubic_up2_grad(_img(g_np, C_EW + 4)))
    lhs = float((up.astype(np.float64) * g_np).sum())
    rhs = float((x_np.astype(np.float64) * upt).sum())
    bound = 32 * 2.0 ** -24 * 1.375 ** 2 * (float(np.abs(g_np).sum()) * float(np.abs(x_np).max()) + float(np.abs(x_np).sum()) * float(np.abs(g_np).max()))
    print("adjoint %dx%d: <up x, g> = %.9g, <x, upT g> = %.9g, difference %.3g (bound %.3g)" % (h, w, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


# ------------------------------------------------------------------ the modules
_cases = {}


class _Case:
    def __init__(self, golden_dir, name):
        from surs_amd import model
        self.name = name
        self.module = hg.CASES[name][0]
        self.gold = hg.load_fixture(golden_dir, name)
        self.opt = hg.opt(name)
        self.net = model.SuRSNet(self.opt).to(device=_dev())
        self.net.load_state_dict(hg.state_dict(name))
        self.x = torch.from_numpy(hg.inputs(name, int(self.gold["seed"]))).to(_dev())
        self.G = torch.from_numpy(hg.upstream(name)).to(_dev())
        self.B, _, self.h, self.w = self.x.shape
        self.prefixes = hg.hourglass_blocks(0, self.opt.hg_depth) if self.module == "m0" else [hg.P + "conv2."]

    def native_net(self):
        from surs_amd import encoder, native
        n = encoder._native_net(self.net._encoder_weights()).net
        return n, (0 if self.module == "m0" else native.hg_block_of(n, hg.P + "conv2.", self.opt.hg_depth))

    def params(self):
        return self.net._hg_param_set()[0].tensors

    def train(self, x=None):
        x = self.x if x is None else x
        return self.net.hourglass_train(0, x) if self.module == "m0" else self.net.conv_block_train("conv2", x)

    def backward(self, g=None):
        g = self.G if g is None else g
        return self.net.hourglass_backward(0, g) if self.module == "m0" else self.net.conv_block_backward("conv2", g)

    def nhwc(self, t, b):
        return t[b].permute(1, 2, 0).contiguous()


def _case(golden_dir, name):
    if name not in _cases:
        _cases[name] = _Case(golden_dir, name)
    return _cases[name]


def _check(c, grads, dx, tag=""):
    """grads: key -> tensor (any order); dx [B,256,h,w]: against the fixture, every parameter of the case and the input."""
    assert sorted(grads) == sorted(hg.param_keys(c.name))
    sd = hg.state_dict(c.name)
    for k, v in grads.items():
        assert tuple(v.shape) == tuple(sd[k].shape) and v.dtype == torch.float32 and v.is_cuda, k
    assert tuple(dx.shape) == tuple(c.x.shape)
    both = OrderedDict((k, grads[k].detach().cpu().numpy()) for k in hg.param_keys(c.name))
    both[hg.INPUT_KEY] = dx.detach().cpu().numpy()
    rows = hg.compare(c.gold, both)
    name, ratio = hg.worst(rows)
    print("%s%s: %d quantities, worst deviation / bound = %.3f at %s; worst deviation / max(e_ref, 2^-20) = %.3f (bound 8)"
          % (c.name, tag, len(rows), ratio, name, max(d / (b / 8.0) for _, d, b in rows)))
    bad = [r for r in rows if not r[1] <= r[2]]
    assert not bad, bad[:5]


MODULE_CASES = ["cb_tiny", "hg_d1", "hg_d2"]


@pytest.mark.parametrize("name", MODULE_CASES)
def test_train_forward_equals_the_host_mirror(golden_dir, name):
    from surs_amd import encoder
    from surs_amd.model import _as_img, _as_nchw_view
    c = _case(golden_dir, name)
    out = c.train()
    W = c.net._encoder_weights()
    for b in range(c.B):
        x = _as_img(c.x[b:b + 1])
        assert x.stats is None
        mirror = encoder.hourglass(W, hg.P + "m0.", c.opt.hg_depth, x) if c.module == "m0" else encoder.conv_block(W, hg.P + "conv2.", x)
        assert torch.equal(out[b:b + 1], _as_nchw_view(mirror)), b
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.0


@pytest.mark.parametrize("name", MODULE_CASES)
def test_module_parity_with_the_reference(golden_dir, name):
    c = _case(golden_dir, name)
    c.train()
    dx, grads = c.backward()
    assert list(grads) == [k for p in c.prefixes for k in hg.block_keys(p)]
    _check(c, grads, dx, tag=" model")


@pytest.mark.parametrize("name", MODULE_CASES)
def test_batch_equals_accumulating_single_images(golden_dir, name):
    """native.hg_train_forward + native.hg_backward image by image, the second with accumulate: the model's bits; a batch of two
    equals the sum of its images' gradients (one fp32 addition per element)."""
    from surs_amd import native
    from surs_amd.model import _as_img
    c = _case(golden_dir, name)
    n, which = c.native_net()
    tapes = [native.hg_train_forward(n, which, _as_img(c.x[b:b + 1]))[1] for b in range(c.B)]
    grads, single, dxs = None, [], []
    for b in range(c.B):
        single.append(native.hg_backward(n, which, c.prefixes, c.params(), tapes[b], c.h, c.w, c.nhwc(c.G, b))[1])
        dx, grads = native.hg_backward(n, which, c.prefixes, c.params(), tapes[b], c.h, c.w, c.nhwc(c.G, b), grads=grads, accumulate=b > 0)
        dxs.append(dx)
    c.train()
    mdx, mgrads = c.backward()
    assert torch.equal(torch.stack(dxs, 0).permute(0, 3, 1, 2), mdx)
    for k in grads:
        assert torch.equal(grads[k], mgrads[k]), k
        assert torch.equal(grads[k], single[0][k] + single[1][k] if c.B == 2 else single[0][k]), k
    _check(c, grads, mdx, tag=" native")


def _fenced(nbytes, offset_bytes=0):
    """A float32 buffer of NaN with `nbytes` usable bytes starting 1024 + offset_bytes bytes into it; (whole buffer, the usable view)."""
    n = (nbytes + 3) // 4
    buf = torch.full((256 + offset_bytes // 4 + n + 256,), float("nan"), dtype=torch.float32, device=_dev())
    return buf, buf[256 + offset_bytes // 4: 256 + offset_bytes // 4 + n]


def _fences_intact(buf, view):
    lo = view.data_ptr() - buf.data_ptr()
    return bool(torch.isnan(buf[:lo // 4]).all()) and bool(torch.isnan(buf[lo // 4 + view.numel():]).all())


@pytest.mark.parametrize("name", ["cb_tiny", "hg_d1"])
def test_same_bits_twice_and_nothing_outside_is_written(golden_dir, name):
    """Two runs with the tape and the workspace at other addresses and other offsets inside their allocations give the same bits; tape,
    workspace and every gradient buffer sit between NaN fences that stay NaN, and every gradient is finite."""
    from surs_amd import native
    from surs_amd.model import _as_img
    c = _case(golden_dir, name)
    n, which = c.native_net()
    hourglass = c.module == "m0"
    tb, wb = native.hg_tape_bytes(n, c.h, c.w, hourglass), native.hg_backward_workspace_bytes(n, c.h, c.w, hourglass)
    keys = [k for p in c.prefixes for k in hg.block_keys(p)]
    runs = []
    for tape_off, ws_off in ((0, 0), (768, 256 + 1024)):     # (both stay 256-byte aligned inside allocations that move)
        tape_buf, tape = _fenced(tb, tape_off)
        ws_buf, ws = _fenced(wb, ws_off)
        if tape.data_ptr() % 256 or ws.data_ptr() % 256:
            pytest.fail("the allocator handed out a buffer that is not 256-byte aligned")
        fenced = OrderedDict((k, _fenced(c.params()[k].numel() * 4)) for k in keys)
        grads = OrderedDict((k, fenced[k][1].view(c.params()[k].shape)) for k in keys)
        outs, dxs = [], []
        for b in range(c.B):
            out, _ = native.hg_train_forward(n, which, _as_img(c.x[b:b + 1]), tape=tape)
            dx, _ = native.hg_backward(n, which, c.prefixes, c.params(), tape, c.h, c.w, c.nhwc(c.G, b), grads=grads, accumulate=b > 0,
                                       workspace=ws)
            outs.append(out.buf.clone())
            dxs.append(dx)
        torch.cuda.synchronize()
        assert _fences_intact(tape_buf, tape) and _fences_intact(ws_buf, ws)
        for k, (buf, view) in fenced.items():
            assert _fences_intact(buf, view), k
            assert bool(torch.isfinite(view).all()), k
        runs.append((grads, outs, dxs))
    (g0, o0, d0), (g1, o1, d1) = runs
    for k in g0:
        assert g0[k].data_ptr() != g1[k].data_ptr() and torch.equal(g0[k], g1[k]), k
    assert all(torch.equal(a, b) for a, b in zip(o0 + d0, o1 + d1))
    _check(c, g0, torch.stack(d0, 0).permute(0, 3, 1, 2), tag=" fenced")


def test_backward_without_a_train_forward_raises(golden_dir):
    from surs_amd import model
    c = _case(golden_dir, "hg_d1")
    net = model.SuRSNet(c.opt).to(device=_dev())
    net.load_state_dict(hg.state_dict("hg_d1"))
    with pytest.raises(RuntimeError, match="hourglass_train"):
        net.hourglass_backward(0, c.G)
    with pytest.raises(RuntimeError, match="conv_block_train"):
        net.conv_block_backward("conv2", c.G)
    net.conv_block_train("conv2", c.x)                      # another module's tape does not serve
    with pytest.raises(RuntimeError, match="conv_block_train"):
        net.conv_block_backward("m0.b1_1", c.G)
    with pytest.raises(ValueError, match="not a multiple of 2"):
        net.hourglass_train(0, c.x[:, :, :3, :])


def test_parameters_are_cached_and_dropped_by_load_state_dict(golden_dir):
    from surs_amd import native
    c = _case(golden_dir, "hg_d1")
    p = c.net.hg_parameters()
    sd = hg.state_dict("hg_d1")
    assert p is c.net.hg_parameters() and list(p) == native.hg_param_keys(sd, c.opt.num_stack_lr, c.opt.hg_depth)
    for k, v in p.items():
        assert isinstance(v, torch.nn.Parameter) and v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == tuple(sd[k].shape)
        assert v.data_ptr() == c.params()[k].data_ptr()
        assert np.array_equal(v.detach().cpu().numpy(), sd[k])
    c.net.load_state_dict(sd)
    assert c.net.hg_parameters() is not p


# ------------------------------------------------------------------ autograd.conv_block / autograd.hourglass
def test_autograd_functions(golden_dir):
    from surs_amd import autograd
    c = _case(golden_dir, "hg_d1")
    net, params = c.net, c.net.hg_parameters()
    x = c.x.clone().requires_grad_()
    out = autograd.hourglass(net, 0, x)
    assert out.grad_fn is not None and torch.equal(out, c.train())
    want_dx, want = c.backward()
    keys = list(want)
    got = torch.autograd.grad((c.G * out).sum(), [x] + [params[k] for k in keys], retain_graph=True)
    assert torch.equal(got[0], want_dx)
    for k, g in zip(keys, got[1:]):
        assert torch.equal(g, want[k]), k
    # a backward long after other work has replaced the tape on the net uses the tape of ITS forward
    net.hourglass_train(0, c.x[:1] * 0.5)
    got = torch.autograd.grad((c.G * out).sum(), [x] + [params[k] for k in keys])
    assert torch.equal(got[0], want_dx) and all(torch.equal(g, want[k]) for k, g in zip(keys, got[1:]))
    # a single block, named without the filter's prefix
    out = autograd.conv_block(net, "m0.b2_plus_1", x)
    dx, grads = (net.conv_block_train("m0.b2_plus_1", c.x), net.conv_block_backward("m0.b2_plus_1", c.G))[1]
    got = torch.autograd.grad((c.G * out).sum(), [x] + [params[k] for k in grads])
    assert torch.equal(got[0], dx) and all(torch.equal(g, grads[k]) for k, g in zip(grads, got[1:]))


def _fresh(c):
    from surs_amd import model
    net = model.SuRSNet(c.opt).to(device=_dev())
    net.load_state_dict(hg.state_dict(c.name))
    return net


def test_autograd_backward_leaves_the_models_tape_alone(golden_dir):
    """The Function owns the tape of its forward: its backward, run after hourglass_train() on ONE other image has filed the model's own
    latest tape, gives the first forward's gradients, and hourglass_backward() then gives what it gives on a fresh net after that
    hourglass_train() alone - the model's tape, its key and its image count are as the train call left them."""
    from surs_amd import autograd
    c = _case(golden_dir, "hg_d1")
    net, params = c.net, c.net.hg_parameters()
    c.train()
    want_dx, want = c.backward()
    keys = list(want)
    x = c.x.clone().requires_grad_()
    out = autograd.hourglass(net, 0, x)
    net.hourglass_train(0, c.x[:1] * 0.5)
    kept, filed = net._tapes[0], set(net._tapes)
    got = torch.autograd.grad((c.G * out).sum(), [x] + [params[k] for k in keys])
    assert torch.equal(got[0], want_dx)
    for k, g in zip(keys, got[1:]):
        assert torch.equal(g, want[k]), k
    assert net._tapes[0] is kept and len(kept[2]) == 1 and set(net._tapes) == filed
    dx, grads = net.hourglass_backward(0, c.G[:1])
    fresh = _fresh(c)
    fresh.hourglass_train(0, c.x[:1] * 0.5)
    fresh_dx, fresh_grads = fresh.hourglass_backward(0, c.G[:1])
    assert torch.equal(dx, fresh_dx) and list(grads) == list(fresh_grads)
    for k in grads:
        assert torch.equal(grads[k], fresh_grads[k]), k


def test_explicit_tapes_serve_their_own_forward(golden_dir):
    """conv_block_backward(tapes=): the tapes of a first forward, passed after the same block ran on another input, give the first
    forward's backward bit for bit, and the model's own entry is neither used nor changed."""
    c = _case(golden_dir, "hg_d1")
    net, block = c.net, "m0.b2_plus_1"
    net.conv_block_train(block, c.x)
    first = net._tapes[hg.P + block + "."]
    want_dx, want = net.conv_block_backward(block, c.G)
    net.conv_block_train(block, c.x[:1] * 0.5)
    latest = net._tapes[hg.P + block + "."]
    assert latest is not first and len(first[2]) == c.B and len(latest[2]) == 1
    dx, grads = net.conv_block_backward(block, c.G, tapes=first)
    assert torch.equal(dx, want_dx) and list(grads) == list(want)
    for k in grads:
        assert torch.equal(grads[k], want[k]), k
    assert net._tapes[hg.P + block + "."] is latest


def test_composed_stack_against_the_reference(golden_dir):
    """stack1: conv2 -> m0 -> top_m_0 through the two autograd Functions, then conv_last0 / bn_end0 / ReLU / l0 in plain torch on
    hg_parameters() (1 x 1 convolutions as matrix products, GroupNorm from mean and variance): the hand-off to torch autograd and a
    composed filter_lr, every parameter's gradient and the input's against the reference's."""
    from surs_amd import autograd
    c = _case(golden_dir, "stack1")
    net, p = c.net, c.net.hg_parameters()
    for v in p.values():
        v.grad = None
    x = c.x.clone().requires_grad_()
    t = autograd.conv_block(net, "top_m_0", autograd.hourglass(net, 0, autograd.conv_block(net, "conv2", x)))
    pw = lambda k, u: torch.einsum("oc,bchw->bohw", p[hg.P + k + ".weight"][:, :, 0, 0], u) + p[hg.P + k + ".bias"][None, :, None, None]
    u = pw("conv_last0", t)
    B, C, h, w = u.shape
    ug = u.reshape(B, 32, -1)
    mean, var = ug.mean(2, keepdim=True), ug.var(2, unbiased=False, keepdim=True)
    un = ((ug - mean) / torch.sqrt(var + 1e-5)).reshape(B, C, h, w)
    un = un * p[hg.P + "bn_end0.weight"][None, :, None, None] + p[hg.P + "bn_end0.bias"][None, :, None, None]
    out = pw("l0", torch.relu(un))
    assert tuple(out.shape) == tuple(c.G.shape)
    (c.G * out).sum().backward()
    keys = hg.param_keys("stack1")
    assert all(p[k].grad is not None for k in keys)
    untouched = [k for k in p if k not in keys]
    assert all(p[k].grad is None for k in untouched)
    _check(c, OrderedDict((k, p[k].grad) for k in keys), x.grad, tag=" composed")
    for v in p.values():
        v.grad = None
