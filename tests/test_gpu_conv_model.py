"""The encoder's split-operand convolutions - conv_x3_kernel on each of its tiles with two f16 parts per operand, one f16 part and
three bf16 parts, stride 1 and 2, and both instantiations of conv1x1_x2_kernel - held to tests/conv_model.py: a float64 model that
rounds where the kernels' sources round and forms the partial products they form.  A correct kernel differs from it by accumulation
order only, so the tolerance is the model's own distance to itself accumulating in fp32 (the kernels' order and its reverse) - not
2e-5 of the output range, which hides what tests/test_conv_model_host.py shows this bound to catch (a truncating conversion, flushed
subnormal parts, one lost partial product, a remainder rounded twice, a fused prologue, padding before the prologue, a bias through
f16), and which a CORRECT kernel legitimately misses below the two-part window.

Per case, over ALL output elements:   dev = |kernel - float64 model|,   e = |fp32-accumulating model - float64 model| (the larger of
the two orders),   floor = 2^-22 max |float64 model|;
    mean(dev) <= 8 max(mean(e), floor),    max(dev) <= 8 max(max(e), floor),    and the same for the median
(column_model.bounds).  Every case prints mean(dev) / mean(e) and max(dev) / max(e) before it asserts; NOTES.md ("conv model") has
the figures of an MI355X, and what rung (2^-20, 1) showed about subnormal operands in the matrix pipe (conv_model._aligned).

Cases (conv_model.KINDS, operands(): everything from seeds, repack_common.PLANTED planted in x and w): 3x3 48 -> 96 on 11 x 40 under
every forced tile, stride 2 on 11 x 41, 1x1 48 -> 256 and 48 -> 64 on 5 x 33; variants plain + bias, prologue + LeakyReLU +
residual into a channel slice between NaN, and the GroupNorm-statistics prologue (64 input channels) with the coefficients the
library folded; the magnitude ladder in full on the plain stride-1 4x32 two-part case and on the plain 1x1 <4> case, three rungs of
it elsewhere; one overflow case per kernel; two runs of a case give the same bits."""
import warnings

import numpy as np
import pytest
import torch

import column_model as cm
import conv_model as cvm
from conv_tiles import force_tile  # noqa: F401  (the fixture that forces the 3x3 kernel's tile)

pytestmark = pytest.mark.gpu

GAP = (24, 16)                 # channels in front of and behind the output slice of the "epi" variant
_models, _ops = {}, {}


@pytest.fixture(scope="module")
def env():
    import gpu_common as g
    from surs_amd import native
    return dict(g=g, native=native, dev=g.dev())


def _chw(img):
    return img.to_nchw()[0].cpu().numpy()


def _dev(env, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(env["dev"])


def _operands(kind, rung, variant, overflow=False):
    key = (kind, rung, variant, overflow)
    if key not in _ops:
        _ops[key] = cvm.operands(kind, rung, variant, overflow=overflow)
    return _ops[key]


def _weights(env, op, parts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (the rungs below W_MIN are here on purpose)
        cw = env["native"].ConvWeights(op["w"], op["b"], env["dev"], reduced=parts == 1)
    assert cw.w3 is not None and cw.parts == (3 if parts == 3 else 2)
    return cw


def launch(env, kind, variant, op, parts):
    """One launch of the case on the library -> (output [cout, ho, wo], (scale, shift) the library folded or (None, None))."""
    nat, g = env["native"], env["g"]
    cout, (ho, wo) = cvm.KINDS[kind][3], cvm.out_size(kind)
    cw, X = _weights(env, op, parts), g.upload_nhwc(op["x"])
    if variant == "plain":
        return _chw(nat.conv2d(X, cw, stride=op["stride"])), (None, None)
    if variant == "gn":
        X = nat.add3(X, g.upload_nhwc(np.zeros_like(op["x"])), want_stats=True)      # x + 0 with the statistics of x
        G, B = _dev(env, op["gamma"]), _dev(env, op["beta"])
        _, _, sc, sh = nat.groupnorm_fold(X, G, B)
        return _chw(nat.conv2d_gn(X, cw, gn=(G, B))), (sc.cpu().numpy(), sh.cpu().numpy())
    wide = nat.Img(ho, wo, GAP[0] + cout + GAP[1], device=env["dev"])
    wide.buf.fill_(float("nan"))
    nat.conv2d(X, cw, out=wide.slice(GAP[0], cout), stride=op["stride"], in_scale=_dev(env, op["scale"]), in_shift=_dev(env, op["shift"]),
               act=1, slope=cvm.SLOPE, residual=g.upload_nhwc(op["res"]))
    full = _chw(wide)
    assert np.isnan(full[:GAP[0]]).all() and np.isnan(full[GAP[0] + cout:]).all()    # the gap holds NaN before and after
    return full[GAP[0]:GAP[0] + cout], (None, None)


def model(kind, variant, rung, parts, op, coeffs, overflow=False):
    """(float64 model, [fp32 ascending, fp32 descending]) of a case, computed once per module (no tile changes it)."""
    key = (kind, variant, rung, parts, overflow)
    if key not in _models:
        _models[key] = cvm.models(op, parts, *coeffs) + (coeffs,)
    ref, forms, had = _models[key]
    if coeffs[0] is not None:                                                        # the fold gives the same bits every time
        assert np.array_equal(had[0], coeffs[0]) and np.array_equal(had[1], coeffs[1])
    return ref, forms


def hold(name, y, ref, forms, sel=None):
    sel = np.ones(ref.shape, bool) if sel is None else sel
    assert y.shape == ref.shape and np.isfinite(y[sel]).all(), name
    bound, e = cvm.bounds(ref, forms, sel)
    dev = np.abs(y.astype(np.float64) - ref)[sel]
    print("%-44s mean(dev) / mean(e) = %6.3f   max(dev) / max(e) = %6.3f   median(dev) / its bound = %5.3f   (dev mean %.3g max %.3g; "
          "bounds %.3g %.3g %.3g; range %.3g)" % (name, dev.mean() / e.mean(), dev.max() / e.max(), np.median(dev) / bound["median"], dev.mean(),
                                                 dev.max(), bound["mean"], bound["max"], bound["median"], np.abs(ref[sel]).max()))
    assert not cm.breaks(dev, bound), (name, cm.breaks(dev, bound))


def check(env, kind, variant, rung, parts, tag, twice=False):
    op = _operands(kind, rung, variant)
    y, coeffs = launch(env, kind, variant, op, parts)
    ref, forms = model(kind, variant, rung, parts, op, coeffs)
    hold("%s %s %s %s" % (kind, tag, variant, cvm.rung_name(rung)), y, ref, forms)
    if twice:
        again = launch(env, kind, variant, op, parts)[0]
        assert np.array_equal(again.view(np.uint32), y.view(np.uint32)), (kind, tag, variant)


def _rungs(full):
    return [pytest.param(r, id=cvm.rung_name(r).replace(" ", "")) for r in (cvm.LADDER if full else cvm.SHORT)]


def _stride1(env, force_tile, monkeypatch, tile, parts, rung):
    if parts == 3:
        monkeypatch.setenv("SURS_CONV_SPLIT", "bf16x3")
    force_tile(tile)
    tag = "%s x%d" % (tile, parts)
    check(env, "s1", "plain", rung, parts, tag, twice=rung == (1.0, 1.0))
    if rung in cvm.SHORT:
        check(env, "s1", "epi", rung, parts, tag, twice=rung == (1.0, 1.0))
        if parts != 3:      # (conv2d_gn reads the two-part image)
            check(env, "s1g", "gn", rung, parts, tag, twice=rung == (1.0, 1.0))


@pytest.mark.parametrize("rung", _rungs(True))
def test_conv3x3_small_tile_over_the_whole_ladder(env, force_tile, monkeypatch, rung):
    _stride1(env, force_tile, monkeypatch, "4x32", 2, rung)


@pytest.mark.parametrize("rung", _rungs(False))
@pytest.mark.parametrize("tile,parts", [("8x32", 2), ("8x64", 2), ("4x32", 1), ("8x32", 1), ("4x32", 3)])
def test_conv3x3_stride1_against_the_model(env, force_tile, monkeypatch, tile, parts, rung):
    _stride1(env, force_tile, monkeypatch, tile, parts, rung)


@pytest.mark.parametrize("rung", _rungs(False))
@pytest.mark.parametrize("parts", [2, 1])
def test_conv3x3_stride2_against_the_model(env, parts, rung):
    for variant in ("plain", "epi"):
        check(env, "s2", variant, rung, parts, "4x32 x%d" % parts, twice=rung == (1.0, 1.0))


def _pointwise(env, kind, rung):
    tag = "<%d> x2" % (4 if kind == "p4" else 1)
    check(env, kind, "plain", rung, 2, tag, twice=rung == (1.0, 1.0))
    if rung in cvm.SHORT:
        check(env, kind, "epi", rung, 2, tag, twice=rung == (1.0, 1.0))
        check(env, kind + "g", "gn", rung, 2, tag, twice=rung == (1.0, 1.0))


@pytest.mark.parametrize("rung", _rungs(True))
def test_pointwise_conv_4_over_the_whole_ladder(env, rung):
    _pointwise(env, "p4", rung)


@pytest.mark.parametrize("rung", _rungs(False))
def test_pointwise_conv_1_against_the_model(env, rung):
    _pointwise(env, "p1", rung)


def _neighbourhood(kind):
    """The outputs that read the first pixel: [ho, wo]."""
    k, stride = cvm.KINDS[kind][:2]
    ho, wo = cvm.out_size(kind)
    near = np.zeros((ho, wo), bool)
    for oy in range(ho):
        for ox in range(wo):
            near[oy, ox] = abs(oy * stride) <= k // 2 and abs(ox * stride) <= k // 2
    return near


@pytest.mark.parametrize("kind", ["s1", "s2", "p4", "p1"])
def test_an_f16_overflow_shows_where_the_model_says(env, force_tile, kind):
    """One activation of 65520 (f16 infinity) at the first pixel, one of 65503.9 (finite) mid-map, two parts: the kernel's non-finite
    outputs are exactly the model's - every channel of the outputs that read the first pixel -, the signal reconstruction()'s retry
    keys on; everything else is inside the bound."""
    force_tile("4x32")
    rung = (1.0, 1.0)
    op = _operands(kind, rung, "plain", overflow=True)
    y, _ = launch(env, kind, "plain", op, 2)
    ref, forms = model(kind, "plain", rung, 2, op, (None, None), overflow=True)
    bad = ~np.isfinite(ref)
    assert np.array_equal(bad, np.broadcast_to(_neighbourhood(kind)[None], ref.shape)) and 0 < bad.sum() <= 4 * ref.shape[0]
    assert np.array_equal(~np.isfinite(y), bad), (int((~np.isfinite(y)).sum()), int(bad.sum()))
    hold("%s overflow x2" % kind, y, ref, forms, ~bad)


def test_three_bf16_parts_do_not_overflow(env, force_tile, monkeypatch):
    monkeypatch.setenv("SURS_CONV_SPLIT", "bf16x3")
    force_tile("4x32")
    rung = (1.0, 1.0)
    op = _operands("s1", rung, "plain", overflow=True)
    y, _ = launch(env, "s1", "plain", op, 3)
    ref, forms = model("s1", "plain", rung, 3, op, (None, None), overflow=True)
    assert np.isfinite(ref).all() and np.isfinite(y).all()
    hold("s1 overflow x3", y, ref, forms)
