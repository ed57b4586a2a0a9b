"""tests/conv_model.py is checked before it judges a kernel (no GPU; of the product only the host packers and the host side of
native.ConvWeights):
  a. with every rounding switched off it IS the convolution: conv_ref.conv, on every case of tests/test_gpu_conv_model.py;
  b. its weight splits are the packers' bytes (surs_conv_pack_weights_x2 / _x3 through the C ABI, repack_common.PLANTED planted);
  c. the grade table: the float64 model's distance to the EXACT float64 convolution over the magnitude ladder, for one, two and
     three parts - where the default two-part form is fp32 grade (TOL[2] = 2e-5 of the output range) and where it stops being so,
     pinned from both sides, and W_MIN derived from the same numbers (DESIGN.md 4.5 carries the table);
  d. the bound of test_gpu_conv_model.py separates wrong models: seven perturbed float64 models each break it against the
     unperturbed one on at least one case and rung - and where the old 2e-5-of-range bound would have noticed, which is printed;
  e. native.ConvWeights warns about a two-part image of a weight tensor below W_MIN, and only about that."""
import ctypes as C
import warnings

import numpy as np
import pytest

import column_model as cm
import common
import conv_model as cvm
import repack_common
from surs_amd import native

FULL = {("s1", "plain"), ("p4", "plain")}          # the cases that run the whole ladder
VARIANTS = {"s1": ("plain", "epi"), "s2": ("plain", "epi"), "p4": ("plain", "epi"), "p1": ("plain", "epi"), "s1g": ("gn",),
            "p4g": ("gn",), "p1g": ("gn",)}
_cache = {}


def cases():
    for kind in cvm.KINDS:
        for variant in VARIANTS[kind]:
            for rung in (cvm.LADDER if (kind, variant) in FULL else cvm.SHORT):
                yield kind, variant, rung


def case(kind, variant, rung, plant=True):
    """(operands, scale, shift) - the last two None unless the case is a "gn" one."""
    key = (kind, variant, rung, plant)
    if key not in _cache:
        op = cvm.operands(kind, rung, variant, plant=plant)
        _cache[key] = (op,) + (cvm.coeffs(op) if variant == "gn" else (None, None))
    return _cache[key]


def test_rounding_off_the_model_is_the_convolution():
    worst = 0.0
    for kind, variant, rung in cases():
        op, sc, sh = case(kind, variant, rung)
        want = cvm.exact(op, sc, sh)
        for parts in (1, 2, 3):
            got = cvm.conv(parts=parts, rounding=False, **cvm.model_args(op, sc, sh))
            assert got.shape == want.shape == (cvm.KINDS[kind][3],) + cvm.out_size(kind)
            err = cvm.grade(got, want)
            worst = max(worst, err)
            assert err <= 1e-13, (kind, variant, rung, parts, err)
    # the overflow case: nothing overflows a model that does not round
    op = cvm.operands("s1", (1.0, 1.0), "plain", overflow=True)
    assert cvm.grade(cvm.conv(rounding=False, **cvm.model_args(op)), cvm.exact(op)) <= 1e-13
    print("rounding off: the model's largest distance to conv_ref.conv over every case: %.1e of the range" % worst)


def _unpack(buf, nparts, cout, cin, k):
    """[parts][taps][cin_pad / 16][cout_pad][16] uint16 -> [parts][cout_pad, cin_pad, k, k]."""
    cin_pad, cout_pad = -(-cin // 16) * 16, -(-cout // 64) * 64
    a = buf.view(np.uint16).reshape(nparts, k * k, cin_pad // 16, cout_pad, 16)
    return a.transpose(0, 3, 2, 4, 1).reshape(nparts, cout_pad, cin_pad, k, k)


@pytest.mark.parametrize("k", [3, 1])
def test_the_models_weight_splits_are_the_packers_bytes(k):
    cout, cin = 40, 24                                   # padded both ways: the padding is zero bits
    w = repack_common.values((cout, cin, k, k), seed=31 + k)
    assert all((w == v).any() for v in repack_common.PLANTED[2:]) and (np.signbit(w) & (w == 0)).any()
    R = cvm.Rounding()
    for nparts, fn in ((2, native.lib().surs_conv_pack_weights_x2), (3, native.lib().surs_conv_pack_weights_x3)):
        buf = np.full(fn(None, cout, cin, k, None), 0xA5, np.uint8)
        assert fn(w.ctypes.data_as(C.c_void_p), cout, cin, k, buf.ctypes.data_as(C.c_void_p)) == buf.size
        got = _unpack(buf, nparts, cout, cin, k)
        parts = R.split(w, nparts, act=False)
        for p in range(nparts):
            if nparts == 2:
                want = parts[p].astype(np.float16)
                assert np.array_equal(want.astype(np.float64), parts[p])          # (an f16 value)
                want = want.view(np.uint16)
            else:
                f = parts[p].astype(np.float32)
                assert np.array_equal(f.astype(np.float64), parts[p]) and not (f.view(np.uint32) & np.uint32(0xffff)).any()
                want = (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
            assert np.array_equal(got[p][:cout, :cin], want), (nparts, p)
            pad = got[p].copy()
            pad[:cout, :cin] = 0
            assert not pad.any()
        if nparts == 2:                                  # subnormal second parts are kept, and there are some
            lo = got[1][:cout, :cin]
            assert ((lo & 0x7c00) == 0).any() and ((lo & 0x7fff) != 0)[(lo & 0x7c00) == 0].any()


# ------------------------------------------------------------------ c. the grade table
def grade_rows():
    """{shape: {rung: {parts: distance of the float64 model to the exact float64 convolution, of the output range}}} on operands
    without planted values (a planted 1 would be a uniform weight tensor's max |w|, which the table's weight axis is about)."""
    if "grades" not in _cache:
        rows = {}
        for kind in ("s1", "p4"):
            rows[kind] = {}
            for rung in cvm.LADDER:
                op, _, _ = case(kind, "plain", rung, plant=False)
                ref = cvm.exact(op)
                rows[kind][rung] = {p: cvm.grade(cvm.conv(parts=p, **cvm.model_args(op)), ref) for p in ((1, 2, 3) if kind == "s1" else (2,))}
        _cache["grades"] = rows
    return _cache["grades"]


# the window the documents state: activations of magnitude 2^-8 and more, max |w| >= W_MIN.  Rungs of the ladder inside it (x uniform
# +-1 x scale: the "magnitude" of a rung is its scale; w uniform +-0.2 x scale) ...
INSIDE = [(2.0 ** 14, 1.0), (1.0, 1.0), (2.0 ** -6, 1.0)]
# ... and the first rung outside it on each axis (and the rung that is outside on both)
FIRST_OUTSIDE = [(2.0 ** -10, 1.0), (1.0, 2.0 ** -8)]


def test_grade_table():
    rows = grade_rows()
    print("\ngrade table: distance of the float64 model to the exact float64 convolution, as a fraction of the output range")
    print("%-16s %-14s | 3x3 48->96 11x40: %-10s %-10s %-10s | 1x1 48->256 5x33: %s" % ("rung (x, w)", "max|x|, max|w|", "one f16", "two f16", "three bf16",
                                                                                       "two f16"))
    for rung in cvm.LADDER:
        g, g1 = rows["s1"][rung], rows["p4"][rung]
        print("%-16s %-7.1e %-7.1e| %18s%-10.1e %-10.1e %-10.1e | %18s%.1e" % (cvm.rung_name(rung), rung[0], 0.2 * rung[1], "", g[1], g[2], g[3], "", g1[2]))
    for kind in ("s1", "p4"):
        for rung in cvm.LADDER:
            g = rows[kind][rung]
            if rung in INSIDE:
                assert g[2] <= cvm.TOL[2], (kind, rung, g)
            if rung in FIRST_OUTSIDE:
                assert g[2] > cvm.TOL[2], (kind, rung, g)
            if 3 in g:
                assert g[3] <= cvm.TOL3, (kind, rung, g)
                assert g[1] <= cvm.TOL[1] or rung[0] < 2.0 ** -14      # (one part: 11 bits wherever the activations are normal f16 values)
    # every rung further out on an axis is further off than the first one outside
    for kind in ("s1", "p4"):
        r = rows[kind]
        assert r[(2.0 ** -20, 1.0)][2] > r[(2.0 ** -14, 1.0)][2] > r[(2.0 ** -10, 1.0)][2]
        assert r[(1.0, 2.0 ** -12)][2] > r[(1.0, 2.0 ** -8)][2] and r[(2.0 ** -10, 2.0 ** -8)][2] > r[(2.0 ** -10, 1.0)][2]
    # W_MIN: on the weight axis the error is c 2^-25 / max |w| of the range (an absolute 2^-25 per weight); c from the rungs
    # that are off that axis' flat part, the larger of the shapes'; the smallest power of two m with c 2^-25 / m <= TOL[2] / 2
    cs = [rows[kind][(1.0, s)][2] * (0.2 * s) / 2.0 ** -25 for kind in ("s1", "p4") for s in (2.0 ** -8, 2.0 ** -12)]
    c = max(cs)
    w_min = 2.0 ** np.ceil(np.log2(c * 2.0 ** -25 / (cvm.TOL[2] / 2)))
    print("weight axis: error = c 2^-25 / max|w| with c = %s; W_MIN = 2^%d (modelled loss at W_MIN: %.1e of the range)"
          % (", ".join("%.2f" % v for v in cs), int(np.log2(w_min)), c * 2.0 ** -25 / w_min))
    assert 0.5 <= min(cs) and c <= 2.0                   # (the one-constant law the warning's "modelled loss" states)
    assert w_min == cvm.W_MIN
    # the same law on the activation axis puts the documented rung: the first power of two that holds TOL[2] itself
    cx = max(rows[kind][(s, 1.0)][2] * s / 2.0 ** -25 for kind in ("s1", "p4") for s in (2.0 ** -10, 2.0 ** -14))
    x_min = 2.0 ** np.ceil(np.log2(cx * 2.0 ** -25 / cvm.TOL[2]))
    print("activation axis: error = c 2^-25 / scale with c = %.2f; two parts hold %.0e from scale 2^%d" % (cx, cvm.TOL[2], int(np.log2(x_min))))
    assert x_min == cvm.X_MIN_SCALE


# ------------------------------------------------------------------ d. perturbations
def _perts(kind, variant):
    nch = -(-cvm.KINDS[kind][2] // 16)
    taps = cvm.KINDS[kind][0] ** 2
    p = {"truncating f16 conversion": {"trunc": True}, "f16 subnormals flushed": {"flush": True},
         "x_lo w_hi lost in one step": {"lose": (nch - 1, taps // 2)}, "remainder rounded twice": {"double_rem": True},
         "bias through f16": {"bias_f16": True}}
    if variant != "plain":
        p.update({"prologue as one fma": {"fused_prologue": True}, "padding before the prologue": {"pad_first": True}})
    return p


NAMES = ["truncating f16 conversion", "f16 subnormals flushed", "x_lo w_hi lost in one step", "remainder rounded twice",
         "prologue as one fma", "padding before the prologue", "bias through f16"]


def test_the_bound_separates_wrong_models():
    caught, old, tried = {n: [] for n in NAMES}, {n: [] for n in NAMES}, {n: 0 for n in NAMES}
    for kind, variant, rung in cases():
        op, sc, sh = case(kind, variant, rung)
        ref, forms = cvm.models(op, 2, sc, sh)
        bound, e = cvm.bounds(ref, forms)
        assert not cm.breaks(np.abs(forms[0] - ref).ravel(), bound)       # the bound holds for what it has to let through
        ex = cvm.exact(op, sc, sh)
        assert cvm.grade(ref, ex) < cvm.TOL[2] or rung not in INSIDE
        for name, pert in _perts(kind, variant).items():
            if name == "padding before the prologue" and cvm.KINDS[kind][0] == 1:
                continue                                                  # (a pointwise convolution pads nothing)
            got = cvm.conv(parts=2, pert=pert, **cvm.model_args(op, sc, sh))
            dev = np.abs(got - ref).ravel()
            tried[name] += 1
            tag = "%s %s %s" % (kind, variant, cvm.rung_name(rung))
            if cm.breaks(dev, bound):
                caught[name].append("%s [%s: max %.0fx mean %.0fx its bound]" % (tag, "/".join(cm.breaks(dev, bound)), dev.max() / bound["max"],
                                                                              dev.mean() / bound["mean"]))
            if cvm.grade(got, ex) >= cvm.TOL[2] > cvm.grade(ref, ex):     # the old bound passes the model and fails the perturbation
                old[name].append(tag)
    print("\nperturbation table: on which cases the bound of test_gpu_conv_model.py catches a perturbed model; where the old bound would")
    for name in NAMES:
        print("  %-28s caught on %d of %d cases; the old 2e-5-of-range bound on %d" % (name, len(caught[name]), tried[name], len(old[name])))
        for line in caught[name]:
            print("      %s" % line)
        if old[name]:
            print("      old bound: %s" % ", ".join(old[name]))
    for name in NAMES:
        assert caught[name], name


# ------------------------------------------------------------------ e. the warning
def _weights(peak, shape=(32, 16, 3, 3)):
    w = np.random.RandomState(5).uniform(-1.0, 1.0, shape).astype(np.float32) * np.float32(peak)
    w.reshape(-1)[11] = peak
    return w


def test_a_weight_tensor_below_the_window_warns(monkeypatch):
    monkeypatch.delenv("SURS_CONV_SPLIT", raising=False)
    monkeypatch.delenv("SURS_CONV_X3", raising=False)
    with pytest.warns(RuntimeWarning, match=r"max \|w\|") as rec:
        native.ConvWeights(_weights(cvm.W_MIN / 2), None, "cpu")
    assert len(rec) == 1
    msg = str(rec[0].message)
    assert "(32, 16, 3, 3)" in msg and "SURS_CONV_SPLIT=bf16x3" in msg and "wide_operands" in msg
    assert ("%.1e" % (2.0 ** -25 / (cvm.W_MIN / 2))) in msg and ("%.3g" % (cvm.W_MIN / 2)) in msg
    assert native.CONV_W_MIN == cvm.W_MIN
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        native.ConvWeights(_weights(2 * cvm.W_MIN), None, "cpu")
        native.ConvWeights(_weights(cvm.W_MIN), None, "cpu")                        # at W_MIN: inside the window
        native.ConvWeights(np.zeros((32, 16, 3, 3), np.float32), None, "cpu")       # all zero: nothing to lose
        native.ConvWeights(_weights(cvm.W_MIN / 2), None, "cpu", reduced=True)      # one part: 11 bits by choice
    with pytest.warns(RuntimeWarning):
        native.ConvWeights(_weights(cvm.W_MIN / 2, (32, 16, 1, 1)), None, "cpu")    # the pointwise kernel reads the same image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        monkeypatch.setenv("SURS_CONV_SPLIT", "bf16x3")
        native.ConvWeights(_weights(cvm.W_MIN / 2), None, "cpu")                    # the bf16 x 3 image
        monkeypatch.setenv("SURS_CONV_SPLIT", "f16x2")
        monkeypatch.setenv("SURS_CONV_X3", "0")
        native.ConvWeights(_weights(cvm.W_MIN / 2), None, "cpu")                    # no split image at all


def test_the_synthetic_checkpoint_does_not_warn(monkeypatch):
    monkeypatch.delenv("SURS_CONV_SPLIT", raising=False)
    sd = common.state_dict()
    convs = [(k, v) for k, v in sd.items() if isinstance(v, np.ndarray) and v.ndim == 4 and v.shape[2] in (1, 3)]
    assert len(convs) > 50
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for k, v in convs:
            native.ConvWeights(v, None, "cpu")
    print("synthetic checkpoint: smallest max |w| over %d convolutions %.3g (W_MIN %.3g)" % (len(convs), min(np.abs(v).max() for _, v in convs),
                                                                                          cvm.W_MIN))
