"""tests/map_ref.py (the references of tests/test_gpu_encoder_maps.py) on the CPU: its float64 functions against torch's CPU float64
operators (1e-12 of the map's maximum) and the C oracle (the tolerances of tests/test_gpu_encoder_ops.py), its fp32 restatements
against them, and the two sides of the bicubic bound  max |t - t64| <= 8 max(e_ref, 2^-22) max |t64|:  the fp32 restatement of the
kernels stays within half of it at every case of the GPU test's table, and the same restatement with one deliberate defect exceeds it
at least ten times at a named case of that table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import common
import map_ref as mr
import oracle
from surs_amd import prng

SHAPES = [(1, 1), (1, 5), (2, 3), (3, 2), (5, 7), (18, 26)]      # the bicubic table of tests/test_gpu_encoder_maps.py
POOL_SHAPES = [(2, 2), (3, 5), (5, 4), (7, 2), (18, 26)]


def _u(tag, seed, shape, lo=-1.0, hi=1.0):
    return prng.uniform("map_ref_host_" + tag, seed, shape, lo, hi)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def _close64(name, got, want):
    want = np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, name
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert err <= 1e-12, (name, err)


# ------------------------------------------------------------------ the references hold
@pytest.mark.parametrize("h,w", POOL_SHAPES)
def test_pooling_against_torch_and_the_oracle(h, w):
    x = _u("pool", h * 31 + w, (5, h, w))
    ref = mr.avgpool2(x)
    assert ref.shape == (5, h // 2, w // 2)
    _close64("avgpool2", ref, F.avg_pool2d(_t64(x)[None], 2, stride=2)[0].numpy())
    f32 = mr.avgpool2_f32(x)
    assert f32.dtype == np.float32 and np.array_equal(f32, oracle.avg_pool2(x))      # (the existing GPU test's tolerance: none)
    assert np.all(np.abs(f32 - ref) <= mr.avgpool2_bound(x))


@pytest.mark.parametrize("factor", [1, 2, 3, 4])
@pytest.mark.parametrize("align", [False, True])
def test_bicubic_against_torch_and_the_oracle(factor, align):
    for h, w in SHAPES:
        x = _u("bic", h * 31 + w, (3, h, w))
        ref = mr.bicubic_up(x, factor, align)
        _close64("bicubic %dx%d x%d" % (h, w, factor), ref, mr.torch_bicubic(x, factor, align, torch.float64))
        if factor == 1:
            assert np.array_equal(ref, x.astype(np.float64))
        if factor == 2:
            # the oracle computes in fp32: the restatement of the kernels at the existing GPU test's 1e-6 (it gives the oracle's bits),
            # the float64 value under the bound the kernels are held to (with aligned corners the fp32 coordinate sy * dst alone puts
            # the oracle, and torch's fp32 kernel with it, 2e-6 of the maximum from float64 at 18 x 26: e_ref carries that)
            orc = oracle.bicubic_up2(x, align)
            assert common.rel_err(mr.bicubic_f32(x, 2, align), orc) < 1e-6
            t64, bound = mr.bicubic_reference(x, 2, align)
            assert np.array_equal(t64, ref) and np.abs(orc - ref).max() <= bound
    ad = _u("bica", factor, (3, 5 * factor, 7 * factor))
    x = _u("bic", 5 * 31 + 7, (3, 5, 7))
    assert np.array_equal(mr.bicubic_up(x, factor, align, addend=ad), ad.astype(np.float64) + mr.bicubic_up(x, factor, align))


def test_pixel_shuffle_add_and_scale_shift_against_torch():
    x = _u("ps", 1, (48, 3, 5))
    x.reshape(-1)[::7] = 0.0
    x.reshape(-1)[3::11] = -0.0
    want = F.pixel_shuffle(_t64(x)[None], 2)[0]
    assert np.array_equal(mr.pixel_shuffle2(x), want.numpy().astype(np.float32))
    assert np.array_equal(mr.pixel_shuffle2(x), oracle.pixel_shuffle2(x))
    for slope in (0.2, 0.0, 1.0):
        s32 = float(np.float32(slope))
        _close64("shuffle", mr.pixel_shuffle2_lrelu(x, slope), F.leaky_relu(want, s32).numpy())
        got = mr.pixel_shuffle2_lrelu_f32(x, slope)
        assert got.dtype == np.float32 and np.array_equal(got, oracle.lrelu(oracle.pixel_shuffle2(x), slope))
        # one rounding of the float64 value; a zero keeps its sign through slope * v (slope >= 0)
        assert np.all(np.abs(got - mr.pixel_shuffle2_lrelu(x, slope)) <= 2.0 ** -24 * np.abs(got))
        z = mr.pixel_shuffle2(x) == 0
        assert z.any() and np.array_equal(np.signbit(got[z]), np.signbit(mr.pixel_shuffle2(x)[z]))
    a, b, c = (_u("add", i, (4, 3, 5)) for i in range(3))
    assert np.array_equal(mr.add(a, b, c), a.astype(np.float64) + b + c) and np.array_equal(mr.add(a, b), a.astype(np.float64) + b)
    assert np.array_equal(mr.add_f32(a, b, c), (a + b) + c) and mr.add_f32(a, b).dtype == np.float32
    assert np.all(np.abs(mr.add_f32(a, b, c) - mr.add(a, b, c)) <= 2.0 ** -23 * (np.abs(a) + np.abs(b) + np.abs(c)))
    sc, sh = _u("sc", 1, (4,), 0.5, 1.5), _u("sh", 1, (4,), -0.3, 0.3)
    t = mr.scale_shift_act(a, sc, sh, False)
    assert np.array_equal(t, a.astype(np.float64) * sc.astype(np.float64)[:, None, None] + sh.astype(np.float64)[:, None, None])
    assert np.array_equal(mr.scale_shift_act(a, sc, sh, True), F.relu(_t64(t)).numpy())
    # the bound admits the fused and the unfused fp32 evaluation
    unfused = a * sc[:, None, None] + sh[:, None, None]
    fused = (a.astype(np.float64) * sc.astype(np.float64)[:, None, None] + sh[:, None, None]).astype(np.float32)   # (product exact in double)
    for v in (unfused, fused):
        assert np.all(np.abs(v - t) <= mr.scale_shift_bound(a, sc, sh))


def test_layouts_are_plain_copies():
    x = _u("lay", 1, (5, 3, 4))
    buf = mr.to_nhwc(x, 8)
    assert buf.shape == (12, 8) and np.isnan(buf[:, 5:]).all()
    assert np.array_equal(buf[:, :5], torch.from_numpy(x).permute(1, 2, 0).reshape(12, 5).numpy())
    assert np.array_equal(mr.from_nhwc(buf, 3, 4, 5), x) and np.array_equal(mr.from_nhwc(buf, 3, 4, 2, c0=1), x[1:3])


@pytest.mark.parametrize("c,groups,hw", [(4, 1, 1), (4, 4, 7), (64, 32, 480), (96, 32, 513), (48, 4, 9)])
def test_groupnorm_coefficients_against_torch_and_the_oracle(c, groups, hw):
    x = _u("gn", c + hw, (c, hw, 1), -2, 3)
    gamma, beta = _u("gg", c, (c,), 0.5, 1.5), _u("gb", c, (c,), -0.3, 0.3)
    scale, shift = mr.group_norm_coeffs(x, gamma, beta, groups)
    got = mr.scale_shift_act(x, scale, shift, False)
    want = F.group_norm(_t64(x)[None], groups, _t64(gamma), _t64(beta), float(np.float32(1e-5)))[0].numpy()
    # (hw = 1 with one channel per group: the variance is 0, both sides are beta up to the cancellation of mean * scale)
    assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), np.abs(np.asarray(scale) * np.abs(x).max()).max())
    if hw > 1:
        assert common.rel_err(got, oracle.group_norm(x, gamma, beta, groups)) < 2e-5
    sums = mr.group_sums(x, groups)
    assert sums.shape == (groups, 2)
    xs = _t64(x).reshape(groups, -1)
    assert np.allclose(sums, torch.stack([xs.sum(1), (xs * xs).sum(1)], 1).numpy(), rtol=1e-13, atol=0)


# ------------------------------------------------------------------ the bound admits a correct kernel
@pytest.mark.parametrize("h,w", SHAPES)
def test_bound_admits_the_fp32_restatement(h, w):
    worst = 0.0
    for factor in (1, 2, 3, 4):
        x = _u("adm", h * 31 + w, (3, h, w))
        ad = _u("adma", h * 31 + w + factor, (3, factor * h, factor * w))
        for align in (False, True):
            for addend in (None, ad):
                t64, bound = mr.bicubic_reference(x, factor, align, addend)
                got = mr.bicubic_f32(x, factor, align, addend)
                assert got.dtype == np.float32 and got.shape == t64.shape
                worst = max(worst, float(np.abs(got - t64).max() / bound))
                if factor == 2:   # the block form is the same expression per output: the same bits, the 1-, 2- and 3-pixel maps included
                    assert np.array_equal(mr.bicubic_block_f32(x, align, addend), got)
                if factor == 1:
                    assert np.array_equal(mr.bicubic_f32(x, 1, align), x)
    print("bicubic %d x %d: the fp32 restatement's worst ratio to the bound %.3f" % (h, w, worst))
    assert worst <= 0.5


# ------------------------------------------------------------------ the bound catches a wrong kernel
DEFECTS = [   # name, (h, w, factor, align_corners): the case of the table that is named to catch it
    ("clamp_hi", (5, 7, 2, False)),        # the rows' upper clamp at h - 2 instead of h - 1
    ("no_lo_clamp", (1, 1, 2, False)),     # no lower clamp, a zero tap instead: the one-pixel map, where every tap is clamped
    ("A", (5, 7, 2, False)),               # A = -0.5
    ("block_column", (2, 3, 2, True)),     # the block form's second column from v[b] where dx = 1
    # the coordinate of factor 3 from the exact phase dst mod 3.  Without aligned corners that phase IS the float64 coordinate, so no
    # float64 comparison can object (it lies closer to float64 than the kernel does: ratio 0.07 at 18 x 26); what the shortcut gets
    # wrong is the aligned case, whose step is (h - 1) / (3 h - 1), not 1 / 3
    ("phase", (18, 26, 3, True)),
]


@pytest.mark.parametrize("name,case", DEFECTS)
def test_bound_catches_a_defect(name, case):
    h, w, factor, align = case
    assert (h, w) in SHAPES
    x = _u("adm", h * 31 + w, (3, h, w))
    t64, bound = mr.bicubic_reference(x, factor, align)
    if name == "block_column":
        bad = mr.bicubic_block_f32(x, align, column_defect=True)
    else:
        bad = mr.bicubic_f32(x, factor, align, defect=name)
    good = float(np.abs(mr.bicubic_f32(x, factor, align) - t64).max() / bound)
    ratio = float(np.abs(bad - t64).max() / bound)
    print("defect %s at %d x %d x%d align_corners=%s: %.3g times the bound (without it %.3f)" % (name, h, w, factor, align, ratio, good))
    assert good <= 0.5 and ratio >= 10.0


def test_pooling_bound_catches_the_row_pitch_of_an_even_width():
    """Pooling that reads row 2 oy + 1 at pitch (w / 2) * 2 instead of w: the same for an even w, a wrong pixel for an odd one."""
    h, w = 3, 5
    assert (h, w) in POOL_SHAPES
    x = _u("pool", h * 31 + w, (5, h, w))
    bound = mr.avgpool2_bound(x)
    ratio = float((np.abs(mr.avgpool2_f32(x, row_pitch_defect=True) - mr.avgpool2(x)) / bound).max())
    print("defect pooling row pitch at %d x %d: %.3g times the bound" % (h, w, ratio))
    assert ratio >= 10.0
    even = _u("pool", 5 * 31 + 4, (5, 5, 4))
    assert np.array_equal(mr.avgpool2_f32(even, row_pitch_defect=True), mr.avgpool2_f32(even))
