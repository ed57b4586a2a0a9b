"""tests/conv_ref.py (the float64 reference of the GPU tile tests) against the C oracle's fp32 conv2d / group_norm / relu / lrelu: 2e-5
of the output range, the bound the GPU tests then hold the kernels to against conv_ref."""
import numpy as np

import common
import conv_ref
import oracle
from surs_amd import prng


def test_stride1_ragged_with_bias_lrelu_and_residual():
    d = conv_ref.inputs("h1", 1, 16, 24, 13, 37)
    ref = oracle.lrelu(oracle.conv2d(d["x"], d["w"], d["b"]), 0.2) + d["res"]
    got = conv_ref.conv(d["x"], d["w"], d["b"], slope=0.2, residual=d["res"])
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert common.rel_err(got, ref) < 2e-5
    assert common.rel_err(conv_ref.conv2d(d["x"], d["w"]), oracle.conv2d(d["x"], d["w"])) < 2e-5
    # 1x1
    w1 = prng.uniform("h1p", 1, (40, 16, 1, 1), -0.2, 0.2)
    assert common.rel_err(conv_ref.conv2d(d["x"], w1, d["b"][:1].repeat(40)), oracle.conv2d(d["x"], w1, d["b"][:1].repeat(40))) < 2e-5


def test_stride2_odd_sizes():
    d = conv_ref.inputs("h2", 2, 32, 48, 33, 47)
    ref = oracle.conv2d(d["x"], d["w"], d["b"], 2)
    got = conv_ref.conv(d["x"], d["w"], d["b"], stride=2)
    assert got.shape == ref.shape == (48, 17, 24)
    assert common.rel_err(got, ref) < 2e-5


def test_groupnorm_prologue_in_both_forms_and_the_conv_block():
    d = conv_ref.inputs("h3", 3, 64, 32, 11, 19)
    x = d["x"] * 2 + 0.5
    gamma, beta = prng.uniform("h3g", 3, (64,), 0.5, 1.5), prng.uniform("h3b", 3, (64,), -0.3, 0.3)
    normed = oracle.relu(oracle.group_norm(x, gamma, beta))
    assert common.rel_err(conv_ref.relu(conv_ref.group_norm(x, gamma, beta)), normed) < 2e-5
    ref = oracle.conv2d(normed, d["w"], d["b"])
    assert common.rel_err(conv_ref.conv(x, d["w"], d["b"], gn=(gamma, beta)), ref) < 2e-5
    # explicit coefficients: the same normalisation handed over as scale / shift; the padding stays zero (a shift does not leak in)
    scale, shift = conv_ref.group_norm_coeffs(x, gamma, beta)
    assert common.rel_err(conv_ref.conv(x, d["w"], d["b"], in_scale=scale, in_shift=shift), ref) < 2e-5
    assert np.allclose(conv_ref.group_sums(x)[:, 0].sum(), x.astype(np.float64).sum(), rtol=1e-12)
    # ConvBlock
    xb = prng.uniform("h3x", 4, (128, 7, 9), -2, 3)
    wts = [prng.uniform("h3w", i, s, -0.1, 0.1) for i, s in enumerate(((64, 128, 3, 3), (32, 64, 3, 3), (32, 32, 3, 3)))]
    gns = [(prng.uniform("h3c", i, (n,), 0.5, 1.5), prng.uniform("h3d", i, (n,), -0.3, 0.3)) for i, n in enumerate((128, 64, 32))]
    o1 = oracle.conv2d(oracle.relu(oracle.group_norm(xb, *gns[0])), wts[0])
    o2 = oracle.conv2d(oracle.relu(oracle.group_norm(o1, *gns[1])), wts[1])
    o3 = oracle.conv2d(oracle.relu(oracle.group_norm(o2, *gns[2])), wts[2])
    got = conv_ref.conv_block(xb, wts, gns)
    assert common.rel_err(got[3], np.concatenate([o1, o2, o3]) + xb) < 2e-5
    assert common.rel_err(got[2], o3) < 2e-5
