"""What the convolution entry points compute from fp32 inputs, restated in float64 on the CPU (plain torch): the yardstick of
tests/test_gpu_conv_tiles.py, itself held to the C oracle by tests/test_conv_ref_host.py.  Images are numpy [C, H, W], weights
[cout, cin, k, k]; every function takes float32 or float64 arrays and returns float64."""
import numpy as np
import torch
import torch.nn.functional as F

from surs_amd import prng


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def conv2d(x, w, b=None, stride=1):
    """Zero-padded k x k convolution (k = 1, 3: padding k // 2), stride 1 or 2, with bias."""
    k = w.shape[2]
    y = F.conv2d(_t(x)[None], _t(w), _t(b) if b is not None else None, stride=stride, padding=k // 2)
    return y[0].numpy()


def relu(x):
    return np.maximum(np.asarray(x, np.float64), 0.0)


def lrelu(x, slope):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, np.float64(np.float32(slope)) * x)


def scale_shift_relu(x, scale, shift):
    """GroupNorm applied as explicit per-channel coefficients, then ReLU."""
    x = np.asarray(x, np.float64)
    return relu(x * np.asarray(scale, np.float64)[:, None, None] + np.asarray(shift, np.float64)[:, None, None])


def group_sums(x, groups=32):
    """[groups][2]: the sum and the sum of squares of each group's values."""
    v = np.asarray(x, np.float64).reshape(groups, -1)
    return np.stack([v.sum(1), (v * v).sum(1)], 1)


def group_norm_coeffs(x, gamma, beta, groups=32, eps=1e-5):
    """The per-channel scale and shift of GroupNorm(groups) from the statistics of x (biased variance, as torch.nn.GroupNorm)."""
    x = np.asarray(x, np.float64)
    c = x.shape[0]
    v = x.reshape(groups, -1)
    mean, var = v.mean(1), v.var(1)
    rstd = np.repeat(1.0 / np.sqrt(var + np.float64(np.float32(eps))), c // groups)
    scale = rstd * np.asarray(gamma, np.float64)
    return scale, np.asarray(beta, np.float64) - np.repeat(mean, c // groups) * scale


def group_norm(x, gamma, beta, groups=32, eps=1e-5):
    scale, shift = group_norm_coeffs(x, gamma, beta, groups, eps)
    return np.asarray(x, np.float64) * scale[:, None, None] + shift[:, None, None]


def conv(x, w, b=None, stride=1, in_scale=None, in_shift=None, gn=None, slope=None, residual=None):
    """One launch of the convolution entry points: [GroupNorm + ReLU ->] zero padding -> convolution + bias [-> LeakyReLU] [+ residual].
    The prologue is either explicit coefficients (in_scale, in_shift) or gn = (gamma, beta), normalising with x's own statistics; it
    comes before the padding, so a padded pixel is zero whatever the shift."""
    x = np.asarray(x, np.float64)
    if in_scale is not None:
        x = scale_shift_relu(x, in_scale, in_shift)
    elif gn is not None:
        x = relu(group_norm(x, *gn))
    y = conv2d(x, w, b, stride)
    if slope is not None:
        y = lrelu(y, slope)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y


def conv_block(x, wts, gns):
    """ConvBlock.forward with in_planes == out_planes (lib/model/HGFilters.py:57-74): three bias-free 3x3 convolutions, each behind
    GroupNorm(32) + ReLU, their outputs concatenated and added to the input.  Returns (o1, o2, o3, out)."""
    o1 = conv(x, wts[0], gn=gns[0])
    o2 = conv(o1, wts[1], gn=gns[1])
    o3 = conv(o2, wts[2], gn=gns[2])
    return o1, o2, o3, np.concatenate([o1, o2, o3]) + np.asarray(x, np.float64)


def inputs(tag, seed, cin, cout, h, w, k=3):
    """The seeded fp32 operands of one convolution case: x, weight, bias, residual (of the stride-1 output), in_scale, in_shift."""
    return dict(x=prng.uniform(tag + "x", seed, (cin, h, w), -1, 1),
                w=prng.uniform(tag + "w", seed, (cout, cin, k, k), -0.2, 0.2),
                b=prng.uniform(tag + "b", seed, (cout,), -0.5, 0.5),
                res=prng.uniform(tag + "r", seed, (cout, h, w), -1, 1),
                scale=prng.uniform(tag + "s", seed, (cin,), 0.5, 1.5),
                shift=prng.uniform(tag + "h", seed, (cin,), -0.3, 0.3))
