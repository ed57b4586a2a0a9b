"""The encoder's map-sized operations (the second half of csrc/surs_encoder.hip: average pooling, bicubic enlargement, pixel shuffle,
the two- and three-way sums, scale-shift-act, the layout conversions, GroupNorm coefficients and statistics) restated in plain numpy:
the yardsticks of tests/test_gpu_encoder_maps.py, themselves held to torch's CPU float64 and the C oracle by
tests/test_map_ref_host.py.

Two kinds.  The float64 functions are written from the operation's formula and take float32 or float64 arrays.  The `_f32` functions
restate what a kernel claims bit for bit - every operation rounded to float32 once, in the kernel's stated order - and take float32.
bicubic_f32 / bicubic_block_f32 restate the bicubic kernels the same way, but only the host test uses them (that the bound admits a
correct kernel and catches a wrong one): the device contracts multiply-adds, so its bits differ.  Images are numpy [C, H, W]."""
import numpy as np

F32 = np.float32
CUBIC_A = -0.75          # torch's upsample_bicubic2d


def _f64(a):
    return np.asarray(a, np.float64)


# ------------------------------------------------------------------ float64, from the formulas
def avgpool2(x):
    """The mean of every whole 2 x 2 block: sizes floor(h / 2), floor(w / 2), an odd last row and column dropped."""
    x = _f64(x)
    ho, wo = x.shape[1] // 2, x.shape[2] // 2
    v = x[:, :2 * ho, :2 * wo]
    return (v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]) / 4.0


def cubic_kernel(d, A=CUBIC_A):
    """Keys' cubic convolution kernel W(d) at the distances d >= 0."""
    d = np.abs(_f64(d))
    near = ((A + 2.0) * d - (A + 3.0)) * d * d + 1.0
    far = ((A * d - 5.0 * A) * d + 8.0 * A) * d - 4.0 * A
    return np.where(d <= 1.0, near, np.where(d < 2.0, far, 0.0))


def source_coordinate(n_in, factor, align_corners):
    """The source coordinate of every destination index 0 .. factor n_in - 1 (float64): dst (n_in - 1) / (n_out - 1) with aligned
    corners, (dst + 1/2) / factor - 1/2 without (not clamped at 0: the taps are)."""
    n_out = factor * n_in
    dst = np.arange(n_out, dtype=np.float64)
    if align_corners:
        return dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    return (dst + 0.5) / factor - 0.5


def _taps64(n_in, factor, align_corners, A):
    r = source_coordinate(n_in, factor, align_corners)
    i0 = np.floor(r)
    t = r - i0
    idx = [np.clip(i0.astype(np.int64) - 1 + a, 0, n_in - 1) for a in range(4)]
    wts = [cubic_kernel(t + 1.0, A), cubic_kernel(t, A), cubic_kernel(1.0 - t, A), cubic_kernel(2.0 - t, A)]
    return idx, wts


def bicubic_up(x, factor, align_corners, addend=None, A=CUBIC_A):
    """torch's upsample_bicubic2d by an integer factor: four border-clamped taps per axis around floor(source coordinate)."""
    x = _f64(x)
    iy, wy = _taps64(x.shape[1], factor, align_corners, A)
    ix, wx = _taps64(x.shape[2], factor, align_corners, A)
    rows = sum(wy[a][None, :, None] * x[:, iy[a], :] for a in range(4))
    y = sum(wx[b][None, None, :] * rows[:, :, ix[b]] for b in range(4))
    return y if addend is None else _f64(addend) + y


def pixel_shuffle2(x):
    """nn.PixelShuffle(2): out[c, 2 i + di, 2 j + dj] = in[4 c + 2 di + dj, i, j]."""
    x = np.asarray(x)
    c4, h, w = x.shape
    out = np.empty((c4 // 4, 2 * h, 2 * w), x.dtype)
    for di in range(2):
        for dj in range(2):
            out[:, di::2, dj::2] = x[2 * di + dj::4]
    return out


def pixel_shuffle2_lrelu(x, slope):
    v = pixel_shuffle2(_f64(x))
    return np.where(v > 0, v, np.float64(F32(slope)) * v)


def add(a, b, c=None):
    y = _f64(a) + _f64(b)
    return y if c is None else y + _f64(c)


def scale_shift_act(x, scale, shift, relu):
    t = _f64(x) * _f64(scale)[:, None, None] + _f64(shift)[:, None, None]
    return np.maximum(t, 0.0) if relu else t


def group_norm_coeffs(x, gamma, beta, groups=32, eps=1e-5):
    """GroupNorm's per-channel scale and shift by the two-pass definition: the group's mean, then the (biased) variance about it;
    scale = gamma rstd, shift = beta - mean scale."""
    x = _f64(x)
    c = x.shape[0]
    cg = c // groups
    v = x.reshape(groups, -1)        # (a group is cg consecutive channels)
    mean = v.sum(1) / v.shape[1]
    var = ((v - mean[:, None]) ** 2).sum(1) / v.shape[1]
    rstd = 1.0 / np.sqrt(var + np.float64(F32(eps)))
    scale = _f64(gamma) * np.repeat(rstd, cg)
    return scale, _f64(beta) - np.repeat(mean, cg) * scale


def group_sums(x, groups=32):
    """[groups][2]: the sum and the sum of squares of each group's values."""
    v = _f64(x).reshape(groups, -1)
    return np.stack([v.sum(1), (v * v).sum(1)], 1)


# ------------------------------------------------------------------ fp32, in the kernels' stated order (bit for bit)
def _is32(*arrays):
    for a in arrays:
        assert a is None or a.dtype == np.float32, "float32 expected"


def avgpool2_f32(x, row_pitch_defect=False):
    """(((x00 + x01) + x10) + x11) * 0.25f, read from the row-major pixels the way the kernels address them: pixel (2 oy) w + 2 ox, its
    right neighbour, and the two a row of w pixels further.  row_pitch_defect: the lower row taken 2 (w / 2) pixels further instead (a
    defect for the host test: wrong for an odd w)."""
    _is32(x)
    c, h, w = x.shape
    ho, wo = h // 2, w // 2
    flat = x.reshape(c, h * w)
    pitch = 2 * wo if row_pitch_defect else w
    p = ((2 * np.arange(ho))[:, None] * w + 2 * np.arange(wo)[None, :]).reshape(-1)
    y = (((flat[:, p] + flat[:, p + 1]) + flat[:, p + pitch]) + flat[:, p + pitch + 1]) * F32(0.25)
    return y.reshape(c, ho, wo)


def pixel_shuffle2_lrelu_f32(x, slope):
    """v > 0 ? v : slope * v on the shuffled map (a zero of either sign goes through the product: slope * -0 keeps its sign)."""
    _is32(x)
    v = pixel_shuffle2(x)
    return np.where(v > 0, v, F32(slope) * v).astype(np.float32)


def add_f32(a, b, c=None):
    """(a + b) + c."""
    _is32(a, b, c)
    y = a + b
    return y if c is None else y + c


def to_nhwc(x, ld=None, fill=np.nan):
    """[C, H, W] -> the NHWC buffer [H W, ld] with `fill` in the gap: a plain copy."""
    c, h, w = x.shape
    buf = np.full((h * w, c if ld is None else ld), fill, x.dtype)
    buf[:, :c] = x.transpose(1, 2, 0).reshape(h * w, c)
    return buf


def from_nhwc(buf, h, w, c, c0=0):
    """Channels [c0, c0 + c) of an NHWC buffer [H W, ld] -> [C, H, W]: a plain copy."""
    return np.ascontiguousarray(buf[:, c0:c0 + c].reshape(h, w, c).transpose(2, 0, 1))


# ---- the bicubic kernels in fp32 (host test only)
def cubic_coeffs_f32(t, A=CUBIC_A):
    """cubic_coeffs of the kernels: the four weights at fraction t, Horner forms with every operation rounded."""
    A = F32(A)
    one, two, three, four, five, eight = (F32(v) for v in (1, 2, 3, 4, 5, 8))
    x = t + one
    c0 = ((A * x - five * A) * x + eight * A) * x - four * A
    x = t
    c1 = ((A + two) * x - (A + three)) * x * x + one
    x = one - t
    c2 = ((A + two) * x - (A + three)) * x * x + one
    x = two - t
    c3 = ((A * x - five * A) * x + eight * A) * x - four * A
    return [c0, c1, c2, c3]


def _coords_f32(n_in, factor, align_corners, phase_defect=False):
    """floor and fraction of the source coordinate as the kernels form them: aligned, (float)(n_in - 1) / (float)(n_out - 1) * dst;
    otherwise (float)(1 / factor) * (dst + 0.5f) - 0.5f with a separately rounded multiply and subtract (for factor 2 both are exact, so a
    contracted multiply-add gives the same).  phase_defect: the coordinate from the exact phase dst mod factor, whatever the alignment."""
    n_out = factor * n_in
    dst = np.arange(n_out, dtype=np.float32)
    if phase_defect:
        d = np.arange(n_out)
        r = ((d // factor) + ((d % factor) + 0.5) / factor - 0.5).astype(np.float32)
    elif align_corners:
        r = (F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)) * dst
    else:
        r = F32(1.0 / factor) * (dst + F32(0.5)) - F32(0.5)
    i0 = np.floor(r)
    return i0.astype(np.int64), (r - i0).astype(np.float32)


BICUBIC_DEFECTS = ("clamp_hi", "no_lo_clamp", "A", "phase")


def bicubic_f32(x, factor, align_corners, addend=None, defect=None):
    """One output per item, as bicubic_up2_kernel / BicubicUp2Op / bicubic_up_kernel: r_a = sum_b cx[b] x[yy_a, xx_b] in order from 0,
    acc = sum_a cy[a] r_a in order from 0, then addend + acc.  defect (host test): "clamp_hi" - the rows' upper clamp at h - 2;
    "no_lo_clamp" - no lower clamp, a tap below 0 reads zero; "A" - A = -0.5; "phase" - the coordinate from dst mod factor."""
    _is32(x, addend)
    assert defect is None or defect in BICUBIC_DEFECTS
    c, h, w = x.shape
    A = -0.5 if defect == "A" else CUBIC_A
    iy, ty = _coords_f32(h, factor, align_corners, defect == "phase")
    ix, tx = _coords_f32(w, factor, align_corners, defect == "phase")
    cy, cx = cubic_coeffs_f32(ty, A), cubic_coeffs_f32(tx, A)
    acc = np.zeros((c, factor * h, factor * w), np.float32)
    for a in range(4):
        yy = iy - 1 + a
        ylow = yy < 0
        yy = np.maximum(np.minimum(yy, h - 2 if defect == "clamp_hi" else h - 1), 0)
        r = np.zeros_like(acc)
        for b in range(4):
            xx = ix - 1 + b
            xlow = xx < 0
            xx = np.clip(xx, 0, w - 1)
            v = x[:, yy][:, :, xx]
            if defect == "no_lo_clamp":
                v = np.where(ylow[None, :, None] | xlow[None, None, :], F32(0), v)
            r = r + cx[b][None, None, :] * v
        acc = acc + cy[a][None, :, None] * r
    return acc if addend is None else addend + acc


def bicubic_block_f32(x, align_corners, addend=None, column_defect=False):
    """Factor 2 as bicubic_block_kernel / bicubic_block_stats_kernel: one item per input pixel (by, bx) = the 2 x 2 outputs (2 by + d,
    2 bx + g) from ONE 5 x 5 window anchored at the first output's taps; the second row / column of outputs reads the window one
    further where its own floor is (dy, dx = 0 or 1).  column_defect (host test): the second column always from v[b]."""
    _is32(x, addend)
    c, h, w = x.shape
    iy, ty = _coords_f32(h, 2, align_corners)
    ix, tx = _coords_f32(w, 2, align_corners)
    cy, cx = cubic_coeffs_f32(ty), cubic_coeffs_f32(tx)
    iy0, ix0 = iy[0::2], ix[0::2]
    dy, dx = iy[1::2] - iy0, ix[1::2] - ix0
    assert set(np.unique(dy)) <= {0, 1} and set(np.unique(dx)) <= {0, 1}
    if column_defect:
        dx = np.zeros_like(dx)
    rows = [np.clip(iy0 - 1 + k, 0, h - 1) for k in range(5)]
    cols = [np.clip(ix0 - 1 + m, 0, w - 1) for m in range(5)]
    r = []                                       # r[k][g]: [c, h, w], horizontal sums of window row k for output column g
    for k in range(5):
        v = [x[:, rows[k]][:, :, cols[m]] for m in range(5)]
        r0 = np.zeros((c, h, w), np.float32)
        r1 = np.zeros((c, h, w), np.float32)
        for b in range(4):
            u = np.where((dx == 1)[None, None, :], v[b + 1], v[b])
            r0 = r0 + cx[b][0::2][None, None, :] * v[b]
            r1 = r1 + cx[b][1::2][None, None, :] * u
        r.append((r0, r1))
    out = np.empty((c, 2 * h, 2 * w), np.float32)
    for d in range(2):
        for g in range(2):
            acc = np.zeros((c, h, w), np.float32)
            for a in range(4):
                rr = np.where(((dy == 1) & (d == 1))[None, :, None], r[a + 1][g], r[a][g])
                acc = acc + cy[a][d::2][None, :, None] * rr
            out[:, d::2, g::2] = acc
    return out if addend is None else addend + out


# ------------------------------------------------------------------ the bicubic bound
BOUND_FACTOR, BOUND_FLOOR = 8.0, 2.0 ** -22      # the factor and the floor of the project's other float64 comparisons


def torch_bicubic(x, factor, align_corners, dtype):
    """torch's own CPU kernel: F.interpolate(mode="bicubic") on the map in `dtype`."""
    import torch
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)[None]
    return F.interpolate(t, scale_factor=factor, mode="bicubic", align_corners=bool(align_corners))[0].numpy()


def bicubic_reference(x, factor, align_corners, addend=None):
    """(t64, bound): the float64 value and the absolute bound  8 max(e_ref, 2^-22) max |t64|  a float32 result is held to.  e_ref is
    the distance of torch's CPU fp32 kernel from its float64 one on the same input, as a fraction of max |t64|; an addend is added to
    both (its own rounding is covered by the floor)."""
    import torch
    t64 = bicubic_up(x, factor, align_corners, addend)
    ref32 = torch_bicubic(x, factor, align_corners, torch.float32)
    ref64 = torch_bicubic(x, factor, align_corners, torch.float64)
    if addend is not None:
        ref32, ref64 = addend + ref32, _f64(addend) + ref64
    e_ref = float(np.abs(_f64(ref32) - ref64).max() / np.abs(ref64).max())
    return t64, BOUND_FACTOR * max(e_ref, BOUND_FLOOR) * float(np.abs(t64).max())


# ------------------------------------------------------------------ the other bounds (derived)
def avgpool2_bound(x):
    """Elementwise bound of (((x00 + x01) + x10) + x11) * 0.25f against the float64 mean: three additions, each rounded to float32 once
    (relative 2^-24 of a partial sum that is at most the sum of the magnitudes), the multiplication by 1/4 exact -
    3 * 2^-24 * (|x00| + |x01| + |x10| + |x11|) / 4."""
    return 3.0 * 2.0 ** -24 * avgpool2(np.abs(_f64(x)))


def scale_shift_bound(x, scale, shift):
    """Elementwise bound of x * scale + shift in float32, fused or not (two roundings at most): 2^-23 (|x scale| + |t64|)."""
    p = _f64(x) * _f64(scale)[:, None, None]
    return 2.0 ** -23 * (np.abs(p) + np.abs(p + _f64(shift)[:, None, None]))
