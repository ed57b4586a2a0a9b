"""What the encoder's split-operand convolutions SHOULD compute: a numpy model (no GPU, no product code) of ONE launch of the
convolution entry points on conv_x3_kernel<KS, STRIDE, TR, NT3, NP> (3x3, stride 1 or 2; NP = 2 f16 parts per operand, 1 f16 part,
3 bf16 parts) and conv1x1_x2_kernel<CT> (pointwise, two f16 parts), written from the kernels' sources in the manner of
tests/column_model.py, whose Rounding, bf16_round, f16_truncate and k-step accumulation it builds on.  It rounds exactly where the
sources round and forms exactly the partial products they form; everything else is accumulation, run either in float64 (the
reference form) or in fp32 with every 16-channel MFMA step as one addend, in the kernels' order or its reverse (the measure of what a
summation order may change - not a claim about bits; the small tile's three accumulators, (acc0 + acc1) + acc2, are one more ordering
inside the same band and are not modelled).  A correct kernel differs from the float64 model by accumulation order only.
tests/test_conv_model_host.py checks the model, tests/test_gpu_conv_model.py holds the kernels to it.

("enc" below = csrc/surs_encoder.hip of the package, "pack" = csrc/surs_pack.cpp, "gather" = csrc/surs_repack_gather.h.)

    prologue    none, or v = max(fp32(fp32(x * scale) + shift), 0): multiply and add rounded separately (the library is built
                with -ffp-contract=off; enc `stage`, and the pointwise kernel's loop); a padded pixel is zero AFTER it
    splits      activations: hi = f16(v), lo = f16(fp32(v - hi)), the remainder exact in fp32 (ConvSplit<2>::split); hi alone
                (ConvSplit<1>); the three bf16 parts of split3 (ConvSplit<3>).  Weights as the packers split them (pack
                surs_conv_pack_weights_x2 / _x3, gather rp_split2 / rp_split3): round to nearest even, subnormal results kept
    products    x_lo w_hi, x_hi w_lo, x_hi w_hi (enc PA / PB; the pointwise kernel's three MFMA groups); x_hi w_hi alone;
                x3 w1, x2 w2, x1 w3, x2 w1, x1 w2, x1 w1 of three parts - per chunk of 16 channels and tap, chunks and taps ascending
    epilogue    + bias, LeakyReLU with the fp32 slope, + residual: an fp32 rounding each
    the pipe    keeps f16 subnormal operands but does not normalise them: the fp32 forms cut a step's products 24 bits below its
                largest encoded exponent where a hi part is subnormal (_aligned: measured on gfx950, not read from a source)

Every function returns float64.  Rounding(on=False) makes every rounding point the identity: the model is then conv_ref.conv.
A change to a rounding point of these kernels must change this file in the same commit.

The two-part form's window (the grade table of DESIGN.md 4.5, measured by test_conv_model_host.py against the exact float64
convolution, never against a kernel): lo is a subnormal f16 once |v| < 2^-3 and gone below 2^-14, so each operand carries an
absolute error of 2^-25, and a tensor of magnitude m loses 2^-25 / m of the output range.  W_MIN below is derived from that table."""
import numpy as np

import column_model as cm
import conv_ref
from repack_common import PLANTED

TOL = {2: 2e-5, 1: 2e-3}      # of the output range against the exact convolution: the bounds of tests/test_gpu_conv_tiles.py
TOL3 = 2.0 ** -22             # three bf16 parts, on every finite rung
# The smallest power of two such that a weight tensor with max |w| >= W_MIN stays under TOL[2] / 2 on the ladder's weight axis
# (the factor 2: margin for other shapes - the error is a maximum over elements).  On that axis the two-part error is
# c 2^-25 / max |w| of the range with c = 0.91 .. 1.02 on the table's two shapes (uniform weights, max |w| = 0.2 x scale:
# 3.6e-5 at 0.2 x 2^-8, 6.2e-4 at 0.2 x 2^-12): 1.02 2^-25 / m <= 1e-5 from m >= 3.1e-3, and the next power of two is 2^-8.
# test_conv_model_host.py::test_grade_table derives the same value from its own numbers and asserts it equals this one.
W_MIN = 2.0 ** -8
# ... and the activations' end of the window by the same law (c = 1.1 on the activation axis): the smallest power-of-two scale of a
# uniform activation tensor at which two parts still hold TOL[2] itself; the ladder pins 2^-6 inside and 2^-10 outside
X_MIN_SCALE = 2.0 ** -9

# (activation scale, weight scale) applied to conv_ref.inputs-style operands (x uniform +-1, w +-0.2)
LADDER = [(2.0 ** 14, 1.0), (1.0, 1.0), (2.0 ** -6, 1.0), (2.0 ** -10, 1.0), (2.0 ** -14, 1.0), (2.0 ** -20, 1.0), (1.0, 2.0 ** -8),
          (1.0, 2.0 ** -12), (2.0 ** -10, 2.0 ** -8)]
SHORT = [(1.0, 1.0), (2.0 ** -10, 1.0), (1.0, 2.0 ** -8)]
# kind -> k, stride, cin, cout, h, w.  3x3: three 16-channel chunks (the tail of the two-chunk loop), a whole and a ragged channel
# tile of 64 (three of 32), 11 rows = two 4-row tiles + 3 = one 8-row tile + 3, columns 32 + 8; stride 2: output 6 x 21.  1x1: 165
# pixels = a whole 128-pixel block and a ragged one, conv1x1_x2_kernel<4> (cout_pad % 256 == 0) and <1>.  "g": 64 input channels
# (the GroupNorm-statistics prologue needs cin % 32 == 0; four chunks).
KINDS = {"s1": (3, 1, 48, 96, 11, 40), "s2": (3, 2, 48, 96, 11, 41), "p4": (1, 1, 48, 256, 5, 33), "p1": (1, 1, 48, 64, 5, 33),
         "s1g": (3, 1, 64, 96, 11, 40), "p4g": (1, 1, 64, 256, 5, 33), "p1g": (1, 1, 64, 64, 5, 33)}
SLOPE = 0.2


def rung_name(rung):
    return "(2^%d, 2^%d)" % (int(np.log2(rung[0])), int(np.log2(rung[1])))


# ------------------------------------------------------------------ the rounding points
class Rounding(cm.Rounding):
    """column_model's rounding points (h(): bf16, the type of the three-part form; f16(): the type of the other two) and the
    convolutions' splits.  The perturbations of test_conv_model_host.py: trunc_act - the activation parts converted towards zero;
    flush - f16 subnormal parts (of both operands: what a matrix pipe that flushes would see) become zero; double_rem - the
    activations' remainder through a bf16 rounding before its f16 one."""

    def __init__(self, on=True, trunc_act=False, flush=False, double_rem=False):
        super().__init__("bf16", on, trunc_act)
        self.flush, self.double_rem = flush, double_rem

    def part16(self, x, act):
        """One f16 part.  act: an activation (converted in the kernel) and not a weight (converted by the packer)."""
        if not self.on:
            return np.asarray(x, np.float64)
        if act and self.trunc_act:
            y = cm.f16_truncate(np.asarray(x, np.float64).astype(np.float32)).astype(np.float64)
        else:
            y = self.f16(x)
        if self.flush:
            y = np.where(np.abs(y) < 2.0 ** -14, 0.0, y)
        return y

    def split_f16(self, v, nparts, act):
        """[hi] or [hi, lo]: ConvSplit<1> / ConvSplit<2>::split (enc), rp_split2 (gather)."""
        hi = self.part16(v, act)
        if nparts == 1:
            return [hi]
        if not self.on:
            return [hi, np.zeros_like(hi)]
        with np.errstate(invalid="ignore"):
            r = self.f(v - hi)                       # fmaf(hi, -1, x): exact (hi = +-inf: -+inf, as the instruction gives)
        if act and self.double_rem:
            r = self.h(r)
        return [hi, self.part16(r, act)]

    def split(self, v, nparts, act):
        return self.split3(v) if nparts == 3 else self.split_f16(v, nparts, act)


# (activation part, weight part) of every product, in the kernels' order: smallest first (enc PA / PB)
PRODUCTS = {1: [(0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 3: [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]}


F16_MIN = 2.0 ** -14          # the smallest normal f16


def _encoded_exponent(v):
    """The exponent an f16 value is ENCODED with: floor(log2 |v|), -14 for a subnormal; a large negative number for zero."""
    m, e = np.frexp(v)
    return np.where(v == 0, -10000, np.maximum(e - 1, -14))


def _aligned(W, X):
    """sum_k W[:, k] X[k] as ONE step of the f16 matrix pipe forms it for operands it does not normalise (measured on gfx950 through
    conv1x1_x2_kernel, NOTES.md "conv model"): every product of the step is cut - towards zero - 24 bits below the largest ENCODED
    product exponent of the step, ea + eb, where a subnormal f16 is encoded with exponent -14 whatever its leading zeros.  With
    normal operands the cut lies at or below the last bit of the largest product, inside what an fp32 accumulator drops anyway;
    a subnormal operand with z leading zeros loses z bits.  Measured: the cut, its direction (on positive products) and its anchor
    for two products in a step.  Supposed: one anchor for all 16 products of a step, the accumulator taking no part in it."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        # (in float32: a product of two f16 values is exact there, and so is what the cut leaves of it)
        prod = W.astype(np.float32)[:, :, None] * X.astype(np.float32)[None]
        E = (_encoded_exponent(W).astype(np.int32)[:, :, None] + _encoded_exponent(X).astype(np.int32)[None]).max(1)
        q = np.ldexp(np.float32(1.0), np.clip(E - 24, -120, 120))[:, None, :]
        out = (np.trunc(prod / q) * q).sum(1, dtype=np.float64)
    plain = W @ X
    return np.where(np.isfinite(out), out, plain)


def _subnormal(v):
    return (v != 0) & (np.abs(v) < F16_MIN)


def _accumulate(xp, wp, parts, stride, ho, wo, acc, order, lose=None):
    """xp: the activation parts [cin_pad, hp, wp] (padded), wp: the weight parts [cout, cin_pad, k, k].  One addend per chunk of 16
    channels, tap and product.  lose = (chunk, tap): the first product (x_lo w_hi) of that step is missing.
    The fp32 forms take a step through _aligned() for the pixels whose HI activation part and the output channels whose HI weight
    part hold a subnormal f16 in the step: there the un-normalised operands cost significant bits.  Where only the lo parts are
    subnormal (every |v| < 2^-3) the cut lies 2^-38 |other operand| deep, under 2^-24 of the step's leading product x_hi w_hi as
    long as that one's operands are normal: those steps are plain sums.  Three bf16 parts: bf16 has fp32's exponents, no such
    regime.  The float64 form is the exact sum of the products everywhere (the reference form)."""
    cout, cin_pad, k, _ = wp[0].shape
    steps = [(s, t, n) for s in range(cin_pad // 16) for t in range(k * k) for n in range(len(PRODUCTS[parts]))]
    if order == "desc":
        steps = steps[::-1]
    a = np.zeros((cout, ho * wo), np.float64 if acc is np.float64 else np.float32)
    align = acc is np.float32 and parts != 3

    def window(q, s, ky, kx):
        return q[16 * s:16 * s + 16, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride].reshape(16, ho * wo)

    for s, t, n in steps:
        if lose == (s, t) and n == 0:
            continue
        i, j = PRODUCTS[parts][n]
        ky, kx = divmod(t, k)
        X, W = window(xp[i], s, ky, kx), wp[j][:, 16 * s:16 * s + 16, ky, kx]
        p = W @ X
        if align:
            cols = np.flatnonzero(_subnormal(window(xp[0], s, ky, kx)).any(0))
            rows = np.flatnonzero(_subnormal(wp[0][:, 16 * s:16 * s + 16, ky, kx]).any(1))
            if cols.size:
                p[:, cols] = _aligned(W, X[:, cols])
            if rows.size:
                p[rows] = _aligned(W[rows], X)
        a += p if acc is np.float64 else p.astype(np.float32)
    return a.astype(np.float64).reshape(cout, ho, wo)


def conv(x, w, b=None, stride=1, in_scale=None, in_shift=None, slope=None, residual=None, parts=2, acc=np.float64, order="asc",
         rounding=True, pert=None):
    """One launch: x [cin, h, w], w [cout, cin, k, k] (k = 1, 3) of fp32 values; in_scale / in_shift [cin]: the prologue's
    coefficients, explicit or as the library folded them from GroupNorm statistics.  pert: the perturbations of
    test_conv_model_host.py - "trunc", "flush", "double_rem" (Rounding), "lose" = (chunk, tap), "fused_prologue",
    "pad_first", "bias_f16"."""
    pert = dict(pert or {})
    R = Rounding(rounding, trunc_act=bool(pert.get("trunc")), flush=bool(pert.get("flush")), double_rem=bool(pert.get("double_rem")))
    assert acc is np.float64 or (acc is np.float32 and order in ("asc", "desc"))
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    cout, cin, k, _ = w.shape
    pad = k // 2
    ho, wo = (x.shape[1] + 2 * pad - k) // stride + 1, (x.shape[2] + 2 * pad - k) // stride + 1
    cpad = -cin % 16
    border = ((0, cpad), (pad, pad), (pad, pad))

    def prologue(v):
        if in_scale is None:
            return v
        sc, sh = (np.asarray(c, np.float64)[:, None, None] for c in (in_scale, in_shift))
        t = R.f(v * sc + sh) if pert.get("fused_prologue") else R.f(R.f(v * sc) + sh)      # v * sc[q] + sh[q], contraction off
        return np.maximum(t, 0.0)                                                            # fmaxf(., 0.f)

    with np.errstate(invalid="ignore", over="ignore"):
        if pert.get("pad_first"):                    # the WRONG order: a padded pixel becomes max(shift, 0)
            xpad = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
            xparts = [np.pad(q, ((0, cpad), (0, 0), (0, 0))) for q in R.split(prologue(xpad), parts, True)]
        else:                                        # "zero padding is applied after the norm"
            xparts = [np.pad(q, border) for q in R.split(prologue(x), parts, True)]
        wparts = [np.pad(q, ((0, 0), (0, cpad), (0, 0), (0, 0))) for q in R.split(w, 2 if parts == 1 else parts, False)]
        t = _accumulate(xparts, wparts, parts, stride, ho, wo, acc, order, pert.get("lose"))
        if b is not None:
            b = np.asarray(b, np.float64)
            if pert.get("bias_f16"):
                b = R.f16(b)
            t = R.f(t + b[:, None, None])                                                    # t += b
        if slope is not None:
            t = np.where(t > 0, t, R.f(np.float64(np.float32(slope)) * t))                   # t > 0.f ? t : slope * t
        if residual is not None:
            t = R.f(t + np.asarray(residual, np.float64))                                    # t += rv[q]
    return t


# ------------------------------------------------------------------ the cases of tests/test_gpu_conv_model.py
def out_size(kind):
    k, stride, cin, cout, h, w = KINDS[kind]
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def operands(kind, rung, variant, plant=True, overflow=False):
    """The fp32 operands of a case.  variant "plain": convolution + bias of x scaled by the rung; "epi": in_scale / in_shift
    prologue + LeakyReLU(0.2) + residual; "gn": GroupNorm(gamma, beta) + ReLU in front (the coefficients come from the caller: the
    library's fold on the GPU, coeffs() below on the host).  With a prologue the rung scales its coefficients (gamma, beta), so the
    NORMALISED activation carries the magnitude.  Bias and residual are scaled by the product of both scales: every term of the
    output keeps the magnitude of the convolution's sum (left at +-0.5 and +-1 they would BE the output on the small rungs, and the
    bound, a fraction of the largest output, would no longer see the products).  plant: repack_common.PLANTED without its last
    element at fixed, sparse positions of x and w.  overflow: one activation of 65520 (f16 infinity) at the first pixel and one of
    65503.9 (finite) mid-map."""
    k, stride, cin, cout, h, w = KINDS[kind]
    ax, aw = (np.float32(v) for v in rung)
    d = conv_ref.inputs("m" + kind, 1, cin, cout, h, w, k)
    x, wt = d["x"].copy(), d["w"].copy()
    if plant:
        n = PLANTED.size - 1
        x.reshape(-1)[5 + 211 * np.arange(n)] = PLANTED[:n]
        wt.reshape(-1)[3 + 97 * np.arange(n)] = PLANTED[:n]
    if overflow:
        assert tuple(rung) == (1.0, 1.0) and variant == "plain"
        x[5, 0, 0], x[7, h // 2, w // 2] = 65520.0, 65503.9
    ho, wo = out_size(kind)
    out = dict(w=wt * aw, b=d["b"] * (ax * aw), stride=stride)
    if variant == "plain":
        out["x"] = x * ax
        return out
    out["x"] = x
    if variant == "epi":
        out.update(scale=d["scale"] * ax, shift=d["shift"] * ax, slope=SLOPE, res=np.ascontiguousarray(d["res"][:, :ho, :wo]) * (ax * aw))
    else:
        assert variant == "gn" and cin % 32 == 0
        out.update(gamma=d["scale"] * ax, beta=d["shift"] * ax)
    return out


def coeffs(op):
    """A "gn" case's coefficients where there is no library to fold them: float64 GroupNorm(32), stored fp32."""
    sc, sh = conv_ref.group_norm_coeffs(op["x"], op["gamma"], op["beta"])
    return sc.astype(np.float32), sh.astype(np.float32)


def model_args(op, scale=None, shift=None):
    """conv()'s arguments from a case's operands (scale, shift: a "gn" case's coefficients)."""
    if "gamma" in op:
        assert scale is not None
    else:
        scale, shift = op.get("scale"), op.get("shift")
    return dict(x=op["x"], w=op["w"], b=op["b"], stride=op["stride"], in_scale=scale, in_shift=shift, slope=op.get("slope"),
                residual=op.get("res"))


def exact(op, scale=None, shift=None):
    """The exact float64 convolution of a case: conv_ref.conv."""
    a = model_args(op, scale, shift)
    return conv_ref.conv(a["x"], a["w"], a["b"], a["stride"], in_scale=a["in_scale"], in_shift=a["in_shift"], slope=a["slope"],
                         residual=a["residual"])


def models(op, parts, scale=None, shift=None, pert=None):
    """(float64 model, [fp32 ascending, fp32 descending])."""
    a = model_args(op, scale, shift)
    return conv(parts=parts, pert=pert, **a), [conv(parts=parts, acc=np.float32, order=o, pert=pert, **a) for o in ("asc", "desc")]


# ------------------------------------------------------------------ the bound
def bounds(ref, forms, sel=None):
    """column_model.bounds' rule as it stands, over the output elements sel (all of them unless given): e = the larger distance of
    the two fp32-order forms to the float64 model, floor = 2^-22 max |model| (four fp32 roundings of the largest element: the floor
    for values read straight from the library), bound[s] = 8 max(s(e), floor) for s = mean, max, median."""
    sel = np.ones(ref.shape, bool) if sel is None else sel
    floor = np.full(int(sel.sum()), 2.0 ** -22 * np.abs(ref[sel]).max())
    return cm.bounds({"logit_y": ref}, [{"logit_y": f} for f in forms], "y", sel, floor)


def grade(y, ref):
    """The distance of y to ref as a fraction of ref's range: common.rel_err."""
    return float(np.abs(y - ref).max() / max(1e-300, np.abs(ref).max()))
