"""The encoder's map-sized kernels (the second half of csrc/surs_encoder.hip) in each of their forms against tests/map_ref.py: average
pooling, bicubic enlargement, pixel shuffle, the two- and three-way sums, scale-shift-act, the layout conversions, GroupNorm
coefficients and the forms that leave GroupNorm statistics - at the map sizes, channel counts, pitches and base addresses at which the
entry points choose another kernel or a kernel takes another path.

Images are built as tests/test_gpu_sr_grads.py builds them: a buffer with the wanted channel pitch and NaN in every gap.  After every
call the gaps of the output are still NaN and the inputs are untouched; whenever two variants or two forms of one call can both run,
their values are bit-equal.  Maps are seeded with prng.uniform; where only the order of fp32 additions is at stake (pooling, the sums)
they are products of two such maps (_v), because sums of prng.uniform(-1, 1)'s multiples of 2^-23 are exact in any order.

Bounds.  Where the file claims bits (pooling, shuffle, sums, layouts) the fp32 restatement of map_ref, bit for bit.  Bicubic, per
tensor:  max |t - t64| <= 8 max(e_ref, 2^-22) max |t64|  (map_ref.bicubic_reference: e_ref is torch's own CPU fp32 distance from its
float64; tests/test_map_ref_host.py shows that a correct fp32 evaluation stays within half of it and that six wrong ones exceed it ten
times and more).  Pooling against the float64 mean: one rounding per addition, 3 * 2^-24 of the mean magnitude of the four values
(map_ref.avgpool2_bound).  Scale-shift-act: 2^-23 (|x scale| + |t64|), a fused or an unfused multiply-add.  GroupNorm coefficients:
2^-22 of the largest coefficient - the kernels sum in double and round once.  Every test prints its worst ratio before it asserts."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import map_ref as mr
from surs_amd import prng

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
KINDS = ("c", "c+4", "c+1", "base+1", "slice4", "slice1")
#  c       ld = c
#  c+4     ld = c + 4: keeps the 16-byte form
#  c+1     ld = c + 1: forces the scalar form where c % 4 == 0
#  base+1  ld = c, the base one float into its allocation: the scalar form as well
#  slice4  channels [4, 4 + c) of an image twice as wide (Img.slice): the 16-byte form
#  slice1  channels [1, 1 + c) of it: the scalar form
ALIGNED = ("c", "c+4", "c+8", "slice4")          # the kinds that keep 16-byte rows when c % 4 == 0 (c+8: the adds' third operand)
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 2), (5, 7), (18, 26)]


def _nat():
    from surs_amd import native
    return native


def _dev():
    import gpu_common as g
    return g.dev()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _u(tag, seed, shape, lo=-1.0, hi=1.0):
    return prng.uniform("enc_maps_" + tag, seed, shape, lo, hi)


def _v(tag, seed, shape):
    """Values off the 2^-23 grid of prng.uniform(-1, 1) (on it fp32 sums are exact and no order of additions shows): the product of
    two seeded maps, magnitudes over a factor of 16, the low bits of the rounded product."""
    return (_u(tag + "_m", seed, shape) * _u(tag + "_s", seed, shape, 0.25, 4.0)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Placed:
    """A [C, H, W] array on the device as an NHWC image of one of KINDS, NaN everywhere else in its allocation."""

    def __init__(self, a, kind="c"):
        native = _nat()
        c, h, w = a.shape
        self.c, self.h, self.w, self.kind = c, h, w, kind
        self.lead, self.c0, self.ld = 0, 0, c
        if kind in ("c+4", "c+8", "c+1", "c+3"):
            self.ld = c + int(kind[2:])
        elif kind == "base+1":
            self.lead = 1
        elif kind in ("slice4", "slice1"):
            self.ld, self.c0 = 2 * c, int(kind[5:])
            assert self.c0 + c <= self.ld
        else:
            assert kind == "c"
        rows = np.full((h * w, self.ld), NAN, np.float32)
        rows[:, self.c0:self.c0 + c] = mr.to_nhwc(np.ascontiguousarray(a, np.float32))
        self.host = np.concatenate([np.full(self.lead, NAN, np.float32), rows.reshape(-1)])
        self.buf = torch.from_numpy(self.host.copy()).to(_dev())
        if self.c0:
            self.img = native.Img(h, w, self.ld, self.ld, self.buf).slice(self.c0, c)
        else:
            self.img = native.Img(h, w, c, self.ld, self.buf, self.lead)
        assert (self.img.off, self.img.ld, self.img.c) == (self.lead + self.c0, self.ld, c)

    def aligned(self):
        return self.c % 4 == 0 and self.ld % 4 == 0 and (self.buf.data_ptr() + 4 * self.img.off) % 16 == 0

    def untouched(self):
        return np.array_equal(_bits(self.buf.cpu().numpy()), _bits(self.host))

    def values(self):
        """[C, H, W] as it stands on the device; asserts that everything else in the allocation is still NaN."""
        flat = self.buf.cpu().numpy()
        rows = flat[self.lead:].reshape(self.h * self.w, self.ld)
        gap = np.ones(rows.shape, bool)
        gap[:, self.c0:self.c0 + self.c] = False
        assert np.isnan(rows[gap]).all() and np.isnan(flat[:self.lead]).all(), "the call wrote into a gap (%s)" % self.kind
        return mr.from_nhwc(rows, self.h, self.w, self.c, self.c0)


def _out(c, h, w, kind):
    return Placed(np.full((c, h, w), NAN, np.float32), kind)


def _kinds(c):
    return [k for k in KINDS if k != "slice4" or c >= 4]


def _in_kind(kind):
    return "c" if kind.startswith("slice") else kind      # (the inputs of a call that writes a slice are plain)


def _check_dispatch(c, placed, kind):
    """The variant is the form it is meant to be: 16-byte rows or not."""
    fits = all(p.aligned() for p in placed)
    assert fits == (c % 4 == 0 and kind in ALIGNED), (c, kind)
    return fits


# ------------------------------------------------------------------ pooling
@pytest.mark.parametrize("c", [3, 4, 64])
@pytest.mark.parametrize("h,w", [(2, 2), (3, 5), (5, 4), (7, 2), (18, 26)])
def test_pooling(h, w, c):
    native = _nat()
    x = _v("pool", h * 31 + w + c, (c, h, w))
    want, t64, bound = mr.avgpool2_f32(x), mr.avgpool2(x), mr.avgpool2_bound(x)
    assert want.shape == (c, h // 2, w // 2)
    # the inputs tell the stated order from another one
    v = x[:, :h // 2 * 2, :w // 2 * 2]
    assert not _same_bits(want, ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * np.float32(0.25))
    worst = float((np.abs(want - t64) / bound).max())
    print("pooling %d x %d x %d: worst ratio to the float64 bound %.3f" % (c, h, w, worst))
    forms = set()
    for kind in _kinds(c):
        X, Y = Placed(x, _in_kind(kind)), _out(c, h // 2, w // 2, kind)
        forms.add(_check_dispatch(c, (X, Y), kind))
        native.avgpool2(X.img, out=Y.img)
        got = Y.values()
        assert X.untouched(), kind
        assert _same_bits(got, want), (kind, np.abs(got - want).max())      # (so every variant equals every other, bit for bit)
        assert np.all(np.abs(got - t64) <= bound)
    assert forms == ({True, False} if c % 4 == 0 else {False})


# ------------------------------------------------------------------ bicubic
_bicubic_refs = {}


def _bicubic_case(h, w, c, factor, align, with_addend):
    """Seeded operands and (t64, bound), computed once."""
    key = (h, w, c, factor, align, with_addend)
    if key not in _bicubic_refs:
        x = _u("bic", h * 31 + w + c, (c, h, w))
        ad = _u("bica", h * 31 + w + c + factor, (c, factor * h, factor * w)) if with_addend else None
        _bicubic_refs[key] = (x, ad) + mr.bicubic_reference(x, factor, align, ad)
    return _bicubic_refs[key]


@contextlib.contextmanager
def _option(name, value):
    """Library option `name` at `value`; the value read before is restored on the way out."""
    native = _nat()
    before = native.get_option(name)
    native.set_option(name, value)
    try:
        yield
    finally:
        native.set_option(name, before)


@pytest.mark.parametrize("c", [3, 4, 32, 64])
@pytest.mark.parametrize("h,w", SHAPES)
def test_bicubic_x2_in_every_form(h, w, c):
    native = _nat()
    worst, launches = 0.0, {"plain": 0, "up": 0, "block": 0, "stats1": 0, "stats0": 0}
    for align in (False, True):
        for with_addend in (False, True):
            x, ad, t64, bound = _bicubic_case(h, w, c, 2, align, with_addend)
            first = None
            for kind in _kinds(c):
                ops = [Placed(x, _in_kind(kind))] + ([Placed(ad, "c+4" if kind == "c" else _in_kind(kind))] if with_addend else [])
                A = ops[1].img if with_addend else None
                outs = [_out(c, 2 * h, 2 * w, kind)]
                fits = _check_dispatch(c, ops + outs, kind)
                forms = [("plain", lambda Y: native.bicubic_up2(ops[0].img, align, addend=A, out=Y)),
                         ("up", lambda Y: native.bicubic_up(ops[0].img, 2, align, addend=A, out=Y))]
                if fits:
                    forms.append(("block", lambda Y: native.bicubic_up2_block(ops[0].img, align, addend=A, out=Y)))
                if fits and c % 32 == 0:
                    forms.append(("stats1", lambda Y: native.bicubic_up2(ops[0].img, align, addend=A, out=Y, want_stats=True)))
                    forms.append(("stats0", forms[-1][1]))
                for name, fn in forms:
                    Y = _out(c, 2 * h, 2 * w, kind)
                    if name.startswith("stats"):
                        with _option("bicubic_block", int(name[-1])):
                            assert fn(Y.img).stats.slots >= 1
                    else:
                        fn(Y.img)
                    got = Y.values()
                    assert all(p.untouched() for p in ops), (name, kind)
                    launches[name] += 1
                    if first is None:
                        first = got
                        assert np.isfinite(got).all()
                        worst = max(worst, float(np.abs(got - t64).max() / bound))
                    assert _same_bits(got, first), (name, kind, align, with_addend, np.abs(got - first).max())
    print("bicubic x2 %d x %d x %d: worst ratio to the bound %.3f; launches %s" % (c, h, w, worst, launches))
    assert launches["block"] == (0 if c % 4 else 12) and launches["stats1"] == launches["stats0"] == (12 if c % 32 == 0 else 0)
    assert worst <= 1.0


@pytest.mark.parametrize("factor", [1, 3, 4])
@pytest.mark.parametrize("h,w", SHAPES)
def test_bicubic_other_factors(h, w, factor):
    native = _nat()
    worst = 0.0
    for c in (3, 8):
        for align in (False, True):
            for with_addend in (False, True):
                x, ad, t64, bound = _bicubic_case(h, w, c, factor, align, with_addend)
                first = None
                for kind in _kinds(c):
                    X, Y = Placed(x, _in_kind(kind)), _out(c, factor * h, factor * w, kind)
                    A = Placed(ad, "c+4" if kind == "c" else _in_kind(kind)) if with_addend else None
                    native.bicubic_up(X.img, factor, align, addend=A.img if A else None, out=Y.img)
                    got = Y.values()
                    assert X.untouched() and (A is None or A.untouched()), kind
                    if first is None:
                        first = got
                        assert np.isfinite(got).all()
                        worst = max(worst, float(np.abs(got - t64).max() / bound))
                    assert _same_bits(got, first), (kind, align, with_addend)
                if factor == 1:      # the input's bits (its only non-zero weight is 1)
                    assert _same_bits(first, mr.add_f32(ad, x) if with_addend else x)
    print("bicubic x%d %d x %d: worst ratio to the bound %.3f" % (factor, h, w, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------ pixel shuffle
@pytest.mark.parametrize("c4", [4, 8, 16, 48, 64])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5)])
def test_pixel_shuffle(h, w, c4):
    native = _nat()
    x = _u("ps", h * 31 + w + c4, (c4, h, w))
    x.reshape(-1)[::7] = 0.0
    x.reshape(-1)[3::11] = -0.0
    c = c4 // 4
    vec = set()
    for slope in (0.2, 0.0, 1.0):
        want = mr.pixel_shuffle2_lrelu_f32(x, slope)
        zeros = want == 0
        assert np.signbit(want[zeros]).any() and (slope == 0.0 or not np.signbit(want[zeros]).all())
        for kind in _kinds(c):
            # (c4 = 16 at a pitch of 17 is kind c+1; the form is chosen by the input's quads and both images' rows)
            X, Y = Placed(x, _in_kind(kind)), _out(c, 2 * h, 2 * w, kind)
            vec.add(c4 % 16 == 0 and X.aligned() and Y.aligned())
            native.pixel_shuffle2(X.img, slope, out=Y.img)
            got = Y.values()
            assert X.untouched(), kind
            assert _same_bits(got, want), (kind, slope)      # the sign of zero included
    assert vec == ({True, False} if c4 % 16 == 0 else {False})


# ------------------------------------------------------------------ the sums
ADD_KINDS = [("c", "c+4", "c+8", k) for k in KINDS] + [("c+1", "c", "c+4", "c"), ("base+1", "c+4", "c", "c+4"), ("c", "c", "c+1", "c")]


@pytest.mark.parametrize("c", [3, 4, 64])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (18, 26)])       # 1, 15 and 468 pixels
def test_add(h, w, c):
    native = _nat()
    a, b, d = (_v("add%d" % i, h * 31 + w + c, (c, h, w)) for i in range(3))
    assert not _same_bits(mr.add_f32(a, b, d), a + (b + d))      # the inputs tell (a + b) + c from a + (b + c)
    forms = set()
    for three in (False, True):
        want = mr.add_f32(a, b, d if three else None)
        assert np.all(np.abs(want - mr.add(a, b, d if three else None)) <= 2.0 ** -23 * (np.abs(a) + np.abs(b) + np.abs(d)))
        for ka, kb, kd, ko in ADD_KINDS:
            if ko == "slice4" and c < 4:
                continue
            ops = [Placed(a, ka), Placed(b, kb)] + ([Placed(d, kd)] if three else [])
            Y = _out(c, h, w, ko)
            forms.add(all(p.aligned() for p in ops + [Y]))
            native.add3(ops[0].img, ops[1].img, ops[2].img if three else None, out=Y.img)
            got = Y.values()
            assert all(p.untouched() for p in ops), (ka, kb, kd, ko)
            assert _same_bits(got, want), (three, ka, kb, kd, ko)
    assert forms == ({True, False} if c % 4 == 0 else {False})


# ------------------------------------------------------------------ scale-shift-act
@pytest.mark.parametrize("c", [4, 64])
@pytest.mark.parametrize("h,w", [(3, 5), (18, 26)])
def test_scale_shift_act(h, w, c):
    native, dev = _nat(), _dev()
    x = _u("ssx", h * 31 + w + c, (c, h, w), -2, 2)
    scale, shift = _u("sss", c, (c,), 0.5, 1.5), _u("ssh", c, (c,), -0.3, 0.3)
    scale[1::4] *= -1.0
    sc, sh = torch.from_numpy(scale).to(dev), torch.from_numpy(shift).to(dev)
    bound = mr.scale_shift_bound(x, scale, shift)
    worst = 0.0
    for relu in (False, True):
        t64 = mr.scale_shift_act(x, scale, shift, False)
        first = None
        for kind in _kinds(c):
            X, Y = Placed(x, _in_kind(kind)), _out(c, h, w, kind)
            native.scale_shift_act(X.img, sc, sh, relu, out=Y.img)
            got = Y.values()
            assert X.untouched() and np.array_equal(sc.cpu().numpy(), scale) and np.array_equal(sh.cpu().numpy(), shift)
            first = got if first is None else first
            assert _same_bits(got, first), kind
        if relu:      # (max(., 0) moves two numbers no further apart: the same bound against the float64 ReLU)
            assert (t64 < 0).any() and (t64 > 0).any()
            assert np.all(first >= 0) and not np.signbit(first[t64 > 0]).any()
            t64 = mr.scale_shift_act(x, scale, shift, True)
        err = np.abs(first - t64)
        worst = max(worst, float((err / bound).max()))
        print("scale-shift-act %d x %d x %d relu=%d: worst ratio to 2^-23 (|x scale| + |t64|) %.3f" % (c, h, w, relu, worst))
        assert np.all(err <= bound)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize("c", [1, 3, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5)])
def test_layouts(h, w, c):
    native, dev = _nat(), _dev()
    x = _u("lay", h * 31 + w + c, (c, h, w))
    t = torch.from_numpy(x[None]).to(dev)
    for ld in (c, c + 3):
        img = native.Img.from_nchw(t, ld if ld != c else None)
        assert (img.h, img.w, img.c, img.ld) == (h, w, c, ld)
        rows = img.buf.cpu().numpy().reshape(h * w, ld)
        assert _same_bits(rows[:, :c], mr.to_nhwc(x))
        back = img.to_nchw()
        assert tuple(back.shape) == (1, c, h, w) and _same_bits(back[0].cpu().numpy(), x)      # the round trip is the identity
        # into an image whose gaps are NaN, and back out of it
        Y = _out(c, h, w, "c" if ld == c else "c+3")
        native.check(native.lib().surs_nchw_to_nhwc(C.c_void_p(t.data_ptr()), c, h, w, Y.img.ptr(), Y.img.ld, _st()))
        torch.cuda.synchronize()
        assert _same_bits(Y.values(), x) and np.array_equal(t.cpu().numpy()[0], x)
        assert _same_bits(Y.img.to_nchw()[0].cpu().numpy(), x) and _same_bits(Y.values(), x)
    for kind in ("slice1", "base+1") + (("slice4",) if c >= 4 else ()):      # to_nchw from a slice, and from an odd base
        X = Placed(x, kind)
        assert _same_bits(X.img.to_nchw()[0].cpu().numpy(), x) and X.untouched()


# ------------------------------------------------------------------ GroupNorm coefficients
GN_CASES = [(4, 1, 1), (4, 4, 7), (32, 32, 1), (64, 32, 480), (96, 32, 511), (96, 32, 513), (48, 4, 9), (128, 64, 100), (1024, 32, 5)]
GN_BOUND = 2.0 ** -22


def _gn_inputs(c, groups, hw):
    maps = [("uniform", _u("gnx", c + hw, (c, hw, 1), -2, 3))]
    if (c, groups, hw) in ((64, 32, 480), (96, 32, 513)):
        maps.append(("offset", (np.float32(64) + _u("gno", c + hw, (c, hw, 1), -1.0 / 16, 1.0 / 16)).astype(np.float32)))
        maps.append(("constant", np.full((c, hw, 1), 2.5, np.float32)))
    return maps


def _coeffs_both_entries(X, c, hw, groups, gamma_d, beta_d, eps=1e-5):
    """(scale, shift) through native.groupnorm_coeffs (surs_groupnorm_coeffs_ws) after asserting that surs_groupnorm_coeffs, with
    the library's own scratch, gives the same bits."""
    native = _nat()
    sc, sh = native.groupnorm_coeffs(X.img, gamma_d, beta_d, groups=groups, eps=eps)
    sc2, sh2 = torch.full_like(sc, float("nan")), torch.full_like(sh, float("nan"))
    native.check(native.lib().surs_groupnorm_coeffs(X.img.ptr(), hw, c, X.img.ld, groups, eps, C.c_void_p(gamma_d.data_ptr()),
                                                    C.c_void_p(beta_d.data_ptr()), C.c_void_p(sc2.data_ptr()),
                                                    C.c_void_p(sh2.data_ptr()), _st()))
    sc, sh, sc2, sh2 = (t.cpu().numpy() for t in (sc, sh, sc2, sh2))
    assert _same_bits(sc, sc2) and _same_bits(sh, sh2)
    return sc, sh


@pytest.mark.parametrize("c,groups,hw", GN_CASES)
def test_groupnorm_coefficients(c, groups, hw):
    dev = _dev()
    gamma, beta = _u("gng", c, (c,), 0.5, 1.5), _u("gnb", c, (c,), -0.3, 0.3)
    gamma[1::3] *= -1.0
    gd, bd = torch.from_numpy(gamma).to(dev), torch.from_numpy(beta).to(dev)
    for name, x in _gn_inputs(c, groups, hw):
        scale64, shift64 = mr.group_norm_coeffs(x, gamma, beta, groups)
        first = None
        for kind in ("c", "c+4"):
            X = Placed(x, kind)
            assert X.aligned()
            sc, sh = _coeffs_both_entries(X, c, hw, groups, gd, bd)
            assert X.untouched() and np.isfinite(sc).all() and np.isfinite(sh).all()
            first = (sc, sh) if first is None else first
            assert _same_bits(sc, first[0]) and _same_bits(sh, first[1])
        sc, sh = first
        r_sc = float(np.abs(sc - scale64).max() / np.abs(scale64).max())
        r_sh = float(np.abs(sh - shift64).max() / np.abs(shift64).max())
        print("GroupNorm coefficients (%d, %d, %d) %s: scale %.3f, shift %.3f of 2^-22 of the largest" % (c, groups, hw, name, r_sc / GN_BOUND,
                                                                                                     r_sh / GN_BOUND))
        assert r_sc <= GN_BOUND and r_sh <= GN_BOUND
        if name == "constant":      # a variance of exactly 0: scale = gamma / sqrt(eps)
            assert np.allclose(scale64, gamma.astype(np.float64) / np.sqrt(np.float64(np.float32(1e-5))), rtol=1e-15, atol=0)


def test_groupnorm_coefficients_refusals():
    """What the host-side checks refuse, with their messages; nothing is launched: the outputs, NaN beforehand, stay NaN."""
    native, dev = _nat(), _dev()
    err = native._lib.SursError
    rows = "channels and pitch must be multiples of 4"
    x = torch.zeros(1028 * 8 + 4, dtype=torch.float32, device=dev)
    gamma = torch.ones(1028, dtype=torch.float32, device=dev)
    scratch = torch.empty(native.lib().surs_groupnorm_scratch_bytes(), dtype=torch.uint8, device=dev)
    for c, groups, ld, off, msg in ((6, 2, 8, 0, rows), (1028, 4, 1028, 0, rows), (64, 32, 64, 1, rows), (64, 32, 65, 0, rows),
                                    (64, 24, 64, 0, "bad GroupNorm shape"), (64, 0, 64, 0, "bad GroupNorm shape")):
        for ws in (False, True):
            sc, sh = (torch.full((1028,), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
            args = [C.c_void_p(x.data_ptr() + 4 * off), 8, c, ld, groups, 1e-5] + [C.c_void_p(t.data_ptr()) for t in (gamma, gamma, sc, sh)]
            fn = native.lib().surs_groupnorm_coeffs_ws if ws else native.lib().surs_groupnorm_coeffs
            with pytest.raises(err, match=msg):
                native.check(fn(*(args + ([C.c_void_p(scratch.data_ptr())] if ws else []) + [_st()])))
            torch.cuda.synchronize()
            assert torch.isnan(sc).all() and torch.isnan(sh).all()


# ------------------------------------------------------------------ the forms that leave statistics: the grid-stride loop
SENTINEL = -12345.0


def _stats_call(op, c, ops, Y, capacity, align=False):
    """One of the three *_gn entry points through the C ABI with an explicit capacity.  Returns (slots, the statistics buffer)."""
    native = _nat()
    lib = native.lib()
    st = torch.full((32 * 512 * 2 + 64,), SENTINEL, dtype=torch.float64, device=_dev())
    slots = C.c_int(-1)
    tail = [Y.img.ptr(), Y.img.ld, C.c_void_p(st.data_ptr()) if capacity is not None else None, capacity or 1, C.byref(slots), _st()]
    X = ops[0].img
    if op == "pool":
        rc = lib.surs_avgpool2_gn(X.ptr(), X.h, X.w, c, X.ld, *tail)
    elif op == "bicubic":
        A = ops[1].img if len(ops) > 1 else None
        rc = lib.surs_bicubic_up2_gn(X.ptr(), X.h, X.w, c, X.ld, int(align), A.ptr() if A else None, A.ld if A else 0, *tail)
    else:
        B, D = ops[1].img, ops[2].img if len(ops) > 2 else None
        rc = lib.surs_add3_gn(X.ptr(), X.ld, B.ptr(), B.ld, D.ptr() if D else None, D.ld if D else 0, X.h * X.w, c, *tail)
    native.check(rc)
    torch.cuda.synchronize()
    return slots.value, st.cpu().numpy()


def _stats_ops(op, c, h, w, kind):
    """Operands (input size h x w), the output's size, the plain call, work items of the one-output forms and of the block form."""
    native = _nat()
    if op == "pool":
        ops = [Placed(_v("stp", c + h, (c, h, w)), kind)]
        return ops, (h // 2, w // 2), lambda Y: native.avgpool2(ops[0].img, out=Y.img), (h // 2) * (w // 2) * (c // 4), None
    if op == "bicubic":
        ops = [Placed(_u("stb", c + h, (c, h, w)), kind), Placed(_u("stba", c + h, (c, 2 * h, 2 * w)), "c+4")]
        return (ops, (2 * h, 2 * w), lambda Y: native.bicubic_up2(ops[0].img, True, addend=ops[1].img, out=Y.img), 4 * h * w * (c // 4),
                h * w * (c // 4))
    ops = [Placed(_v("sta%d" % i, c + h, (c, h, w)), k) for i, k in enumerate((kind, "c+4", "c"))]
    return ops, (h, w), lambda Y: native.add3(ops[0].img, ops[1].img, ops[2].img, out=Y.img), h * w * (c // 4), None


def _stats_case(op, c, h, w, capacities, block):
    ops, (ho, wo), plain, items, block_items = _stats_ops(op, c, h, w, "c+4")
    P = _out(c, ho, wo, "slice4")
    plain(P)
    want = P.values()
    threads, n = (512, block_items) if (op == "bicubic" and block) else (1024, items)
    seen = []
    for cap in capacities:
        Y = _out(c, ho, wo, "slice4")
        slots, st = _stats_call(op, c, ops, Y, cap, align=True)
        assert slots == min(cap, -(-n // threads), 512), (op, cap, slots)
        seen.append(slots)
        got = Y.values()
        assert all(p.untouched() for p in ops)
        assert _same_bits(got, want), (op, cap, block)
        used = 32 * slots * 2
        assert np.all(st[used:] == SENTINEL), "the statistics buffer was written beyond its %d slots" % slots
        folded = st[:used].reshape(32, slots, 2).sum(1)
        sums = mr.group_sums(got)
        assert np.allclose(folded, sums, rtol=1e-12, atol=1e-9), (op, cap, np.abs(folded - sums).max())
    return n, threads, seen


@pytest.mark.parametrize("op,block", [("pool", None), ("add", None), ("bicubic", 1), ("bicubic", 0)])
def test_statistics_forms_grid_stride_loop(op, block):
    """2080 items of four channels at c = 32 (pooling a 40 x 26 map, enlarging a 5 x 13 one, adding 10 x 26 ones).  The one-output
    forms' workgroups take 1024 items a trip, two trips at a time: capacity 1 - one workgroup, a pair of items and then a single one
    (and nothing for the threads past item 2079); capacity 2 - a pair whose second item only 32 threads have; capacity 8 - three
    workgroups of one item, the last nearly empty.  The block form has 520 items (input pixels x quads) for workgroups of 512."""
    h, w = {"pool": (40, 26), "bicubic": (5, 13), "add": (10, 26)}[op]
    with _option("bicubic_block", 1 if block is None else block):
        n, threads, seen = _stats_case(op, 32, h, w, (1, 2, 8), block)
    assert (n, threads, seen) == ((520, 512, [1, 2, 2]) if block else (2080, 1024, [1, 2, 3]))


@pytest.mark.parametrize("op,block", [("pool", None), ("add", None), ("bicubic", 1), ("bicubic", 0)])
def test_statistics_forms_at_1024_channels(op, block):
    """c = 1024 on a 2 x 2 input: 256 quads a pixel, so four pixel lanes per workgroup of 1024 (two per 512 of the block form) and
    half or more of the fold's eight sub-lanes idle."""
    with _option("bicubic_block", 1 if block is None else block):
        n, threads, seen = _stats_case(op, 1024, 2, 2, (1, 8), block)
    assert seen == [1, min(8, -(-n // threads))]


def test_statistics_forms_refusals():
    native = _nat()
    err = native._lib.SursError
    for op, (h, w) in (("pool", (4, 6)), ("bicubic", (2, 3)), ("add", (2, 3))):
        for block in (1, 0):
            with _option("bicubic_block", block):
                for c, cap, msg in ((48, 4, "power of two in \\[32, 1024\\]"), (32, None, "null statistics buffer")):
                    ops, (ho, wo), _, _, _ = _stats_ops(op, c, h, w, "c")
                    Y = _out(c, ho, wo, "c")
                    with pytest.raises(err, match=msg):
                        _stats_call(op, c, ops, Y, cap)
                    assert np.isnan(Y.values()).all()
