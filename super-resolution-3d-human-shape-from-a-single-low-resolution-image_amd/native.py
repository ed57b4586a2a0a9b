"""Thin torch-tensor wrappers over the C ABI (include/surs.h).

PyTorch is used for device memory and streams only; every function here hands raw
device pointers to libsurs_hip.so.  Tensors must live on the current CUDA (HIP)
device.  Nothing here computes on the CPU and nothing falls back.
"""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, settings
from ._lib import BF16, DTYPES, F16, F32, check, lib  # noqa: F401


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "device tensor expected"
    return C.c_void_p(t.data_ptr())


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), "contiguous float32 tensor expected"
    return t


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("surs_amd needs a HIP device (MI355X); there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def device_info():
    cu = C.c_int(0)
    arch = C.create_string_buffer(32)
    check(lib().surs_device_info(C.byref(cu), arch))
    return cu.value, arch.value.decode()


# ------------------------------------------------------------------ NHWC image tensors

class Img:
    """NHWC fp32 device image: a view (h, w, c) into a buffer with channel pitch ld."""
    __slots__ = ("buf", "h", "w", "c", "ld", "off", "stats")

    def __init__(self, h, w, c, ld=None, buf=None, off=0, device=None):
        ld = c if ld is None else ld
        if buf is None:
            buf = torch.empty(h * w * ld, dtype=torch.float32, device=device or require_gpu())
        self.buf, self.h, self.w, self.c, self.ld, self.off = buf, h, w, c, ld, off
        self.stats = None   # GnStats of exactly these values, if the kernel that wrote them left any (conv2d_gn, *_gn below)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def slice(self, c0, c):
        """channels [c0, c0+c) of the same pixels (the reference's torch.cat, in place)."""
        return Img(self.h, self.w, c, self.ld, self.buf, self.off + c0)

    def to_nchw(self):
        out = torch.empty((1, self.c, self.h, self.w), dtype=torch.float32, device=self.buf.device)
        check(lib().surs_nhwc_to_nchw(self.ptr(), self.c, self.h, self.w, self.ld, _ptr(out), _stream()))
        return out

    @staticmethod
    def from_nchw(t, ld=None):
        t = _f32c(t.reshape(t.shape[-3:]).contiguous())
        c, h, w = t.shape
        img = Img(h, w, c, ld, device=t.device)
        check(lib().surs_nchw_to_nhwc(_ptr(t), c, h, w, img.ptr(), img.ld, _stream()))
        return img


import contextlib
import threading

_wide = threading.local()


@contextlib.contextmanager
def wide_operands():
    """Everything computed inside runs its fp32-grade matrix products on three bf16 parts per operand (fp32's exponent range)
    instead of two f16 parts (|x| < 65504): the point / octree / multi-view kernels and the GEMMs behind the sweep through the
    calling thread's operand split (surs_set_operand_split_local), the encoder's 3x3 convolutions through ConvWeights'
    bf16 x 3 image (packed on first use).  What reconstruction() and SuRSNet.query_* repeat a computation under after it produced
    non-finite values - the reference is plain fp32 and has no such range limit."""
    prev = getattr(_wide, "on", False)
    _wide.on = True
    check(lib().surs_set_operand_split_local(3))
    try:
        yield
    finally:
        _wide.on = prev
        check(lib().surs_set_operand_split_local(3 if prev else 0))


def wide_operands_active():
    return getattr(_wide, "on", False)


@contextlib.contextmanager
def reduced_point_operands(on=True):
    """Inside, surs_query_points / surs_query_points_hr of this thread run ONE f16 product per MAC (one f16 part per operand: 11
    significant bits, a third of the matrix work of the fp32-grade point path): the arbitrary-point evaluator of `--precision bf16 |
    fp16` (SuRSNet.query_mr / query_sr).  No effect inside wide_operands() (the retry after an overflow is fp32-grade) or with
    on=False."""
    if not on or wide_operands_active():
        yield
        return
    check(lib().surs_set_operand_split_local(1))
    try:
        yield
    finally:
        check(lib().surs_set_operand_split_local(3 if wide_operands_active() else 0))


# The lower edge of the two-f16-part convolutions' window for weights: the second part of an operand below 2^-3 is a subnormal f16, so
# a weight carries an absolute error of 2^-25 and a tensor with max |w| = m loses 2^-25 / m of the output range.  CONV_W_MIN is the
# smallest power of two from which that stays under half the fp32-grade bound of 2e-5 (the grade table of DESIGN.md 4.5, derived in
# tests/conv_model.py and pinned by tests/test_conv_model_host.py).
CONV_W_MIN = 2.0 ** -8


def _warn_small_weights(w):
    """One RuntimeWarning for a weight tensor whose two-part image is not fp32 grade (ConvWeights; host only)."""
    peak = float(np.abs(w).max()) if w.size else 0.0
    if 0.0 < peak < CONV_W_MIN:
        import warnings
        warnings.warn("convolution weights %s with max |w| = %.3g < %.3g: as two f16 parts per operand they lose about %.1e of the "
                      "output range (2^-25 / max |w|; fp32 grade is 2e-5).  Pack them with SURS_CONV_SPLIT=bf16x3 or run the "
                      "computation inside native.wide_operands()." % (tuple(w.shape), peak, CONV_W_MIN, 2.0 ** -25 / peak),
                      RuntimeWarning, stacklevel=3)


class ConvWeights:
    """Packed conv weights ([tap][cin_pad][cout_pad]) + bias on the device."""

    def __init__(self, w, b, device, reduced=False):
        w = np.ascontiguousarray(w, np.float32)
        self._host_w, self._w3_wide = w, None
        self._master = self._table = None   # repack(): the device tensor the images were last packed from, and its one-item table
        self.reduced = bool(reduced)   # 3x3: one f16 product per MAC (surs_conv2d_nhwc_x1) - the encoder of --precision bf16 / fp16
        self.cout, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        n = lib().surs_conv_pack_weights(None, self.cout, self.cin, self.k, None)
        packed = np.empty(n, np.float32)
        lib().surs_conv_pack_weights(w.ctypes.data_as(C.c_void_p), self.cout, self.cin, self.k,
                                     packed.ctypes.data_as(C.c_void_p))
        self.w = torch.from_numpy(packed).to(device)
        self.b = torch.from_numpy(np.ascontiguousarray(b, np.float32)).to(device) if b is not None else None
        # split image for the 3x3 / stride-1 kernel: two f16 parts (surs_conv2d_nhwc_x2, default) or, with SURS_CONV_SPLIT=bf16x3,
        # three bf16 parts (surs_conv2d_nhwc_x3: fp32's exponent range); SURS_CONV_X3=0: neither (fp32 MFMA kernel).  1x1
        # convolutions have a two-part kernel only (conv1x1_x2_kernel); with three parts asked for they stay on the fp32 MFMA kernel
        self.w3, self.parts = None, 3 if settings.get("SURS_CONV_SPLIT").startswith("b") else 2
        if (self.k == 3 or (self.k == 1 and self.parts == 2)) and settings.get("SURS_CONV_X3") != "0":
            pack = lib().surs_conv_pack_weights_x3 if self.parts == 3 else lib().surs_conv_pack_weights_x2
            nb = pack(None, self.cout, self.cin, self.k, None)
            buf = np.empty(nb, np.uint8)
            pack(w.ctypes.data_as(C.c_void_p), self.cout, self.cin, self.k, buf.ctypes.data_as(C.c_void_p))
            self.w3 = torch.from_numpy(buf).to(device)
            if self.parts == 2 and not self.reduced:
                _warn_small_weights(w)

    def split_image(self):
        """(packed split weights, parts) for the 3x3 / stride-1 kernel; inside wide_operands() the bf16 x 3 image, packed on first use."""
        if self.w3 is None or self.parts == 3 or not wide_operands_active():
            return self.w3, self.parts
        if self.k == 1:
            return None, 0    # (1x1: the plain fp32 MFMA kernel is the wide form)
        if self._w3_wide is None:
            pack = lib().surs_conv_pack_weights_x3
            nb = pack(None, self.cout, self.cin, self.k, None)
            if self._master is not None:
                # (the values were committed on the device: repack(); the host copy is gone - pack from the device master.  Whoever
                # holds a table over this convolution sees the new image through wide_image_built() and takes it in)
                self._w3_wide = torch.empty(nb, dtype=torch.uint8, device=self.w.device)
                conv_repack(RepackTable([(self._master, self.cout, self.cin, self.k, None, None, self._w3_wide)], self.w.device))
                return self._w3_wide, 3
            buf = np.empty(nb, np.uint8)
            pack(self._host_w.ctypes.data_as(C.c_void_p), self.cout, self.cin, self.k, buf.ctypes.data_as(C.c_void_p))
            self._w3_wide = torch.from_numpy(buf).to(self.w.device)
        return self._w3_wide, 3

    def check_master(self, w_dev):
        """ValueError unless w_dev can be this convolution's device master; changes nothing."""
        if tuple(w_dev.shape) != (self.cout, self.cin, self.k, self.k) or w_dev.dtype != torch.float32 or not w_dev.is_contiguous() \
                or w_dev.device != self.w.device:
            raise ValueError("repack: a contiguous float32 [%d,%d,%d,%d] tensor on %s is expected, not %s %s on %s"
                             % (self.cout, self.cin, self.k, self.k, self.w.device, w_dev.dtype, tuple(w_dev.shape), w_dev.device))

    def repack_entry(self, w_dev):
        """This convolution's row of a RepackTable reading the plain [cout,cin,k,k] device tensor w_dev: the images the constructor
        packed - w, and w3 as two f16 or (SURS_CONV_SPLIT=bf16x3) three bf16 parts, none with SURS_CONV_X3=0; `reduced` reads part 0
        of the two-part image - plus the wide image where wide_operands() has already asked for it.  The object then packs a wide
        image it is asked for later from w_dev (kept, not copied: its host copy of the old values is dropped)."""
        self.check_master(w_dev)
        self._master, self._host_w = w_dev.detach(), None
        x2 = self.w3 if self.parts == 2 else None
        x3 = self.w3 if self.parts == 3 else self._w3_wide
        return (self._master, self.cout, self.cin, self.k, self.w, x2, x3)

    def repack(self, w_dev, b_dev=None):
        """Refreshes w, w3 (and the wide image, if it exists) and b IN PLACE from device tensors of new values: one surs_conv_repack
        of a one-item table on the current stream.  data_ptr() of every image stays, so a NativeNet or a captured graph that holds
        the raw pointers keeps reading valid - now updated - weights."""
        entry = self.repack_entry(w_dev)
        key = tuple(t.data_ptr() if t is not None else 0 for t in (entry[0],) + entry[4:])
        if self._table is None or self._table[0] != key:
            self._table = (key, RepackTable([entry], self.w.device))
        conv_repack(self._table[1])
        if b_dev is not None:
            if self.b is None:
                raise ValueError("repack: this convolution has no bias")
            self.b.copy_(b_dev.detach().reshape(-1))


class RepackTable:
    """A device table of SursRepackItem (include/surs.h) over entries (w, cout, cin, ksize, packed, x2, x3) of device tensors (the
    images nullable), with the tile prefix surs_conv_repack finds a workgroup's item by.  Built once: the addresses are constant."""

    def __init__(self, entries, device):
        items = (_lib.RepackItem * len(entries))()
        end = 0
        for it, (w, cout, cin, k, packed, x2, x3) in zip(items, entries):
            tiles = lib().surs_conv_repack_tiles(cout, cin, k)
            if tiles <= 0:
                raise ValueError("surs_conv_repack: a %dx%d convolution of %d -> %d channels is not supported" % (k, k, cin, cout))
            end += tiles
            it.w, it.cout, it.cin, it.ksize, it.tile_end = w.data_ptr(), cout, cin, k, end
            it.packed, it.x2, it.x3 = [t.data_ptr() if t is not None else None for t in (packed, x2, x3)]
        self.n, self.tiles = len(entries), end
        self.keep = [t for e in entries for t in e if torch.is_tensor(t)]
        self.table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(device)


def conv_repack(table):
    """surs_conv_repack of a RepackTable: every image it names, in one launch on the current stream."""
    check(lib().surs_conv_repack(_ptr(table.table), table.n, _stream()))


def conv1x1_merge(w_bl, b_bl, w_al, b_al, w_l, b_l, w_out, b_out):
    """surs_conv1x1_merge: w_out [256,256] = w_bl + w_al [256,d] w_l [d,256], b_out = b_bl + w_al b_l + b_al, sums in double in index
    order - EncoderWeights' next{s} - on the current stream."""
    d = w_l.shape[0]
    assert tuple(w_bl.shape[:2]) == (256, 256) and tuple(w_al.shape[:2]) == (256, d) and tuple(w_l.shape[:2]) == (d, 256)
    assert w_out.numel() == 256 * 256 and b_out.numel() == 256
    check(lib().surs_conv1x1_merge(*[_ptr(_f32c(t)) for t in (w_bl, b_bl, w_al, b_al, w_l, b_l)], d, _ptr(_f32c(w_out)),
                                   _ptr(_f32c(b_out)), _stream()))


def conv2d(x, cw, out=None, stride=1, in_scale=None, in_shift=None, act=0, slope=0.0, residual=None):
    pad = cw.k // 2
    ho, wo = (x.h + 2 * pad - cw.k) // stride + 1, (x.w + 2 * pad - cw.k) // stride + 1
    assert x.c == cw.cin
    if out is None:
        out = Img(ho, wo, cw.cout, device=x.buf.device)
    assert (out.h, out.w, out.c) == (ho, wo, cw.cout)
    # 3 output channels (the image head of the super-resolution net): the direct fp32 kernel behind surs_conv2d_nhwc, not a matrix tile
    thin = cw.k == 3 and stride == 1 and in_scale is None and cw.cout <= 4 and cw.cin == 32
    x3 = (cw.w3 is not None and not thin and (stride == 1 or (stride == 2 and cw.k == 3)) and x.c % 16 == 0 and x.ld % 4 == 0
          and (x.buf.data_ptr() + 4 * x.off) % 16 == 0)
    w3, parts = cw.split_image() if x3 else (None, 0)
    x3 = x3 and w3 is not None and (stride == 1 or parts == 2)
    fn, wt = ((lib().surs_conv2d_nhwc_x3 if parts == 3 else lib().surs_conv2d_nhwc_x2), w3) if x3 else (lib().surs_conv2d_nhwc, cw.w)
    if x3 and parts == 2 and cw.reduced and cw.k == 3 and not wide_operands_active():
        fn = lib().surs_conv2d_nhwc_x1
    check(fn(x.ptr(), x.h, x.w, x.c, x.ld, _ptr(wt), _ptr(cw.b), out.ptr(), cw.cout, out.ld, cw.k,
             stride, _ptr(in_scale), _ptr(in_shift), act, slope,
             residual.ptr() if residual is not None else None,
             residual.ld if residual is not None else 0, _stream()))
    out.stats = None
    return out


class GnStats:
    """GroupNorm(32) statistics of an image as the kernel that wrote it left them: partial sums [32 groups][slots][2] (sum, sum of
    squares; float64), folded in a fixed order by the 3x3 convolution that applies the normalisation (conv2d_gn)."""
    __slots__ = ("buf", "slots")

    def __init__(self, capacity, device):
        self.buf = torch.empty(32 * capacity * 2, dtype=torch.float64, device=device)
        self.slots = 0


def fused_groupnorm():
    """SURS_ENC_FUSED_GN=0: GroupNorm coefficients by surs_groupnorm_coeffs' two launches per normalisation (rounds 1 - 3)."""
    return settings.get("SURS_ENC_FUSED_GN") != "0"


def conv_gn_eligible(x, cw):
    """Can conv2d_gn run this 3x3 convolution (two-part f16 weight image, 32 | cin, 16-byte aligned pixels)?"""
    if cw.k not in (1, 3) or cw.w3 is None or x.c % 32 or x.ld % 4 or (x.buf.data_ptr() + 4 * x.off) % 16:
        return False
    w3, parts = cw.split_image()
    return w3 is not None and parts == 2


def conv2d_gn(x, cw, out=None, gn=None, want_stats=False, eps=1e-5, act=0, slope=0.0, residual=None):
    """3x3 / 1x1 convolution, stride 1, with GroupNorm(32) handed over between kernels: gn = (gamma, beta) applies GroupNorm + ReLU to
    x from x.stats (left by x's producer); want_stats leaves the statistics of the output (after activation and residual) in
    out.stats."""
    if out is None:
        out = Img(x.h, x.w, cw.cout, device=x.buf.device)
    assert x.c == cw.cin and (out.h, out.w, out.c) == (x.h, x.w, cw.cout)
    w3, parts = cw.split_image()
    assert parts == 2
    if gn is not None and x.stats is None:
        raise RuntimeError("conv2d_gn: the input carries no GroupNorm statistics")
    cap = (out.h * out.w + 127) // 128 if cw.k == 1 else ((out.w + 31) // 32) * ((out.h + 3) // 4)
    st = GnStats(cap, x.buf.device) if want_stats else None
    slots = C.c_int(0)
    check(lib().surs_conv2d_nhwc_gn(1 if cw.reduced else 2, x.ptr(), x.h, x.w, x.c, x.ld, _ptr(w3), _ptr(cw.b), out.ptr(), cw.cout, out.ld,
                                    cw.k, 1, _ptr(x.stats.buf) if gn is not None else None, x.stats.slots if gn is not None else 0,
                                    _ptr(gn[0]) if gn is not None else None, _ptr(gn[1]) if gn is not None else None, eps, act, slope,
                                    residual.ptr() if residual is not None else None, residual.ld if residual is not None else 0,
                                    _ptr(st.buf) if st is not None else None, st.buf.numel() // 64 if st is not None else 0,
                                    C.byref(slots), _stream()))
    if st is not None:
        st.slots = slots.value
    out.stats = st
    return out


def _ew_stats(n_items, device):
    return GnStats(min(512, (n_items + 1023) // 1024), device)   # (workgroups of 1024 threads, at most 512 of them)


def groupnorm_coeffs(x, gamma, beta, groups=32, eps=1e-5):
    scale = torch.empty(x.c, dtype=torch.float32, device=x.buf.device)
    shift = torch.empty_like(scale)
    # (the partial sums' scratch from the caching allocator: nothing is allocated inside the library, so the launches can be
    #  captured into a HIP graph - encoder.py)
    scratch = torch.empty(lib().surs_groupnorm_scratch_bytes(), dtype=torch.uint8, device=x.buf.device)
    check(lib().surs_groupnorm_coeffs_ws(x.ptr(), x.h * x.w, x.c, x.ld, groups, eps, _ptr(gamma), _ptr(beta), _ptr(scale),
                                         _ptr(shift), _ptr(scratch), _stream()))
    return scale, shift


def scale_shift_act(x, scale, shift, relu, out=None):
    out = out or Img(x.h, x.w, x.c, device=x.buf.device)
    check(lib().surs_scale_shift_act(x.ptr(), x.h * x.w, x.c, x.ld, _ptr(scale), _ptr(shift), int(relu), out.ptr(), out.ld,
                                     _stream()))
    out.stats = None   # (whatever GroupNorm statistics travelled with `out` described other values)
    return out


def avgpool2(x, out=None, want_stats=False):
    out = out or Img(x.h // 2, x.w // 2, x.c, device=x.buf.device)
    if want_stats:
        st, slots = _ew_stats(out.h * out.w * (x.c // 4), x.buf.device), C.c_int(0)
        check(lib().surs_avgpool2_gn(x.ptr(), x.h, x.w, x.c, x.ld, out.ptr(), out.ld, _ptr(st.buf), st.buf.numel() // 64, C.byref(slots),
                                     _stream()))
        st.slots = slots.value
        out.stats = st
        return out
    check(lib().surs_avgpool2(x.ptr(), x.h, x.w, x.c, x.ld, out.ptr(), out.ld, _stream()))
    out.stats = None
    return out


def bicubic_up2(x, align_corners, addend=None, out=None, want_stats=False):
    out = out or Img(2 * x.h, 2 * x.w, x.c, device=x.buf.device)
    if want_stats:
        st, slots = _ew_stats(out.h * out.w * (x.c // 4), x.buf.device), C.c_int(0)
        check(lib().surs_bicubic_up2_gn(x.ptr(), x.h, x.w, x.c, x.ld, int(bool(align_corners)),
                                        addend.ptr() if addend is not None else None, addend.ld if addend is not None else 0,
                                        out.ptr(), out.ld, _ptr(st.buf), st.buf.numel() // 64, C.byref(slots), _stream()))
        st.slots = slots.value
        out.stats = st
        return out
    out.stats = None
    check(lib().surs_bicubic_up2(x.ptr(), x.h, x.w, x.c, x.ld, int(bool(align_corners)),
                                 addend.ptr() if addend is not None else None, addend.ld if addend is not None else 0,
                                 out.ptr(), out.ld, _stream()))
    return out


def bicubic_up(x, scale, align_corners=False, addend=None, out=None):
    """Bicubic enlargement by an integer factor in 1..4 with PyTorch's coordinate arithmetic (surs_bicubic_up); 2: bicubic_up2's bits."""
    out = out or Img(scale * x.h, scale * x.w, x.c, device=x.buf.device)
    out.stats = None
    check(lib().surs_bicubic_up(x.ptr(), x.h, x.w, x.c, x.ld, int(scale), int(bool(align_corners)),
                                addend.ptr() if addend is not None else None, addend.ld if addend is not None else 0,
                                out.ptr(), out.ld, _stream()))
    return out


def bicubic_up2_block(x, align_corners, addend=None, out=None):
    """bicubic_up2 as 2 x 2 output blocks per work item - the kernel form of bicubic_up2(want_stats=True) without its statistics."""
    out = out or Img(2 * x.h, 2 * x.w, x.c, device=x.buf.device)
    out.stats = None
    check(lib().surs_bicubic_up2_block(x.ptr(), x.h, x.w, x.c, x.ld, int(bool(align_corners)),
                                       addend.ptr() if addend is not None else None, addend.ld if addend is not None else 0,
                                       out.ptr(), out.ld, _stream()))
    return out


def stats_calls():
    """Calls so far into the library's GroupNorm-statistics entry points (surs_stats_calls): a BatchNorm encoder makes none."""
    return int(lib().surs_stats_calls())


def pixel_shuffle2(x, slope, out=None):
    out = out or Img(2 * x.h, 2 * x.w, x.c // 4, device=x.buf.device)
    check(lib().surs_pixel_shuffle2(x.ptr(), x.h, x.w, x.c, x.ld, slope, out.ptr(), out.ld, _stream()))
    out.stats = None
    return out


def add3(a, b, c=None, out=None, want_stats=False):
    out = out or Img(a.h, a.w, a.c, device=a.buf.device)
    if want_stats:
        st, slots = _ew_stats(a.h * a.w * (a.c // 4), a.buf.device), C.c_int(0)
        check(lib().surs_add3_gn(a.ptr(), a.ld, b.ptr(), b.ld, c.ptr() if c is not None else None, c.ld if c is not None else 0,
                                 a.h * a.w, a.c, out.ptr(), out.ld, _ptr(st.buf), st.buf.numel() // 64, C.byref(slots), _stream()))
        st.slots = slots.value
        out.stats = st
        return out
    check(lib().surs_add3(a.ptr(), a.ld, b.ptr(), b.ld, c.ptr() if c is not None else None, c.ld if c is not None else 0,
                          a.h * a.w, a.c, out.ptr(), out.ld, _stream()))
    out.stats = None
    return out


# ------------------------------------------------------------------ point evaluator

def pack_mlp(sd, dtype, device):
    """Pack mlp_lr / mlp_hr from a (numpy) state dict into the device blob of surs_mlp_pack."""
    keep = []

    def arrs(prefix):
        ws, bs = (C.c_void_p * 5)(), (C.c_void_p * 5)()
        for l in range(5):
            w = np.ascontiguousarray(np.asarray(sd[prefix + "conv%d.weight" % l], np.float32).reshape(
                np.asarray(sd[prefix + "conv%d.weight" % l]).shape[0], -1))
            b = np.ascontiguousarray(np.asarray(sd[prefix + "conv%d.bias" % l], np.float32))
            keep.extend([w, b])
            ws[l], bs[l] = w.ctypes.data, b.ctypes.data
        return ws, bs

    expect = {"mlp_lr.": [(1024, 321), (512, 1024), (256, 833), (128, 577), (1, 449)],
              "mlp_hr.": [(1024, 322), (512, 1024), (256, 834), (128, 578), (1, 450)]}
    for prefix, shapes in expect.items():
        for l, s in enumerate(shapes):
            got = tuple(np.asarray(sd[prefix + "conv%d.weight" % l]).shape[:2])
            if got != s:
                raise ValueError("SurfaceClassifier shape %s%d: %s is not the released shape these kernels are built for: "
                                 "pack it with pack_mlp_generic (mlp_shapes gives the supported limits)" % (prefix, l, got))
    wl, bl = arrs("mlp_lr.")
    wh, bh = arrs("mlp_hr.")
    code = DTYPES[dtype] if isinstance(dtype, str) else dtype
    core = BF16 if code in (F32, _lib.F32_GEMM) else code
    n = lib().surs_mlp_pack(wl, bl, wh, bh, core, None)
    host = np.zeros(n, np.uint8)
    lib().surs_mlp_pack(wl, bl, wh, bh, core, host.ctypes.data_as(C.c_void_p))
    return torch.from_numpy(host).to(device), core


DEFAULT_MLP_SHAPES = (((321, 1024, 512, 256, 128, 1), (2, 3, 4)), ((322, 1024, 512, 256, 128, 1), (2, 3, 4)))
MLP_MAX_LAYERS, MLP_MAX_WIDTH = 8, 2048
HG_DIM_RULE = "the supported values are the multiples of 16 from 16 to 512"


def check_hg_dim(hg_dim):
    """--hg_dim, the channels of the hourglass encoder's output (lib/model/HGFilters.py:166-174): multiples of 16 (the cin % 16 rule
    of the split-operand convolutions, which al{s} meets with cin = hg_dim) from 16 to 512 (beyond it the LDS of the fused
    evaluators leaves too little for the hidden layers).  Returns it as an int; ValueError otherwise."""
    ok = isinstance(hg_dim, (int, np.integer)) and not isinstance(hg_dim, bool) and 16 <= hg_dim <= 512 and hg_dim % 16 == 0
    if not ok:
        raise ValueError("hg_dim %r: %s" % (hg_dim, HG_DIM_RULE))
    return int(hg_dim)


def mlp_max_hidden(hg_dim, views=False):
    """The widest hidden layer the fused evaluator (views: the multi-view one) takes with --hg_dim hg_dim: what a 16-point tile holds
    in the 160 KiB of LDS beside its feature rows of pad32(hg_dim + 66) + 4 floats (csrc/surs_mlp_generic.h gen_max_hidden): 2048 /
    1824 up to the released 256, less beyond it."""
    fs = -(-(hg_dim + 66) // 32) * 32 + 4
    rows, extra, cap = (2, 24, 1824) if views else (1, 16, MLP_MAX_WIDTH)
    return min(cap, ((160 * 1024 // 16 - extra) // 4 - 4 - rows * fs) // 32 * 32)


def mlp_hg_dim(shapes):
    """--hg_dim of a classifier pair: its lr input width is [hg_dim lr | 64 hr | z]."""
    return int(shapes[0][0][0]) - 65


def _check_feat_channels(c_lr, c_hr, g):
    """The feature maps a generic evaluator is about to read against the shape it was packed for: the kernel reads rows of hg_dim
    floats, so any other channel count would be read out of bounds."""
    D = mlp_hg_dim(g.shapes)
    if c_lr != D or c_hr != 64:
        raise ValueError("feature maps with %d lr / %d hr channels; the classifiers (input width %d) read %d (--hg_dim) / 64"
                         % (c_lr, c_hr, g.shapes[0][0][0], D))


def mlp_shapes(sd, opt=None):
    """((dims_lr, res_lr), (dims_hr, res_hr)) of the two SurfaceClassifiers in state dict `sd`, derived from the weight tensors
    (lib/model/SurfaceClassifier.py:7-43: layer l sees dims[l] channels, plus dims[0] when l is a skip layer) and cross-checked
    against opt's --mlp_dim_* / --mlp_res_layers_* / --no_residual when opt is given.  Raises ValueError naming the limit for
    anything the evaluators do not support: 1..8 layers, input width hg_dim + 65 (lr) / hg_dim + 66 (hr) - fixed by the encoder's
    --hg_dim, taken from opt (256 without it: 321 / 322) -, last width 1, hidden widths 1..2048 (less for hg_dim > 256:
    mlp_max_hidden), skip layers in [0, L)."""
    out = []
    hg_dim = check_hg_dim(getattr(opt, "hg_dim", 256)) if opt is not None else 256
    max_width = mlp_max_hidden(hg_dim)
    for m, (prefix, c0) in enumerate((("mlp_lr.", hg_dim + 65), ("mlp_hr.", hg_dim + 66))):
        L = 0
        while prefix + "conv%d.weight" % L in sd:
            L += 1
        if not 1 <= L <= MLP_MAX_LAYERS:
            raise ValueError("%s: %d layers; the number of layers must be between 1 and %d" % (prefix[:-1], L, MLP_MAX_LAYERS))
        dims, res = [], []
        for l in range(L):
            w = np.asarray(sd[prefix + "conv%d.weight" % l])
            cout, cin = int(w.shape[0]), int(w.shape[1])
            if l == 0:
                if cin not in (c0, 2 * c0):
                    raise ValueError("%s: input width %d; it must be %d (%d + 64 + z%s: --hg_dim %d), or %d with a skip at layer 0"
                                     % (prefix[:-1], cin, c0, hg_dim, "" if m == 0 else " + p_lr", hg_dim, 2 * c0))
                dims.append(c0)
            if cin - dims[l] == c0:
                res.append(l)
            elif cin != dims[l]:
                raise ValueError("%s.conv%d: %d input channels fit neither %d nor %d + %d" % (prefix[:-1], l, cin, dims[l], dims[l], c0))
            dims.append(cout)
        if dims[-1] != 1:
            raise ValueError("%s: last width %d; it must be 1" % (prefix[:-1], dims[-1]))
        for d in dims[1:-1]:
            if not 1 <= d <= MLP_MAX_WIDTH:
                raise ValueError("%s: hidden width %d; hidden widths must be between 1 and %d" % (prefix[:-1], d, MLP_MAX_WIDTH))
            if d > max_width:   # (the library's words: gen_shape_error)
                raise ValueError("%s: hidden width %d; hidden widths must be at most %d with hg_dim %d (the LDS of a 16-point tile)"
                                 % (prefix[:-1], d, max_width, hg_dim))
        if opt is not None:
            want_dims = [int(v) for v in (opt.mlp_dim_lr if m == 0 else opt.mlp_dim_hr)]
            want_res = [] if opt.no_residual else sorted(set(int(v) for v in (opt.mlp_res_layers_lr if m == 0 else opt.mlp_res_layers_hr)))
            if any(r < 0 or r >= len(want_dims) - 1 for r in want_res):
                raise ValueError("%s: skip layers %s; they must be in [0, %d)" % (prefix[:-1], want_res, len(want_dims) - 1))
            if want_dims != dims or want_res != res:
                raise ValueError("%s: the weights describe dims %s, skips %s; the options say dims %s, skips %s"
                                 % (prefix[:-1], dims, res, want_dims, want_res))
        out.append((tuple(dims), tuple(res)))
    return tuple(out)


def is_default_mlp(shapes):
    return tuple(shapes) == DEFAULT_MLP_SHAPES


class GenericMlp:
    """A classifier pair of any supported shape packed for the fused evaluator (surs_mlp_pack_generic): device blob + shapes."""

    def __init__(self, blob, shapes):
        self.blob, self.shapes = blob, shapes
        self.lr, self.hr = (_shape_struct(*s) for s in shapes)

    def info(self):
        return mlp_generic_info(self.shapes)


def mlp_generic_info(shapes):
    """(points per tile, LDS bytes per workgroup, blob offsets [2,8,4] of the one-, two-, three-part images and the bias of each
    layer) of surs_mlp_generic_info: how the fused evaluator runs this pair (host only)."""
    lr, hr = (_shape_struct(*s) for s in shapes)
    tp, lds = C.c_int(0), C.c_int(0)
    off = np.zeros((2, 8, 4), np.uint64)
    check(lib().surs_mlp_generic_info(C.byref(lr), C.byref(hr), C.byref(tp), C.byref(lds), off.ctypes.data_as(C.c_void_p)))
    return tp.value, lds.value, off


def _shape_struct(dims, res):
    s = _lib.MlpShape()
    s.n_layers = len(dims) - 1
    for i, d in enumerate(dims):
        s.dims[i] = int(d)
    s.res_mask = sum(1 << int(r) for r in res)
    return s


def pack_mlp_generic_host(sd, shapes=None):
    """surs_mlp_pack_generic into a numpy uint8 array: (host blob, shapes)."""
    shapes = mlp_shapes(sd) if shapes is None else shapes   # (given: any --hg_dim, the library checks them)
    keep, args = [], []
    for m, prefix in enumerate(("mlp_lr.", "mlp_hr.")):
        L = len(shapes[m][0]) - 1
        ws, bs = (C.c_void_p * L)(), (C.c_void_p * L)()
        for l in range(L):
            w = np.ascontiguousarray(np.asarray(sd[prefix + "conv%d.weight" % l], np.float32).reshape(shapes[m][0][l + 1], -1))
            b = np.ascontiguousarray(np.asarray(sd[prefix + "conv%d.bias" % l], np.float32))
            keep.extend([w, b])
            ws[l], bs[l] = w.ctypes.data, b.ctypes.data
        args.append((_shape_struct(*shapes[m]), ws, bs))
    (sl, wl, bl), (sh, wh, bh) = args
    n = lib().surs_mlp_pack_generic(C.byref(sl), wl, bl, C.byref(sh), wh, bh, None)
    if n == 0:
        raise ValueError(lib().surs_last_error().decode())
    host = np.zeros(n, np.uint8)
    lib().surs_mlp_pack_generic(C.byref(sl), wl, bl, C.byref(sh), wh, bh, host.ctypes.data_as(C.c_void_p))
    return host, shapes


def pack_mlp_generic(sd, device, shapes=None):
    """Pack mlp_lr / mlp_hr of any supported shape for the fused evaluator: a GenericMlp on `device`."""
    host, shapes = pack_mlp_generic_host(sd, shapes)
    return GenericMlp(torch.from_numpy(host).to(device), shapes)


def query_points_generic(points, calib, zmul, zdiv, feat_lr, feat_hr, g, p_lr=None, want_logits=False):
    """surs_query_points_generic: both classifiers of GenericMlp g on points [3,N] in one launch (p_lr [N] given: the hr classifier
    alone).  Returns (pred_hr, pred_lr[, logit_hr, logit_lr]); with p_lr, pred_lr is p_lr and logit_lr None."""
    points = _f32c(points)
    n = points.shape[1]
    dev = points.device
    phr = torch.empty(n, dtype=torch.float32, device=dev)
    if p_lr is not None:
        p_lr = _f32c(p_lr.reshape(-1))
        assert p_lr.numel() == n
        plr = p_lr
    else:
        plr = torch.empty(n, dtype=torch.float32, device=dev)
    lg = [torch.empty(n, dtype=torch.float32, device=dev) if want_logits else None for _ in range(2)]
    if p_lr is not None:
        lg[1] = None
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    _check_feat_channels(feat_lr.c, feat_hr.c, g)
    assert feat_lr.ld == feat_lr.c and feat_hr.ld == feat_hr.c
    check(lib().surs_query_points_generic(_ptr(points), n, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w,
                                          feat_hr.ptr(), feat_hr.h, feat_hr.w, C.byref(g.lr), C.byref(g.hr), _ptr(g.blob), _ptr(p_lr),
                                          _ptr(phr), None if p_lr is not None else _ptr(plr), _ptr(lg[0]), _ptr(lg[1]), _stream()))
    return (phr, plr, lg[0], lg[1]) if want_logits else (phr, plr)


def _stack_table(feats_lr, feat_hr):
    """The host table of the S lr map pointers (one geometry for all maps) of the stacks entries."""
    f0 = feats_lr[0]
    for f in feats_lr:
        if (f.h, f.w, f.c) != (f0.h, f0.w, f0.c) or f.ld != f.c:
            raise ValueError("the feature maps of the stacks must share one size and have ld == c")
    assert feat_hr.ld == feat_hr.c
    return (C.c_void_p * len(feats_lr))(*[f.ptr().value for f in feats_lr])


def _stack_outputs(points, S, p_lr, lr_only):
    """(points, n, p_lr [S,n] or None, pred_hr [S,n] or None, pred_lr [S,n]) of a stacks call in one of its three forms."""
    if p_lr is not None and lr_only:
        raise ValueError("p_lr (hr only) and lr_only exclude each other")
    points = _f32c(points)
    n, dev = points.shape[1], points.device
    phr = None if lr_only else torch.empty((S, n), dtype=torch.float32, device=dev)
    if p_lr is not None:
        p_lr = _f32c(p_lr.reshape(S, -1))
        assert p_lr.shape[1] == n
        plr = p_lr
    else:
        plr = torch.empty((S, n), dtype=torch.float32, device=dev)
    return points, n, p_lr, phr, plr


def query_points_generic_stacks(points, calib, zmul, zdiv, feats_lr, feat_hr, g, p_lr=None, lr_only=False):
    """surs_query_points_generic_stacks: GenericMlp g on points [3,N] for every lr map of feats_lr (a list of S Img; one hr map) in
    one launch.  Returns (pred_hr [S,N], pred_lr [S,N]), row s = query_points_generic on map s, bit for bit.  p_lr [S,N]: the hr
    classifier alone (pred_lr is p_lr); lr_only: the lr classifier alone (pred_hr is None)."""
    S = len(feats_lr)
    points, n, p_lr, phr, plr = _stack_outputs(points, S, p_lr, lr_only)
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    for f in feats_lr:
        _check_feat_channels(f.c, feat_hr.c, g)
    tab = _stack_table(feats_lr, feat_hr)
    f0 = feats_lr[0]
    check(lib().surs_query_points_generic_stacks(_ptr(points), n, cal, float(zmul), float(zdiv), S, tab, f0.h, f0.w, feat_hr.ptr(),
                                                 feat_hr.h, feat_hr.w, C.byref(g.lr), C.byref(g.hr), _ptr(g.blob), _ptr(p_lr), _ptr(phr),
                                                 None if p_lr is not None else _ptr(plr), None, None, _stream()))
    return phr, plr


def query_grid_generic(i0, i1, ry, rz, mat, calib, zmul, zdiv, feat_lr, feat_hr, g, vol_hr=None, vol_lr=None):
    """surs_query_grid_generic: the dense sweep of grid slab [i0, i1) with the fused evaluator.  Returns (vol_hr, vol_lr) float32
    device tensors [(i1-i0), ry, rz]."""
    dev = g.blob.device
    if vol_hr is None:
        vol_hr = torch.empty((i1 - i0, ry, rz), dtype=torch.float32, device=dev)
        vol_lr = torch.empty_like(vol_hr)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    _check_feat_channels(feat_lr.c, feat_hr.c, g)
    assert feat_lr.ld == feat_lr.c and feat_hr.ld == feat_hr.c
    check(lib().surs_query_grid_generic(i0, i1, ry, rz, m, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w,
                                        feat_hr.ptr(), feat_hr.h, feat_hr.w, C.byref(g.lr), C.byref(g.hr), _ptr(g.blob), _ptr(vol_hr),
                                        _ptr(vol_lr), _stream()))
    return vol_hr, vol_lr


def mlp_generic_views_info(shapes, num_views):
    """(points per tile, LDS bytes per workgroup) of surs_mlp_generic_views_info: how the multi-view evaluator runs this pair for
    num_views views (host only).  Raises ValueError with the library's message for what it refuses: num_views outside [1, 64], a
    hidden layer wider than the multi-view limit."""
    lr, hr = (_shape_struct(*s) for s in shapes)
    tp, lds = C.c_int(0), C.c_int(0)
    if lib().surs_mlp_generic_views_info(C.byref(lr), C.byref(hr), int(num_views), C.byref(tp), C.byref(lds)) != 0:
        raise ValueError(lib().surs_last_error().decode())
    return tp.value, lds.value


def _device_calibs(calibs, dev):
    """calibs [V,12] (host array, or a device tensor already) -> contiguous float32 device tensor [V,12]."""
    if torch.is_tensor(calibs) and calibs.is_cuda:
        return _f32c(calibs.reshape(calibs.shape[0], -1)[:, :12].contiguous())
    cal = np.ascontiguousarray(np.asarray(calibs, np.float32).reshape(np.shape(calibs)[0], -1)[:, :12])
    return torch.from_numpy(cal).to(dev)


def query_points_generic_views(points, calibs, zmul, zdiv, feat_lr, feat_hr, g, p_lr=None, want_logits=False):
    """surs_query_points_generic_views: both classifiers of GenericMlp g for one subject seen by V views, in one launch.  points
    [V,3,N] f32 device tensor; calibs [V,12] (host rows or a device tensor); feat_lr [V,hl,wl,hg_dim] and feat_hr [V,hh,wh,64]
    contiguous NHWC device tensors; p_lr [V,N] given: the hr classifier alone.  Returns (pred_hr [V,N], pred_lr [V,N][, logit_hr [N],
    logit_lr [N]]); with p_lr, pred_lr is p_lr and logit_lr None."""
    points = _f32c(points)
    V, _, n = points.shape
    mlp_generic_views_info(g.shapes, V)
    dev = points.device
    feat_lr, feat_hr = _f32c(feat_lr), _f32c(feat_hr)
    _check_feat_channels(feat_lr.shape[3], feat_hr.shape[3], g)
    assert feat_lr.shape[0] == V and feat_hr.shape[0] == V
    cal = _device_calibs(calibs, dev)
    assert cal.shape == (V, 12)
    phr = torch.empty((V, n), dtype=torch.float32, device=dev)
    if p_lr is not None:
        p_lr = _f32c(p_lr.reshape(V, n))
        plr = p_lr
    else:
        plr = torch.empty_like(phr)
    lg = [torch.empty(n, dtype=torch.float32, device=dev) if want_logits else None for _ in range(2)]
    if p_lr is not None:
        lg[1] = None
    check(lib().surs_query_points_generic_views(_ptr(points), n, V, _ptr(cal), float(zmul), float(zdiv), _ptr(feat_lr), feat_lr.shape[1],
                                                feat_lr.shape[2], _ptr(feat_hr), feat_hr.shape[1], feat_hr.shape[2], C.byref(g.lr),
                                                C.byref(g.hr), _ptr(g.blob), _ptr(p_lr), _ptr(phr),
                                                None if p_lr is not None else _ptr(plr), _ptr(lg[0]), _ptr(lg[1]), _stream()))
    return (phr, plr, lg[0], lg[1]) if want_logits else (phr, plr)


def query_grid_generic_views(i0, i1, ry, rz, mat, calibs, zmul, zdiv, feat_lr, feat_hr, g, vol_hr=None, vol_lr=None):
    """surs_query_grid_generic_views: the dense sweep of grid slab [i0, i1) for a multi-view model with the fused evaluator - every
    voxel seen by every view, view 0's predictions kept (lib/mesh_util.py:20-28).  calibs [V,12]; feat_lr [V,hl,wl,256], feat_hr
    [V,hh,wh,64] contiguous NHWC device tensors.  Returns (vol_hr, vol_lr) float32 device tensors [(i1-i0), ry, rz]."""
    feat_lr, feat_hr = _f32c(feat_lr), _f32c(feat_hr)
    V = feat_lr.shape[0]
    mlp_generic_views_info(g.shapes, V)
    dev = g.blob.device
    _check_feat_channels(feat_lr.shape[3], feat_hr.shape[3], g)
    assert feat_hr.shape[0] == V
    cal = _device_calibs(calibs, dev)
    assert cal.shape == (V, 12)
    if vol_hr is None:
        vol_hr = torch.empty((i1 - i0, ry, rz), dtype=torch.float32, device=dev)
        vol_lr = torch.empty_like(vol_hr)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    check(lib().surs_query_grid_generic_views(i0, i1, ry, rz, m, V, _ptr(cal), float(zmul), float(zdiv), _ptr(feat_lr), feat_lr.shape[1],
                                              feat_lr.shape[2], _ptr(feat_hr), feat_hr.shape[1], feat_hr.shape[2], C.byref(g.lr),
                                              C.byref(g.hr), _ptr(g.blob), _ptr(vol_hr), _ptr(vol_lr), _stream()))
    return vol_hr, vol_lr


class Workspace:
    """Grow-only device scratch buffer; remembers mesh capacities between extractions."""

    def __init__(self, device):
        self.device = device
        self.buf = None
        self.mc_capacity = {}     # key -> (verts, faces) of that field's last extraction: sizes the next one without a counting pass
        self.mesh_ws = {}         # key -> private marching-cubes workspace of an incremental extraction (MeshStream)

    def get(self, nbytes):
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = None
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self.buf

    def to_host(self, tensors):
        """device tensors -> numpy arrays backed by pinned host memory (one sync for the whole batch).  Each array owns
        its pinned block (torch's caching host allocator recycles it once the array is garbage collected), so the
        results stay valid like the reference's freshly allocated arrays, without a second host copy."""
        outs = []
        for t in tensors:
            if t is None:
                outs.append(None)
                continue
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            outs.append(h)
        torch.cuda.current_stream().synchronize()
        return [o.numpy() if o is not None else None for o in outs]

    def to_host_async(self, tensors):
        """Same copies on a side stream, ordered after the work enqueued so far; returns a HostCopy."""
        return _to_host_async(self, tensors)


class HostCopy:
    """Device -> pinned host copies in flight on the workspace's copy stream (Workspace.to_host_async); result() waits
    for them and returns the numpy arrays.  Lets the copy of one mesh run under the marching cubes of the next."""

    def __init__(self, hosts, done, keep):
        self._hosts, self._done, self._keep = hosts, done, keep

    def result(self):
        self._done.synchronize()
        self._keep = None
        return [h.numpy() if h is not None else None for h in self._hosts]


_shared_streams = {}


def shared_stream(device, name):
    """The process's side stream `name` on `device` (copy stream, one marching-cubes stream per field): ONE set per device, shared
    by every Workspace.  HIP maps streams onto a handful of hardware queues; a second SuRSNet object with side streams of its own
    (bench.py's fp32 leg) found its copy stream on the hardware queue of the sweep, and the 1 GB of mesh copies that should travel
    under the sweep followed it instead: + 19 ms per 512^3 reconstruction (round 4, tools/diag/second_net.py)."""
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), name)
    st = _shared_streams.get(key)
    if st is None:
        st = _shared_streams[key] = torch.cuda.Stream(device=dev)
    return st


def _to_host_async(ws, tensors):
    cur = torch.cuda.current_stream()
    side = shared_stream(ws.device, "copy")
    ready = torch.cuda.Event()
    ready.record(cur)
    side.wait_event(ready)
    hosts = []
    with torch.cuda.stream(side):
        for t in tensors:
            if t is None:
                hosts.append(None)
                continue
            t.record_stream(side)   # the caching allocator must not hand the block out again before the copy ran
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            hosts.append(h)
        done = torch.cuda.Event()
        done.record(side)
    return HostCopy(hosts, done, list(tensors))


def query_points(points, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws, want_logits=False):
    """points [3,N] f32 device tensor; calib: 12 floats (host); feat_*: Img with ld == c.  Returns pred_hr, pred_lr[, logits]."""
    points = _f32c(points)
    n = points.shape[1]
    dev = points.device
    outs = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4 if want_logits else 2)]
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    need = lib().surs_query_workspace_bytes(n)
    w = ws.get(need)
    assert feat_lr.ld == feat_lr.c == 256 and feat_hr.ld == feat_hr.c == 64
    check(lib().surs_query_points(_ptr(points), n, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w,
                                  feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob), _ptr(w), w.numel(), _ptr(outs[0]),
                                  _ptr(outs[1]), _ptr(outs[2]) if want_logits else None,
                                  _ptr(outs[3]) if want_logits else None, _stream()))
    return tuple(outs)


def set_option(name, value):
    """surs_set_option: a library option by name (include/surs.h; `options()` lists them)."""
    check(lib().surs_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int(0)
    check(lib().surs_get_option(name.encode(), C.byref(v)))
    return v.value


def options():
    """{name: (value, help)} of every library option."""
    out, i = {}, 0
    while True:
        name = lib().surs_option_name(i)
        if name is None:
            return out
        out[name.decode()] = (get_option(name.decode()), lib().surs_option_help(i).decode())
        i += 1


def any_nonfinite(a, b=None):
    """surs_nonfinite: True if the float32 device tensors a / b hold a NaN or an infinity (one small launch, one 4-byte read-back)."""
    a = _f32c(a.reshape(-1))
    if b is not None:
        b = _f32c(b.reshape(-1))
        assert b.numel() == a.numel()
    if a.numel() == 0:
        return False
    flag = torch.empty(1, dtype=torch.int32, device=a.device)
    check(lib().surs_nonfinite(_ptr(a), _ptr(b) if b is not None else None, a.numel(), _ptr(flag), _stream()))
    return bool(flag.item())


POINT_RUNS_CHUNK = 262144   # points per surs_query_points_columns call


def query_points_columns(points, calib, zmul, zdiv, feat_lr, feat_hr, blob, dtype, ws):
    """surs_query_points_columns: both classifiers on points [3,N] THROUGH THE COLUMN KERNELS where the points come as runs that share
    their (x, y) - what the reference's sweep loop (lib/sdf.py:32-45: 50 000 consecutive grid points per call, z fastest) hands the
    facade.  dtype: the blob's ("fp32": kernel v11, fp32-grade; "bf16" / "fp16": kernel v10).  Returns (pred_hr, pred_lr), or None
    when the array holds no such runs (random samples; a general calibration; fewer than 2048 points; inside wide_operands()) - the
    caller then takes query_points.  One host synchronisation (the run count)."""
    if wide_operands_active() or settings.get("SURS_POINT_RUNS") == "0":
        return None
    points = _f32c(points)
    n = points.shape[1]
    if n < 2048:
        return None
    dev = points.device
    phr = torch.empty(n, dtype=torch.float32, device=dev)
    plr = torch.empty(n, dtype=torch.float32, device=dev)
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    code = DTYPES[dtype] if isinstance(dtype, str) else dtype
    w = ws.get(lib().surs_query_points_columns_workspace_bytes())
    assert feat_lr.ld == feat_lr.c == 256 and feat_hr.ld == feat_hr.c == 64
    ncols = C.c_int(0)
    for p0 in range(0, n, POINT_RUNS_CHUNK):
        nb = min(POINT_RUNS_CHUNK, n - p0)
        check(lib().surs_query_points_columns(C.c_void_p(points.data_ptr() + 4 * p0), n, nb, cal, float(zmul), float(zdiv),
                                              feat_lr.ptr(), feat_lr.h, feat_lr.w, feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob),
                                              code, _ptr(w), w.numel(), C.c_void_p(phr.data_ptr() + 4 * p0),
                                              C.c_void_p(plr.data_ptr() + 4 * p0), C.byref(ncols), _stream()))
        if ncols.value == 0:
            if p0 == 0 and nb == n:
                return None
            # this piece holds no runs: the point kernels for it, in the arithmetic the rest of the array gets (one product per
            # MAC behind --precision bf16 | fp16: the column kernel's pieces are 16-bit there too)
            with reduced_point_operands(code != DTYPES["fp32"]):
                a, b = query_points(points[:, p0:p0 + nb], calib, zmul, zdiv, feat_lr, feat_hr, blob, ws)
            phr[p0:p0 + nb] = a
            plr[p0:p0 + nb] = b
    return phr, plr


def point_runs(points, tile=64):
    """surs_point_runs: the runs surs_query_points_columns would evaluate in points [3,N] (N <= POINT_RUNS_CHUNK) - numpy arrays
    (colstart, kcount, tiles [ntiles, 2], meta [4]); kcount / tiles are empty when the array holds more than one run per tile / 4 points."""
    points = _f32c(points)
    n = points.shape[1]
    dev = points.device
    cs, kc = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    tl, meta = torch.empty(2 * n, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    check(lib().surs_point_runs(_ptr(points), n, n, int(tile), _ptr(cs), _ptr(kc), _ptr(tl), _ptr(meta), _stream()))
    m = meta.cpu().numpy()
    nc, nt = int(m[0]), int(m[1])
    listed = nc * (int(tile) // 4) <= n
    return (cs[:nc].cpu().numpy(), kc[:nc].cpu().numpy() if listed else np.zeros(0, np.int32),
            tl[:2 * nt].cpu().numpy().reshape(-1, 2) if listed else np.zeros((0, 2), np.int32), m)


def query_points_hr(points, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws, p_lr):
    """surs_query_points_hr: the hr classifier on points [3,N] with the lr occupancies p_lr [N] given (query_sr on points other than
    query_mr's).  Returns pred_hr [N]."""
    points = _f32c(points)
    n = points.shape[1]
    p_lr = _f32c(p_lr.reshape(-1))
    assert p_lr.numel() == n
    out = torch.empty(n, dtype=torch.float32, device=points.device)
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    w = ws.get(lib().surs_query_workspace_bytes(n))
    check(lib().surs_query_points_hr(_ptr(points), n, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w,
                                     feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob), _ptr(w), w.numel(), _ptr(p_lr), _ptr(out), None,
                                     _stream()))
    return out


def query_points_stacks(points, calib, zmul, zdiv, feats_lr, feat_hr, blob, ws, p_lr=None, lr_only=False):
    """surs_query_points_stacks: the released shape's layer kernels on points [3,N] once per lr map of feats_lr (a list of S Img), in
    one call on one workspace.  Returns (pred_hr [S,N], pred_lr [S,N]), row s = query_points (p_lr [S,N] given: query_points_hr) on
    map s, bit for bit; lr_only: the lr classifier alone (pred_hr is None)."""
    S = len(feats_lr)
    points, n, p_lr, phr, plr = _stack_outputs(points, S, p_lr, lr_only)
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    tab = _stack_table(feats_lr, feat_hr)
    f0 = feats_lr[0]
    assert f0.c == 256 and feat_hr.c == 64
    w = ws.get(lib().surs_query_workspace_bytes(n))
    check(lib().surs_query_points_stacks(_ptr(points), n, cal, float(zmul), float(zdiv), S, tab, f0.h, f0.w, feat_hr.ptr(), feat_hr.h,
                                         feat_hr.w, _ptr(blob), _ptr(w), w.numel(), _ptr(p_lr), _ptr(phr),
                                         None if p_lr is not None else _ptr(plr), None, None, _stream()))
    return phr, plr


def forward_losses(pred_lr=None, lab_lr=None, pred_hr=None, lab_hr=None, img_sr=None, img_hr=None, weights=None):
    """surs_forward_losses: the terms of SuRSNet.forward's loss in one deterministic reduction, without a host synchronisation.
    pred_lr / pred_hr [S,M] float32 device tensors, lab_lr / lab_hr [M] (the labels each is held against), img_sr / img_hr: equal
    element counts in one element order; a group left None gives a zero term.  Returns (terms [4] float32 device tensor:
    get_error_lr, get_error_hr, get_errorSR, get_error_disp_1; total: 0-dim float32 device tensor of weights (4 host floats) times
    the terms, None without weights)."""
    ref = next(t for t in (pred_lr, pred_hr, img_sr) if t is not None)
    dev = ref.device
    S, M = 1, 0
    for p, l in ((pred_lr, lab_lr), (pred_hr, lab_hr)):
        if (p is None) != (l is None):
            raise ValueError("predictions and their labels come together")
    if pred_lr is not None or pred_hr is not None:
        shp = [tuple(p.shape) for p in (pred_lr, pred_hr) if p is not None]
        if len(shp[0]) != 2 or any(q != shp[0] for q in shp):
            raise ValueError("predictions must be [S,M] and agree: %s" % (shp,))
        S, M = shp[0]
        pred_lr, pred_hr = (None if p is None else _f32c(p) for p in (pred_lr, pred_hr))
        lab_lr, lab_hr = (None if l is None else _f32c(l.to(dev).reshape(-1)) for l in (lab_lr, lab_hr))
        if any(l is not None and l.numel() != M for l in (lab_lr, lab_hr)):
            raise ValueError("labels must hold one value per point: %d" % M)
    K = 0
    if img_sr is not None:
        if img_hr is None or img_hr.numel() != img_sr.numel():
            raise ValueError("get_errorSR: image_SR %s against images_hr %s" % (tuple(img_sr.shape), None if img_hr is None else tuple(img_hr.shape)))
        img_sr, img_hr = _f32c(img_sr.reshape(-1)), _f32c(img_hr.reshape(-1))
        K = img_sr.numel()
    ws = torch.empty(lib().surs_forward_losses_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    terms = torch.empty(4, dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev) if weights is not None else None
    wt = (C.c_float * 4)(*[float(v) for v in weights]) if weights is not None else None
    check(lib().surs_forward_losses(_ptr(pred_lr), _ptr(pred_hr), int(S), int(M), _ptr(lab_lr), _ptr(lab_hr), _ptr(img_sr), _ptr(img_hr),
                                    int(K), wt, _ptr(ws), ws.numel() * 8, _ptr(terms), _ptr(total), _stream()))
    return terms, total


# ------------------------------------------------------------------ classifier gradients

def mlp_param_keys(shapes):
    """The state-dict keys of both classifiers in state_dict() order: mlp_lr.conv0.weight, mlp_lr.conv0.bias, ..., mlp_hr...."""
    return [p + "conv%d.%s" % (l, kind) for m, p in enumerate(("mlp_lr.", "mlp_hr.")) for l in range(len(shapes[m][0]) - 1)
            for kind in ("weight", "bias")]


def _f32_tensors(sd, keys, device):
    """OrderedDict key -> sd[key] (a tensor or an array) as a contiguous float32 tensor on `device`, in `keys`' order: the masters of
    MlpParams, SrParams and HgParams."""
    out = OrderedDict()
    for k in keys:
        v = sd[k]
        v = v.detach() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, np.float32))
        out[k] = v.to(device, torch.float32).contiguous()
    return out


class MlpParams:
    """The plain fp32 Conv1d weights [out,in] and biases [out] of a classifier pair on the device: what surs_mlp_grad reads."""

    def __init__(self, sd, device, shapes=None):
        self.shapes = mlp_shapes(sd) if shapes is None else shapes
        self.lr, self.hr = (_shape_struct(*s) for s in self.shapes)
        self.tensors = OrderedDict((k, v.reshape(v.shape[0], -1) if k.endswith("weight") else v.reshape(-1))
                                   for k, v in _f32_tensors(sd, mlp_param_keys(self.shapes), device).items())
        for m, p in enumerate(("mlp_lr.", "mlp_hr.")):
            dims, res = self.shapes[m]
            for l in range(len(dims) - 1):
                want = (dims[l + 1], dims[l] + (dims[0] if l in res else 0))
                if tuple(self.tensors[p + "conv%d.weight" % l].shape) != want or self.tensors[p + "conv%d.bias" % l].numel() != want[0]:
                    raise ValueError("%sconv%d: weight %s / bias %d against the shape's %s" % (
                        p, l, tuple(self.tensors[p + "conv%d.weight" % l].shape), self.tensors[p + "conv%d.bias" % l].numel(), want))

    def table(self, m, kind, tensors=None):
        t = self.tensors if tensors is None else tensors
        p = ("mlp_lr.", "mlp_hr.")[m]
        L = len(self.shapes[m][0]) - 1
        return (C.c_void_p * L)(*[t[p + "conv%d.%s" % (l, kind)].data_ptr() for l in range(L)])

    def device_tables(self):
        """(w_lr, b_lr, w_hr, b_hr): the four pointer tables of the parameters as device tensors (int64), built once - what the
        device repack reads."""
        if getattr(self, "_dev_tables", None) is None:
            dev = next(iter(self.tensors.values())).device
            self._dev_tables = [torch.tensor(list(self.table(m, kind)), dtype=torch.int64).to(dev)
                                for m in (0, 1) for kind in ("weight", "bias")]
        return self._dev_tables


def mlp_repack(params, blob, dtype):
    """surs_mlp_repack: every section of the released shape's blob (pack_mlp) rewritten in place from MlpParams `params`, in the
    blob's 16-bit dtype (BF16 / F16), on the current stream."""
    if not is_default_mlp(params.shapes):
        raise ValueError("mlp_repack: the released shape only; a GenericMlp is refreshed by mlp_repack_generic")
    check(lib().surs_mlp_repack(dtype, *[_ptr(t) for t in params.device_tables()], _ptr(blob), _stream()))


def mlp_repack_generic(params, g):
    """surs_mlp_repack_generic: the images and biases of GenericMlp `g`'s blob rewritten in place from MlpParams `params`."""
    if tuple(params.shapes) != tuple(g.shapes):
        raise ValueError("mlp_repack_generic: parameters of shapes %s against a blob packed for %s" % (params.shapes, g.shapes))
    wl, bl, wh, bh = params.device_tables()
    check(lib().surs_mlp_repack_generic(C.byref(g.lr), _ptr(wl), _ptr(bl), C.byref(g.hr), _ptr(wh), _ptr(bh), _ptr(g.blob), _stream()))


# ------------------------------------------------------------------ optimiser step

OPTIM_KINDS = {"SGD": _lib.OPTIM_SGD, "ADAM": _lib.OPTIM_ADAM, "AMSgrad": _lib.OPTIM_AMSGRAD, "RMSprop": _lib.OPTIM_RMSPROP}
OPTIM_STATES = {"SGD": ("momentum_buffer",), "ADAM": ("exp_avg", "exp_avg_sq"), "AMSgrad": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"),
                "RMSprop": ("square_avg",)}      # torch.optim's names of s0, s1, s2 (SGD: none with momentum 0)


def optim_hyper(kind, t, lr, weight_decay=0.0, momentum=0.0, betas=(0.9, 0.999), eps=1e-8, alpha=0.99, first_step=False):
    """SursOptimHyper of step t (1-based) of `kind` (a name of OPTIM_KINDS, or any int: the library refuses an unknown one): the
    step-dependent scalars lr / (1 - beta1^t), sqrt(1 - beta2^t) and the complements 1 - beta formed here in double, as torch forms
    them, and rounded to the fp32 the kernel takes.  momentum: SGD's; the other kinds have none."""
    h = _lib.OptimHyper()
    h.kind = OPTIM_KINDS[kind] if kind in OPTIM_KINDS else int(kind)
    b1, b2 = float(betas[0]), float(betas[1])
    t = max(int(t), 1)
    h.first_step = int(bool(first_step))
    h.lr, h.weight_decay, h.momentum = float(lr), float(weight_decay), float(momentum) if h.kind == _lib.OPTIM_SGD else 0.0
    h.beta1_c, h.beta2, h.beta2_c = 1.0 - b1, b2, 1.0 - b2
    h.alpha, h.alpha_c, h.eps = float(alpha), 1.0 - float(alpha), float(eps)
    h.step_size, h.bc2_sqrt = float(lr) / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5
    return h


def optim_items(rows):
    """A host array of SursOptimItem over rows (p, g, s0, s1, s2, n) of raw addresses (None: NULL), chunk_end filled in."""
    items = (_lib.OptimItem * max(len(rows), 1))()
    end = 0
    for it, (p, g, s0, s1, s2, n) in zip(items, rows):
        end += lib().surs_optim_chunks(n)
        it.p, it.g, it.s0, it.s1, it.s2, it.n, it.chunk_end = p, g, s0, s1, s2, n, end
    return items


def optim_check(items, n_items, hyper):
    """surs_optim_check of a host table: SursError for what surs_optim_step could only misuse."""
    check(lib().surs_optim_check(C.cast(items, C.c_void_p), n_items, C.byref(hyper)))


def optim_step(table, n_items, hyper):
    """surs_optim_step: every item of the DEVICE table `table` (the bytes of optim_items, checked by optim_check) updated in place by one
    launch on the current stream."""
    check(lib().surs_optim_step(_ptr(table), n_items, C.byref(hyper), _stream()))


def optim_step_host(tensors, hyper):
    """surs_optim_step_host over rows (p, g, s0, s1, s2) of contiguous float32 numpy arrays (states None where the kind has none; g of
    any shape with p's element count), updated in place on the HOST: no device needed."""
    rows = []
    for r in tensors:
        p, g = r[0], r[1]
        for a in r:
            if a is not None and (a.dtype != np.float32 or not a.flags.c_contiguous):
                raise ValueError("optim_step_host: contiguous float32 arrays expected")
        for a in r[1:]:
            if a is not None and a.size != p.size:
                raise ValueError("optim_step_host: a tensor of %d elements against a parameter of %d" % (a.size, p.size))
        rows.append(tuple(a.ctypes.data if a is not None else None for a in r) + (p.size,))
    check(lib().surs_optim_step_host(C.cast(optim_items(rows), C.c_void_p), len(rows), C.byref(hyper)))


def optim_step_ranks(table, n_items, hyper, num_ranks, rank_stride, scale):
    """surs_optim_step_ranks: optim_step with the gradient of element i of an item read as g[i + r * rank_stride], r = 0 .. num_ranks - 1
    (g points into row 0 of a gathered [num_ranks, rank_stride] buffer), summed in fp32 left to right from g_0 and multiplied once by
    the fp32 `scale` (skipped at 1.0) - in the pass that applies it; the sum is never written.  One launch on the current stream."""
    check(lib().surs_optim_step_ranks(_ptr(table), n_items, C.byref(hyper), int(num_ranks), int(rank_stride), float(scale), _stream()))


def optim_step_ranks_host(tensors, hyper, num_ranks, rank_stride, scale):
    """surs_optim_step_ranks_host over rows (p, g, s0, s1, s2) as optim_step_host takes them, except that g is a VIEW into row 0 of a
    contiguous float32 [num_ranks, rank_stride] numpy array (p.size elements of it): the rows behind it are read through the stride."""
    rows = []
    for r in tensors:
        p = r[0]
        for a in r:
            if a is not None and (a.dtype != np.float32 or not a.flags.c_contiguous):
                raise ValueError("optim_step_ranks_host: contiguous float32 arrays expected")
        for a in r[1:]:
            if a is not None and a.size != p.size:
                raise ValueError("optim_step_ranks_host: a tensor of %d elements against a parameter of %d" % (a.size, p.size))
        rows.append(tuple(a.ctypes.data if a is not None else None for a in r) + (p.size,))
    check(lib().surs_optim_step_ranks_host(C.cast(optim_items(rows), C.c_void_p), len(rows), C.byref(hyper), int(num_ranks),
                                           int(rank_stride), float(scale)))


def pack_items(rows):
    """A host array of SursPackItem over rows (src, dst, n) of raw addresses, chunk_end filled in, checked by the library."""
    items = (_lib.PackItem * max(len(rows), 1))()
    end = 0
    for it, (src, dst, n) in zip(items, rows):
        end += lib().surs_optim_chunks(n)
        it.src, it.dst, it.n, it.chunk_end = src, dst, n, end
    check(lib().surs_tensors_pack_check(C.cast(items, C.c_void_p), len(rows)))
    return items


def tensors_pack(table, n_items):
    """surs_tensors_pack: every item of the DEVICE table `table` (the bytes of pack_items' array) copied by one launch on the current
    stream."""
    check(lib().surs_tensors_pack(_ptr(table), n_items, _stream()))


def tensors_pack_host(pairs):
    """surs_tensors_pack_host over (src, dst) pairs of contiguous float32 numpy arrays of equal size."""
    for s, d in pairs:
        if any(a.dtype != np.float32 or not a.flags.c_contiguous for a in (s, d)) or s.size != d.size:
            raise ValueError("tensors_pack_host: contiguous float32 arrays of equal size expected")
    rows = [(s.ctypes.data, d.ctypes.data, s.size) for s, d in pairs]
    check(lib().surs_tensors_pack_host(C.cast(pack_items(rows), C.c_void_p), len(rows)))


# ------------------------------------------------------------------ training step: the loss head and the non-finite guard

def forward_losses_grad(pred_lr, lab_lr, pred_hr, lab_hr, img_sr_nhwc, img_hr, weights, want_grad=True):
    """surs_forward_losses_grad: forward_losses' (terms, total) - the same bits - from img_sr_nhwc [B,H,W,C], the model's own NHWC
    memory, and img_hr [B,C,H,W] as the dataset hands it, and d (weights[2] terms[2]) / d img_sr as a new [B,H,W,C] tensor (None with
    want_grad=False).  Returns (terms, total, d_img_sr).  One launch pair on the current stream, no synchronisation."""
    dev = img_sr_nhwc.device
    if pred_lr.dim() != 2 or tuple(pred_lr.shape) != tuple(pred_hr.shape):
        raise ValueError("predictions must be [S,M] and agree: %s" % ([tuple(pred_lr.shape), tuple(pred_hr.shape)],))
    S, M = pred_lr.shape
    pred_lr, pred_hr = _f32c(pred_lr), _f32c(pred_hr)
    lab_lr, lab_hr = (_f32c(l.to(dev).reshape(-1)) for l in (lab_lr, lab_hr))
    if lab_lr.numel() != M or lab_hr.numel() != M:
        raise ValueError("labels must hold one value per point: %d" % M)
    if img_sr_nhwc.dim() != 4 or img_hr.dim() != 4:
        raise ValueError("img_sr [B,H,W,C] and img_hr [B,C,H,W] are expected")
    B, H, W, Cc = img_sr_nhwc.shape
    if tuple(img_hr.shape) != (B, Cc, H, W):
        raise ValueError("get_errorSR: image_SR %s against images_hr %s" % ((B, Cc, H, W), tuple(img_hr.shape)))
    img_sr_nhwc, img_hr = _f32c(img_sr_nhwc), _f32c(img_hr)
    ws = torch.empty(lib().surs_forward_losses_grad_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    terms = torch.empty(4, dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float32, device=dev)
    d_img = torch.empty_like(img_sr_nhwc) if want_grad else None
    wt = (C.c_float * 4)(*[float(v) for v in weights])
    check(lib().surs_forward_losses_grad(_ptr(pred_lr), _ptr(pred_hr), int(S), int(M), _ptr(lab_lr), _ptr(lab_hr), _ptr(img_sr_nhwc),
                                         _ptr(img_hr), int(B), int(Cc), int(H), int(W), wt, _ptr(ws), ws.numel() * 8, _ptr(terms),
                                         _ptr(total), _ptr(d_img), _stream()))
    return terms, total, d_img


def forward_losses_grad_host(img_sr_nhwc, img_hr, w_sr):
    """surs_forward_losses_grad_host: d_img_sr [B,H,W,C] of contiguous float32 numpy arrays img_sr_nhwc [B,H,W,C], img_hr [B,C,H,W]."""
    B, H, W, Cc = img_sr_nhwc.shape
    if img_hr.shape != (B, Cc, H, W) or any(a.dtype != np.float32 or not a.flags.c_contiguous for a in (img_sr_nhwc, img_hr)):
        raise ValueError("forward_losses_grad_host: contiguous float32 [B,H,W,C] and [B,C,H,W] arrays expected")
    out = np.empty_like(img_sr_nhwc)
    check(lib().surs_forward_losses_grad_host(img_sr_nhwc.ctypes.data, img_hr.ctypes.data, B, Cc, H, W, float(w_sr), out.ctypes.data))
    return out


def tensor_refs(rows):
    """(a host array of SursTensorRef over rows (address, n), chunk_end filled in; its chunk count), checked by the library."""
    items = (_lib.TensorRef * max(len(rows), 1))()
    end = 0
    for it, (p, n) in zip(items, rows):
        end += lib().surs_optim_chunks(n)
        it.p, it.n, it.chunk_end = p, n, end
    total = C.c_longlong(0)
    check(lib().surs_tensors_nonfinite_check(C.cast(items, C.c_void_p), len(rows), C.byref(total)))
    return items, total.value


def tensors_nonfinite(table, n_items, total_chunks, workspace=None, result=None):
    """surs_tensors_nonfinite over the DEVICE table `table` (the bytes of tensor_refs' array): a 0-dim int32 device tensor holding the
    lowest index whose tensor has a NaN or an infinity, or -1.  No synchronisation: reading the result is the caller's."""
    dev = table.device
    need = lib().surs_tensors_nonfinite_workspace_bytes(total_chunks)
    if workspace is None or workspace.numel() * 4 < need:
        workspace = torch.empty(max(need // 4, 1), dtype=torch.int32, device=dev)
    if result is None:
        result = torch.empty((), dtype=torch.int32, device=dev)
    check(lib().surs_tensors_nonfinite(_ptr(table), n_items, total_chunks, _ptr(workspace), workspace.numel() * 4, _ptr(result), _stream()))
    return result


def tensors_nonfinite_device(tensors):
    """tensors_nonfinite of a list of contiguous float32 device tensors, table built and uploaded here (tests and tools; the
    optimiser keeps its table between steps)."""
    tensors = [_f32c(t) for t in tensors]
    items, total = tensor_refs([(t.data_ptr(), t.numel()) for t in tensors])
    dev = tensors[0].device
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    return tensors_nonfinite(table, len(tensors), total)


def tensors_nonfinite_host(arrays):
    """surs_tensors_nonfinite_host over contiguous float32 numpy arrays: the lowest index with a NaN or an infinity, or -1."""
    for a in arrays:
        if a.dtype != np.float32 or not a.flags.c_contiguous:
            raise ValueError("tensors_nonfinite_host: contiguous float32 arrays expected")
    items, _ = tensor_refs([(a.ctypes.data, a.size) for a in arrays])
    res = C.c_int(0)
    check(lib().surs_tensors_nonfinite_host(C.cast(items, C.c_void_p), len(arrays), C.byref(res)))
    return res.value


def mlp_grad_workspace_bytes(shapes):
    """surs_mlp_grad_workspace_bytes: the device workspace of mlp_grads for this pair - a function of the shapes, not of n."""
    lr, hr = (_shape_struct(*s) for s in shapes)
    n = lib().surs_mlp_grad_workspace_bytes(C.byref(lr), C.byref(hr))
    if n == 0:
        raise ValueError(lib().surs_last_error().decode())
    return n


def mlp_grad_features_workspace_bytes(shapes):
    """surs_mlp_grad_features_workspace_bytes: the workspace of mlp_grads(feat_grads=...) - a function of the shapes, neither of n nor
    of the map sizes."""
    lr, hr = (_shape_struct(*s) for s in shapes)
    n = lib().surs_mlp_grad_features_workspace_bytes(C.byref(lr), C.byref(hr))
    if n == 0:
        raise ValueError(lib().surs_last_error().decode())
    return n


class FeatGrads:
    """d error / d (the feature maps) of one image, as mlp_grads(feat_grads=...) fills them: lr - a list of S NHWC float32 device
    tensors [hl,wl,D], one per lr map -, hr [hh,wh,64].  Given tensors are used as they are (contiguous float32, e.g. views into
    a batch's buffer); FeatGrads.like(feats_lr, feat_hr) allocates."""

    def __init__(self, lr, hr):
        self.lr, self.hr = list(lr), hr

    @staticmethod
    def like(feats_lr, feat_hr, device):
        return FeatGrads([torch.empty((f.h, f.w, f.c), dtype=torch.float32, device=device) for f in feats_lr],
                         torch.empty((feat_hr.h, feat_hr.w, feat_hr.c), dtype=torch.float32, device=device))

    def check(self, feats_lr, feat_hr, device):
        if len(self.lr) != len(feats_lr):
            raise ValueError("feat_grads: %d lr maps against %d feature maps" % (len(self.lr), len(feats_lr)))
        for t, f in zip(self.lr + [self.hr], list(feats_lr) + [feat_hr]):
            if tuple(t.shape) != (f.h, f.w, f.c) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
                raise ValueError("feat_grads: a contiguous float32 tensor %s on %s is needed, not %s %s"
                                 % ((f.h, f.w, f.c), device, tuple(t.shape), t.dtype))


def mlp_grads(points_mr, points_sr, calib_mr, calib_sr, zmul, zdiv, feats_lr, feat_hr, params, lab_lr, lab_hr, loss_weights, m_total,
              grads=None, accumulate=False, want_preds=False, workspace=None, feat_grads=None, accumulate_features=False):
    """surs_mlp_grad: the gradients of SuRSNet.forward's loss with respect to every parameter of MlpParams `params`, for ONE image.
    points_mr / points_sr [3,N] (query_mr's / query_sr's points), calib_* 12 host floats, feats_lr: a list of S Img (one hr map),
    lab_lr / lab_hr [N]: what the lr / hr predictions are held against, loss_weights (mlp1, mlp2, dispweight), m_total: the number of
    points the batch's means run over.  grads: an OrderedDict as this function returns it, to overwrite (accumulate False) or add to
    (True); None: a new one (accumulate needs one).  Returns grads - keys in state_dict() order, float32 device tensors of the
    parameters' shapes ([out,in,1] weights) -, with want_preds (grads, pred_lr [S,N], pred_hr [S,N]) of the call's own forward.
    feat_grads (surs_mlp_grad_features): a FeatGrads to overwrite (accumulate_features False: whatever it held, also with N = 0) or
    add to (True), or True for a new one; it is returned last - (grads, feat_grads) or (grads, pred_lr, pred_hr, feat_grads) - and
    holds d error / d (the maps of feats_lr) and d error / d feat_hr of this image.  The parameter gradients have the same bits with
    and without it.  None: the call, launches and workspace of surs_mlp_grad."""
    S = len(feats_lr)
    if S < 1:
        raise ValueError("at least one lr feature map")
    points_mr, points_sr = _f32c(points_mr), _f32c(points_sr)
    if points_mr.dim() != 2 or points_mr.shape[0] != 3 or tuple(points_sr.shape) != tuple(points_mr.shape):
        raise ValueError("points_mr %s and points_sr %s must both be [3,N]" % (tuple(points_mr.shape), tuple(points_sr.shape)))
    n, dev = points_mr.shape[1], points_mr.device
    lab_lr, lab_hr = (_f32c(l.to(dev).reshape(-1)) for l in (lab_lr, lab_hr))
    if lab_lr.numel() != n or lab_hr.numel() != n:
        raise ValueError("labels must hold one value per point: %d" % n)
    if len(loss_weights) != 3:
        raise ValueError("loss_weights: (mlp1, mlp2, dispweight)")
    if int(m_total) < max(n, 1):
        raise ValueError("m_total %d: the means run over at least this image's %d points" % (m_total, n))
    if accumulate and grads is None:
        raise ValueError("accumulate needs the grads to add to")
    g = params
    for f in feats_lr:
        _check_feat_channels(f.c, feat_hr.c, g)
    tab = _stack_table(feats_lr, feat_hr)
    keys = mlp_param_keys(g.shapes)
    if grads is None:
        grads = OrderedDict((k, torch.empty(tuple(g.tensors[k].shape) + ((1,) if k.endswith("weight") else ()), dtype=torch.float32,
                                            device=dev)) for k in keys)
    else:
        for k in keys:
            want = tuple(g.tensors[k].shape) + ((1,) if k.endswith("weight") else ())
            if k not in grads or tuple(grads[k].shape) != want or grads[k].dtype != torch.float32 or not grads[k].is_contiguous() \
                    or grads[k].device != dev:
                raise ValueError("grads[%r] must be a contiguous float32 tensor %s on %s" % (k, want, dev))
    preds = [torch.empty((S, n), dtype=torch.float32, device=dev) if want_preds else None for _ in range(2)]
    if feat_grads is True:
        feat_grads = FeatGrads.like(feats_lr, feat_hr, dev)
    elif feat_grads is False:
        feat_grads = None
    if feat_grads is None and accumulate_features:
        raise ValueError("accumulate_features needs the feat_grads to add to")
    if feat_grads is not None:
        feat_grads.check(feats_lr, feat_hr, dev)
    need = mlp_grad_workspace_bytes(g.shapes) if feat_grads is None else mlp_grad_features_workspace_bytes(g.shapes)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=dev)
    elif workspace.numel() * workspace.element_size() < need or workspace.device != dev:
        raise ValueError("workspace: %d bytes needed on %s" % (need, dev))
    cm, cs = ((C.c_float * 12)(*[float(v) for v in c]) for c in (calib_mr, calib_sr))
    lw = (C.c_float * 3)(*[float(v) for v in loss_weights])
    f0 = feats_lr[0]
    head = (_ptr(points_mr), _ptr(points_sr), n, cm, cs, float(zmul), float(zdiv), S, tab, f0.h, f0.w, feat_hr.ptr(), feat_hr.h,
            feat_hr.w, C.byref(g.lr), C.byref(g.hr), g.table(0, "weight"), g.table(0, "bias"), g.table(1, "weight"),
            g.table(1, "bias"), _ptr(lab_lr), _ptr(lab_hr), lw, int(m_total), 1 if accumulate else 0, g.table(0, "weight", grads),
            g.table(0, "bias", grads), g.table(1, "weight", grads), g.table(1, "bias", grads), _ptr(preds[0]), _ptr(preds[1]))
    tail = (_ptr(workspace), workspace.numel() * workspace.element_size(), _stream())
    if feat_grads is None:
        check(lib().surs_mlp_grad(*head, *tail))
    else:
        maps = (C.c_void_p * S)(*[t.data_ptr() for t in feat_grads.lr])
        check(lib().surs_mlp_grad_features(*head, maps, _ptr(feat_grads.hr), 1 if accumulate_features else 0, *tail))
    out = (grads, preds[0], preds[1]) if want_preds else (grads,)
    if feat_grads is not None:
        out += (feat_grads,)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------ super-resolution gradients

def conv_grad_weight_workspace_bytes(ho, wo, cin, cout, ksize):
    """surs_conv_grad_weight_workspace_bytes: ceil(ho wo / 1024) slabs of [cout][k k cin + 1] floats."""
    n = lib().surs_conv_grad_weight_workspace_bytes(ho, wo, cin, cout, ksize)
    if n == 0:
        raise ValueError("surs_conv_grad_weight_workspace_bytes refused %dx%d, %d -> %d, k = %d" % (ho, wo, cin, cout, ksize))
    return n


def _mask_args(g, y):
    if y is None:
        return None, 0
    if (y.h, y.w, y.c) != (g.h, g.w, g.c):
        raise ValueError("the stored output %s must have the gradient's shape %s" % ((y.h, y.w, y.c), (g.h, g.w, g.c)))
    return y.ptr(), y.ld


def conv_grad_weight(g, x, ksize, stride=1, y=None, slope=1.0, dw=None, db=None, accumulate=False, workspace=None):
    """surs_conv_grad_weight: (dw [cout,cin,k,k], db [cout]) of the k x k convolution (padding k // 2) that took Img x to an Img of g's
    shape, from g = d L / d (its stored output y); y None: g is the gradient of the convolution's own result.  slope: what the
    activation's derivative is where y <= 0 (0.2 LeakyReLU, 0 ReLU).  accumulate adds to the given dw / db."""
    dev = g.buf.device
    if dw is None:
        if accumulate:
            raise ValueError("accumulate needs the dw / db to add to")
        dw = torch.empty((g.c, x.c, ksize, ksize), dtype=torch.float32, device=dev)
        db = torch.empty((g.c,), dtype=torch.float32, device=dev)
    elif tuple(dw.shape) != (g.c, x.c, ksize, ksize) or not dw.is_contiguous() or dw.dtype != torch.float32 or \
            (db is not None and (db.numel() != g.c or not db.is_contiguous() or db.dtype != torch.float32)):
        raise ValueError("dw must be a contiguous float32 %s, db %s" % ((g.c, x.c, ksize, ksize), (g.c,)))
    yp, yld = _mask_args(g, y)
    if workspace is None:
        workspace = torch.empty(conv_grad_weight_workspace_bytes(g.h, g.w, x.c, g.c, ksize) // 4, dtype=torch.float32, device=dev)
    check(lib().surs_conv_grad_weight(g.ptr(), g.h, g.w, g.c, g.ld, yp, yld, float(slope), x.ptr(), x.h, x.w, x.c, x.ld, ksize, stride,
                                      _ptr(dw), _ptr(db), 1 if accumulate else 0, _ptr(workspace),
                                      workspace.numel() * workspace.element_size(), _stream()))
    return dw, db


def conv_grad_input(g, weight, h, w, stride=1, y=None, slope=1.0, dx=None, add=False):
    """surs_conv_grad_input: Img dx [h,w,cin] = d L / d (the convolution's input) from g (as conv_grad_weight) and the plain weight
    [cout,cin,k,k] (device).  add: added to what the given dx holds."""
    weight = _f32c(weight)
    cout, cin, k, _ = weight.shape
    if cout != g.c:
        raise ValueError("weight %s against a gradient of %d channels" % (tuple(weight.shape), g.c))
    if dx is None:
        if add:
            raise ValueError("add needs the dx to add to")
        dx = Img(h, w, cin, device=g.buf.device)
    elif (dx.h, dx.w, dx.c) != (h, w, cin):
        raise ValueError("dx %s against %s" % ((dx.h, dx.w, dx.c), (h, w, cin)))
    yp, yld = _mask_args(g, y)
    check(lib().surs_conv_grad_input(g.ptr(), g.h, g.w, g.c, g.ld, yp, yld, float(slope), _ptr(weight), cin, k, stride, dx.ptr(), h, w,
                                     dx.ld, 1 if add else 0, _stream()))
    return dx


def pixel_unshuffle2_grad(g, y, slope, out=None):
    """surs_pixel_unshuffle2_grad: g, y Img [2h,2w,c] (the gradient of the shuffled map and the map itself) -> Img [h,w,4c], the
    gradient in front of conv -> LeakyReLU -> PixelShuffle(2) -> LeakyReLU's first LeakyReLU (slope = 0.2f * 0.2f there)."""
    if (y.h, y.w, y.c) != (g.h, g.w, g.c) or g.h % 2 or g.w % 2:
        raise ValueError("pixel_unshuffle2_grad: g %s / y %s must be one even-sized shape" % ((g.h, g.w, g.c), (y.h, y.w, y.c)))
    if out is None:
        out = Img(g.h // 2, g.w // 2, 4 * g.c, device=g.buf.device)
    check(lib().surs_pixel_unshuffle2_grad(g.ptr(), g.h // 2, g.w // 2, g.c, g.ld, y.ptr(), y.ld, float(slope), out.ptr(), out.ld, _stream()))
    return out


def sr_conv_names(n_block):
    """The super-resolution convolutions in SursEncoderNet's order, as (field, index, state-dict module name)."""
    names = [("head", None, "head.0")]
    names += [("down", i, "down%d.0" % (i + 1)) for i in range(3)]
    names += [("tail0", i, "tail%d.0" % (i + 1)) for i in range(3)]
    names += [("tail2", i, "tail%d.2" % (i + 1)) for i in range(3)]
    names += [(f, None, k) for f, k in (("bottleneck", "bottleneck.0"), ("bott2", "bott2.0"), ("ups2", "ups2.0"), ("ups3", "ups3.0"),
                                        ("ups4", "ups4.0"), ("last0", "last.0"), ("last2", "last.2"))]
    j = 0
    for i, nb in enumerate(n_block):
        for b in range(nb):
            for part in (0, 2):
                names.append(("body", j, "body%d.%d.body.%d" % (i + 1, b, part)))
                j += 1
    return names


def sr_param_keys(sd, n_block):
    """The state-dict keys super_res_backward returns gradients for, in sd's order: every super_resolution.* convolution (not the
    sub_mean / add_mean the forward never runs) and image_filter_hr.conv5."""
    mods = {"super_resolution." + k for _, _, k in sr_conv_names(n_block)} | {"image_filter_hr.conv5"}
    return [k for k in sd if k.rsplit(".", 1)[0] in mods and k.rsplit(".", 1)[1] in ("weight", "bias")]


class SrParams:
    """The plain fp32 weights [cout,cin,k,k] and biases [cout] of the super-resolution convolutions and conv5 on the device: what
    surs_encoder_super_res_backward reads (the forward runs on PACKED copies of the same values)."""

    def __init__(self, sd, n_block, device):
        self.n_block = [int(v) for v in n_block]
        self.keys = sr_param_keys(sd, self.n_block)
        self.tensors = _f32_tensors(sd, self.keys, device)
        want = 2 * (len(sr_conv_names(self.n_block)) + 1)
        if len(self.keys) != want:
            raise ValueError("the state dict holds %d of the %d super-resolution / conv5 parameters" % (len(self.keys), want))

    def struct(self, tensors=None):
        """SursSrParams of `tensors` (default: the parameters themselves; else an OrderedDict of gradients with the same keys).
        Returns (struct, keep-alive)."""
        t = self.tensors if tensors is None else tensors
        s = _lib.SrParamsStruct()
        n_body = max(1, 2 * sum(self.n_block))
        body = (_lib.SrParam * n_body)()
        for field, i, name in sr_conv_names(self.n_block):
            p = _lib.SrParam(t["super_resolution.%s.weight" % name].data_ptr(), t["super_resolution.%s.bias" % name].data_ptr())
            if field == "body":
                body[i] = p
            elif i is None:
                setattr(s, field, p)
            else:
                getattr(s, field)[i] = p
        s.body = body
        s.conv5 = _lib.SrParam(t["image_filter_hr.conv5.weight"].data_ptr(), t["image_filter_hr.conv5.bias"].data_ptr())
        return s, body


# the checks the taped train forwards and their backwards below share (super-resolution, ConvBlock / HourGlass, stack tail, filter_lr)

def _size(what, net, h, w):
    """The library's size query `what` - a tape's or a backward workspace's bytes - for an h x w input of _lib.EncoderNet `net`."""
    n = getattr(lib(), what)(C.byref(net), h, w)
    if n == 0:
        raise ValueError("%s refused a %dx%d input: %s" % (what, h, w, lib().surs_last_error().decode()))
    return n


def _nbytes(t):
    return t.numel() * t.element_size()


def _buffer(t, need, dev, what, aligned=True):
    """The tape or workspace `t` if it holds `need` bytes on `dev` (256-byte aligned, unless the call aligns it itself); None: a new one."""
    if t is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if _nbytes(t) < need or t.device != dev or (aligned and t.data_ptr() % 256):
        raise ValueError("%s: %d bytes needed on %s%s" % (what, need, dev, ", 256-byte aligned" if aligned else ""))
    return t


def _check_grads(grads, keys, params, dev, accumulate):
    """`grads` if it holds a contiguous float32 tensor of params[k]'s shape on `dev` for every k of `keys`; None: a new OrderedDict."""
    if accumulate and grads is None:
        raise ValueError("accumulate needs the grads to add to")
    if grads is None:
        return OrderedDict((k, torch.empty_like(params[k])) for k in keys)
    for k in keys:
        if k not in grads or tuple(grads[k].shape) != tuple(params[k].shape) or grads[k].dtype != torch.float32 \
                or not grads[k].is_contiguous() or grads[k].device != dev:
            raise ValueError("grads[%r] must be a contiguous float32 tensor %s on %s" % (k, tuple(params[k].shape), dev))
    return grads


def _check_g(g, shape, dev, name):
    """The upstream gradient `g` if it is None or a contiguous float32 NHWC tensor of `shape` on `dev`."""
    if g is None:
        return None
    if tuple(g.shape[-3:]) != shape or g.numel() != shape[0] * shape[1] * shape[2] or g.dtype != torch.float32 or not g.is_contiguous() \
            or g.device != dev:
        raise ValueError("%s must be a contiguous float32 NHWC tensor %s on %s, not %s" % (name, shape, dev, tuple(g.shape)))
    return g


def sr_tape_bytes(net, h, w):
    """surs_encoder_sr_tape_bytes: the tape of sr_train_forward for an h x w input image (net: _lib.EncoderNet)."""
    return _size("surs_encoder_sr_tape_bytes", net, h, w)


def sr_backward_workspace_bytes(net, h, w):
    """surs_encoder_sr_backward_workspace_bytes."""
    return _size("surs_encoder_sr_backward_workspace_bytes", net, h, w)


def sr_scale(net):
    """--scale as the library reads it off a _lib.EncoderNet: sr_scale with ENC_EXTENDED in flags, else 2."""
    return int(net.sr_scale) if (net.flags & _lib.ENC_EXTENDED) and net.sr_scale else 2


def sr_train_forward(net, x, scale=None, tape=None):
    """surs_encoder_super_res_train: super_res(want_image) + filter_hr of Img x [h,w,3] with every map the backward reads kept in `tape`
    (a uint8 / float32 device tensor of sr_tape_bytes, 256-byte aligned; None: a new one).  Returns (img_sr, feature_lr, feature_hr,
    im_feat_hr, tape) - the four as Img, bit for bit those of the two calls."""
    dev = x.buf.device
    tape = _buffer(tape, sr_tape_bytes(net, x.h, x.w), dev, "tape")
    if scale not in (None, sr_scale(net)):
        raise ValueError("scale %r against the net's %d" % (scale, sr_scale(net)))
    H2, W2 = sr_scale(net) * x.h, sr_scale(net) * x.w
    img_sr, f_lr, f_hr = Img(H2, W2, 3, device=dev), Img(H2 // 4, W2 // 4, 256, device=dev), Img(H2, W2, 64, device=dev)
    im_hr = Img(H2, W2, net.conv5.cout, device=dev)
    check(lib().surs_encoder_super_res_train(C.byref(net), x.ptr(), x.h, x.w, x.ld, img_sr.ptr(), f_lr.ptr(), f_hr.ptr(), im_hr.ptr(),
                                             _ptr(tape), _nbytes(tape), _stream()))
    return img_sr, f_lr, f_hr, im_hr, tape


def sr_backward(net, params, tape, h, w, g_img_sr=None, g_feature_lr=None, g_im_feat_hr=None, grads=None, accumulate=False,
                workspace=None, scale=None):
    """surs_encoder_super_res_backward for ONE image: the gradients of <g_img_sr, img_sr> + <g_feature_lr, feature_lr> + <g_im_feat_hr,
    im_feat_hr> with respect to every parameter of SrParams `params`, from the tape sr_train_forward left for the h x w input image.
    g_*: contiguous float32 NHWC device tensors of the outputs' shapes, or None (zero).  grads: an OrderedDict as returned, to
    overwrite or (accumulate) add to; None: a new one.  Returns grads: params.keys in order, tensors of the parameters' shapes."""
    dev = tape.device
    grads = _check_grads(grads, params.keys, params.tensors, dev, accumulate)
    if scale not in (None, sr_scale(net)):
        raise ValueError("scale %r against the net's %d" % (scale, sr_scale(net)))
    H2, W2 = sr_scale(net) * h, sr_scale(net) * w
    g_img_sr = _check_g(g_img_sr, (H2, W2, 3), dev, "g_img_sr")
    g_feature_lr = _check_g(g_feature_lr, (H2 // 4, W2 // 4, 256), dev, "g_feature_lr")
    g_im_feat_hr = _check_g(g_im_feat_hr, (H2, W2, net.conv5.cout), dev, "g_im_feat_hr")
    tape = _buffer(tape, sr_tape_bytes(net, h, w), dev, "tape")
    workspace = _buffer(workspace, sr_backward_workspace_bytes(net, h, w), dev, "workspace", aligned=False)   # (the library aligns it)
    ps, keep_p = params.struct()
    gs, keep_g = params.struct(grads)
    check(lib().surs_encoder_super_res_backward(C.byref(net), C.byref(ps), _ptr(tape), h, w, _ptr(g_img_sr), _ptr(g_feature_lr),
                                                _ptr(g_im_feat_hr), C.byref(gs), 1 if accumulate else 0, _ptr(workspace),
                                                _nbytes(workspace), _stream()))
    del keep_p, keep_g
    return grads


# ------------------------------------------------------------------ hourglass gradients

def groupnorm_fold(x, gamma, beta, eps=1e-5):
    """surs_groupnorm_fold: (mean [32], rstd [32], scale [c], shift [c]) of GroupNorm(32) on Img x - from x.stats where the kernel that
    wrote x left them (the convolutions' in-kernel fold, restated), else from the map (groupnorm_coeffs' launches and one more)."""
    dev = x.buf.device
    mean, rstd = torch.empty(32, dtype=torch.float32, device=dev), torch.empty(32, dtype=torch.float32, device=dev)
    scale, shift = torch.empty(x.c, dtype=torch.float32, device=dev), torch.empty(x.c, dtype=torch.float32, device=dev)
    if x.stats is not None:
        st = _lib.GnStats(x.stats.buf.data_ptr(), x.stats.slots, 0, 0, (C.c_int * 3)(x.stats.slots, x.stats.slots, x.stats.slots))
        check(lib().surs_groupnorm_fold(C.byref(st), None, x.h * x.w, x.c, x.ld, eps, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                                        _ptr(scale), _ptr(shift), None, _stream()))
    else:
        scratch = torch.empty(lib().surs_groupnorm_scratch_bytes(), dtype=torch.uint8, device=dev)
        check(lib().surs_groupnorm_fold(None, x.ptr(), x.h * x.w, x.c, x.ld, eps, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                                        _ptr(scale), _ptr(shift), _ptr(scratch), _stream()))
    return mean, rstd, scale, shift


def groupnorm_relu_grad(g, x, coeffs, gamma, dx=None, add=False, dgamma=None, dbeta=None, accumulate=False, workspace=None):
    """surs_groupnorm_relu_grad: the backward of relu(GroupNorm32(x; gamma, beta)) from g = d L / d (its output) and the site's
    groupnorm_fold() vectors `coeffs`.  Returns (dx Img, dgamma, dbeta); add: dx is added to; accumulate: dgamma / dbeta are."""
    dev = g.buf.device
    if (g.h, g.w, g.c) != (x.h, x.w, x.c):
        raise ValueError("groupnorm_relu_grad: g %s against x %s" % ((g.h, g.w, g.c), (x.h, x.w, x.c)))
    if dx is None:
        if add:
            raise ValueError("add needs the dx to add to")
        dx = Img(x.h, x.w, x.c, device=dev)
    if dgamma is None:
        if accumulate:
            raise ValueError("accumulate needs the dgamma / dbeta to add to")
        dgamma, dbeta = torch.empty(x.c, dtype=torch.float32, device=dev), torch.empty(x.c, dtype=torch.float32, device=dev)
    need = lib().surs_groupnorm_relu_grad_workspace_bytes(x.h * x.w, x.c)
    if need == 0:
        raise ValueError("surs_groupnorm_relu_grad_workspace_bytes refused %d pixels of %d channels" % (x.h * x.w, x.c))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    mean, rstd, scale, shift = coeffs
    check(lib().surs_groupnorm_relu_grad(g.ptr(), g.ld, x.ptr(), x.ld, x.h * x.w, x.c, _ptr(mean), _ptr(rstd), _ptr(scale), _ptr(shift),
                                         _ptr(_f32c(gamma)), dx.ptr(), dx.ld, 1 if add else 0, _ptr(_f32c(dgamma)), _ptr(_f32c(dbeta)),
                                         1 if accumulate else 0, _ptr(workspace), workspace.numel() * workspace.element_size(), _stream()))
    return dx, dgamma, dbeta


def avgpool2_grad(g, dx=None, add=False):
    """surs_avgpool2_grad: Img g [h,w,c] -> Img dx [2h,2w,c] (+)= 0.25 g[y // 2][x // 2]."""
    if dx is None:
        if add:
            raise ValueError("add needs the dx to add to")
        dx = Img(2 * g.h, 2 * g.w, g.c, device=g.buf.device)
    elif (dx.h, dx.w, dx.c) != (2 * g.h, 2 * g.w, g.c):
        raise ValueError("avgpool2_grad: dx %s against g %s" % ((dx.h, dx.w, dx.c), (g.h, g.w, g.c)))
    check(lib().surs_avgpool2_grad(g.ptr(), g.h, g.w, g.c, g.ld, dx.ptr(), dx.ld, 1 if add else 0, _stream()))
    return dx


def bicubic_up2_grad(g, dx=None, add=False):
    """surs_bicubic_up2_grad: Img g [2h,2w,c] -> Img dx [h,w,c], the transpose of bicubic_up2(align_corners=True)."""
    if g.h % 2 or g.w % 2:
        raise ValueError("bicubic_up2_grad: g %s must have an even size" % ((g.h, g.w, g.c),))
    if dx is None:
        if add:
            raise ValueError("add needs the dx to add to")
        dx = Img(g.h // 2, g.w // 2, g.c, device=g.buf.device)
    elif (2 * dx.h, 2 * dx.w, dx.c) != (g.h, g.w, g.c):
        raise ValueError("bicubic_up2_grad: dx %s against g %s" % ((dx.h, dx.w, dx.c), (g.h, g.w, g.c)))
    check(lib().surs_bicubic_up2_grad(g.ptr(), dx.h, dx.w, g.c, g.ld, dx.ptr(), dx.ld, 1 if add else 0, _stream()))
    return dx


HG = "image_filter_lr."
_BLOCK_FIELDS = (("weight", ("conv1.weight", "conv2.weight", "conv3.weight")), ("gamma", ("bn1.weight", "bn2.weight", "bn3.weight")),
                 ("beta", ("bn1.bias", "bn2.bias", "bn3.bias")))


def hg_block_prefixes(stack, depth):
    """The ConvBlocks of image_filter_lr.m{stack} in module order (SursEncoderNet.hg's): b1_d, b2_d, [level d - 1], b2_plus_1, b3_1, ..."""
    out = []

    def gen(level):
        out.append(HG + "m%d.b1_%d." % (stack, level))
        out.append(HG + "m%d.b2_%d." % (stack, level))
        if level > 1:
            gen(level - 1)
        else:
            out.append(HG + "m%d.b2_plus_%d." % (stack, level))
        out.append(HG + "m%d.b3_%d." % (stack, level))
    gen(depth)
    return out


def hg_block_keys(prefix):
    """The nine tensors of a ConvBlock the forward reads (bn4 belongs to the downsample path in_planes == out_planes never takes)."""
    return [prefix + k for k in ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
                                 "bn3.weight", "bn3.bias")]


def hg_param_keys(sd, num_stack, depth):
    """Every image_filter_lr.* key the forward reads, in sd's order: the ConvBlocks' nine tensors each and the stacks' 1 x 1 tails."""
    want = set(hg_block_keys(HG + "conv2."))
    for s in range(num_stack):
        for p in hg_block_prefixes(s, depth) + [HG + "top_m_%d." % s]:
            want |= set(hg_block_keys(p))
        tails = ["conv_last%d" % s, "bn_end%d" % s, "l%d" % s] + (["bl%d" % s, "al%d" % s] if s < num_stack - 1 else [])
        want |= {HG + t + e for t in tails for e in (".weight", ".bias")}
    return [k for k in sd if k in want]


class HgParams:
    """The plain fp32 device copies of hg_param_keys(): what the hourglass backward reads (the forward runs on packed copies)."""

    def __init__(self, sd, num_stack, depth, device):
        self.num_stack, self.depth = int(num_stack), int(depth)
        self.keys = hg_param_keys(sd, self.num_stack, self.depth)
        self.tensors = _f32_tensors(sd, self.keys, device)

    @staticmethod
    def struct(prefixes, tensors):
        """(ctypes array of SursHgBlockParams for the blocks `prefixes`, over `tensors`: key -> contiguous float32 device tensor)."""
        arr = (_lib.HgBlockParams * len(prefixes))()
        for i, p in enumerate(prefixes):
            for field, names in _BLOCK_FIELDS:
                for k, n in enumerate(names):
                    getattr(arr[i], field)[k] = _f32c(tensors[p + n]).data_ptr()
        return arr


def hg_block_of(net, prefix, depth):
    """The SursConvBlock of _lib.EncoderNet `net` behind a state-dict prefix (image_filter_lr.conv2. / .top_m_{s}. / .m{s}.b*_{l}.)."""
    name = prefix[len(HG):].rstrip(".") if prefix.startswith(HG) else None
    if name == "conv2":
        return net.conv2
    if name and name.startswith("top_m_") and name[6:].isdigit() and int(name[6:]) < net.num_stack:
        return net.top_m[int(name[6:])]
    if name and name.startswith("m") and "." in name and name[1:name.index(".")].isdigit():
        s = int(name[1:name.index(".")])
        pre = hg_block_prefixes(s, depth)
        if s < net.num_stack and prefix in pre:
            return net.hg[s * len(pre) + pre.index(prefix)]
    raise ValueError("%r is no ConvBlock of image_filter_lr" % (prefix,))


def hg_tape_bytes(net, h, w, hourglass):
    """surs_encoder_hourglass_tape_bytes / surs_encoder_convblock_tape_bytes."""
    return _size("surs_encoder_%s_tape_bytes" % ("hourglass" if hourglass else "convblock"), net, h, w)


def hg_backward_workspace_bytes(net, h, w, hourglass):
    return _size("surs_encoder_%s_backward_workspace_bytes" % ("hourglass" if hourglass else "convblock"), net, h, w)


def hg_train_forward(net, which, x, tape=None):
    """surs_encoder_convblock_train (which: a _lib.ConvBlock of net) / surs_encoder_hourglass_train (which: the stack's index) of Img x
    [h,w,256].  Returns (out Img - encoder.conv_block's / encoder.hourglass's bits on the same statistics-free x -, tape)."""
    dev = x.buf.device
    hourglass = isinstance(which, int)
    if x.c != 256:
        raise ValueError("a map of 256 channels is expected, not %d" % x.c)
    tape = _buffer(tape, hg_tape_bytes(net, x.h, x.w, hourglass), dev, "tape")
    out = Img(x.h, x.w, 256, device=dev)
    tb = _nbytes(tape)
    if hourglass:
        check(lib().surs_encoder_hourglass_train(C.byref(net), which, x.ptr(), x.h, x.w, x.ld, out.ptr(), _ptr(tape), tb, _stream()))
    else:
        check(lib().surs_encoder_convblock_train(C.byref(net), C.byref(which), x.ptr(), x.h, x.w, x.ld, out.ptr(), _ptr(tape), tb, _stream()))
    return out, tape


def hg_backward(net, which, prefixes, params, tape, h, w, g, grads=None, accumulate=False, workspace=None):
    """surs_encoder_convblock_backward / surs_encoder_hourglass_backward for ONE image: g = d L / d out, a contiguous float32 NHWC device
    tensor [h,w,256]; prefixes: the module's ConvBlock prefixes in its order (one for a block, hg_block_prefixes for an hourglass);
    params: key -> plain fp32 device tensor (HgParams.tensors).  grads: an OrderedDict as returned, to overwrite or (accumulate) add
    to.  Returns (dx [h,w,256] tensor, grads: the module's keys in prefix order)."""
    dev = tape.device
    hourglass = isinstance(which, int)
    keys = [k for p in prefixes for k in hg_block_keys(p)]
    grads = _check_grads(grads, keys, params, dev, accumulate)
    if g is None:
        raise ValueError("hg_backward: the gradient is None")
    g = _check_g(g, (h, w, 256), dev, "g")
    tape = _buffer(tape, hg_tape_bytes(net, h, w, hourglass), dev, "tape")
    workspace = _buffer(workspace, hg_backward_workspace_bytes(net, h, w, hourglass), dev, "workspace")
    ps, gs = HgParams.struct(prefixes, params), HgParams.struct(prefixes, grads)
    dx = torch.empty((h, w, 256), dtype=torch.float32, device=dev)
    wb = _nbytes(workspace)
    if hourglass:
        check(lib().surs_encoder_hourglass_backward(C.byref(net), which, ps, _ptr(tape), h, w, _ptr(g), _ptr(dx), gs, 1 if accumulate else 0,
                                                    _ptr(workspace), wb, _stream()))
    else:
        check(lib().surs_encoder_convblock_backward(C.byref(net), C.byref(which), ps, _ptr(tape), h, w, _ptr(g), _ptr(dx), gs,
                                                    1 if accumulate else 0, _ptr(workspace), wb, _stream()))
    return dx, grads


# ------------------------------------------------------------------ stack-tail gradients, and the whole low-resolution filter

def tail_joint_grad(g_out, g_next, w_al, w_l, w_bl, d_out=None, d_a=None):
    """surs_tail_joint_grad: (dOut Img [h,w,D], dA Img [h,w,256]) = (g_out + g_next W_al, dOut W_l + g_next W_bl) in one launch, from
    Img g_out [h,w,D] and g_next [h,w,256] (either None = zero, not both) and the plain weights al [256,D,1,1], l [D,256,1,1],
    bl [256,256,1,1] (device; al and bl are read only with g_next)."""
    ref = g_out if g_out is not None else g_next
    if ref is None:
        raise ValueError("tail_joint_grad: both gradients are None")
    w_l = _f32c(w_l)
    D, h, w, dev = w_l.shape[0], ref.h, ref.w, ref.buf.device
    if w_l.numel() != D * 256 or (g_out is not None and g_out.c != D) or (g_next is not None and g_next.c != 256):
        raise ValueError("tail_joint_grad: l %s against g_out / g_next of %s / %s channels"
                         % (tuple(w_l.shape), g_out and g_out.c, g_next and g_next.c))
    if g_next is not None and (_f32c(w_al).numel() != 256 * D or _f32c(w_bl).numel() != 256 * 256 or (g_next.h, g_next.w) != (h, w)):
        raise ValueError("tail_joint_grad: al %s, bl %s against D = %d" % (tuple(w_al.shape), tuple(w_bl.shape), D))
    d_out = Img(h, w, D, device=dev) if d_out is None else d_out
    d_a = Img(h, w, 256, device=dev) if d_a is None else d_a
    if (d_out.h, d_out.w, d_out.c) != (h, w, D) or (d_a.h, d_a.w, d_a.c) != (h, w, 256):
        raise ValueError("tail_joint_grad: outputs of %s / %s" % ((h, w, D), (h, w, 256)))
    check(lib().surs_tail_joint_grad(g_out.ptr() if g_out is not None else None, g_out.ld if g_out is not None else 0,
                                     g_next.ptr() if g_next is not None else None, g_next.ld if g_next is not None else 0,
                                     _ptr(w_al) if g_next is not None else None, _ptr(w_l), _ptr(w_bl) if g_next is not None else None,
                                     h * w, D, d_out.ptr(), d_out.ld, d_a.ptr(), d_a.ld, _stream()))
    return d_out, d_a


def hg_tail_keys(stack, num_stack):
    """The tail of stack `stack`: conv_last, bn_end, l and - not for the last stack - bl, al, .weight and .bias each."""
    names = ["conv_last%d", "bn_end%d", "l%d"] + (["bl%d", "al%d"] if stack < num_stack - 1 else [])
    return [HG + n % stack + e for n in names for e in (".weight", ".bias")]


def _fill_tail(t, stack, num_stack, tensors):
    for field in ("conv_last", "l") + (("bl", "al") if stack < num_stack - 1 else ()):
        getattr(t, field).weight = _f32c(tensors[HG + "%s%d.weight" % (field, stack)]).data_ptr()
        getattr(t, field).bias = _f32c(tensors[HG + "%s%d.bias" % (field, stack)]).data_ptr()
    t.gamma = _f32c(tensors[HG + "bn_end%d.weight" % stack]).data_ptr()
    t.beta = _f32c(tensors[HG + "bn_end%d.bias" % stack]).data_ptr()


def hg_tail_struct(stack, num_stack, tensors):
    """SursHgTailParams of stack `stack` over `tensors`: key -> contiguous float32 device tensor."""
    t = _lib.HgTailParams()
    _fill_tail(t, stack, num_stack, tensors)
    return t


def hg_filter_struct(num_stack, depth, tensors):
    """(SursHgFilterParams over `tensors`, the ctypes arrays behind its pointers - keep them alive for the call)."""
    pre = [p for s in range(num_stack) for p in hg_block_prefixes(s, depth)]
    hg = HgParams.struct(pre, tensors)
    top = HgParams.struct([HG + "top_m_%d." % s for s in range(num_stack)], tensors)
    tails = (_lib.HgTailParams * num_stack)()
    for s in range(num_stack):
        _fill_tail(tails[s], s, num_stack, tensors)
    f = _lib.HgFilterParams(HgParams.struct([HG + "conv2."], tensors)[0], hg, top, tails)
    return f, (hg, top, tails)


def tail_tape_bytes(net, h, w):
    return _size("surs_encoder_tail_tape_bytes", net, h, w)


def tail_backward_workspace_bytes(net, h, w):
    return _size("surs_encoder_tail_backward_workspace_bytes", net, h, w)


def filter_lr_tape_bytes(net, h, w):
    return _size("surs_encoder_filter_lr_tape_bytes", net, h, w)


def filter_lr_backward_workspace_bytes(net, h, w):
    return _size("surs_encoder_filter_lr_backward_workspace_bytes", net, h, w)


def tail_train_forward(net, stack, ll, previous=None, tape=None):
    """surs_encoder_tail_train: the tail of stack `stack` on Img ll [h,w,256] and - every stack but the last - Img previous [h,w,256].
    Returns (out Img [h,w,D], next Img [h,w,256] or None, tape): the bits of filter_lr()'s tail on the same maps."""
    dev, last = ll.buf.device, stack == net.num_stack - 1
    if ll.c != 256 or (previous is not None and (previous.h, previous.w, previous.c) != (ll.h, ll.w, 256)):
        raise ValueError("maps of 256 channels and one size are expected")
    if last != (previous is None):
        raise ValueError("previous goes with every stack but the last (stack %d of %d)" % (stack, net.num_stack))
    tape = _buffer(tape, tail_tape_bytes(net, ll.h, ll.w), dev, "tape")
    out = Img(ll.h, ll.w, net.l[stack].cout, device=dev)
    nxt = None if last else Img(ll.h, ll.w, 256, device=dev)
    check(lib().surs_encoder_tail_train(C.byref(net), stack, ll.ptr(), ll.ld, None if last else previous.ptr(), 0 if last else previous.ld,
                                        ll.h, ll.w, out.ptr(), None if last else nxt.ptr(), _ptr(tape), _nbytes(tape), _stream()))
    return out, nxt, tape


def tail_backward(net, stack, params, tape, h, w, g_out=None, g_next=None, grads=None, accumulate=False, workspace=None):
    """surs_encoder_tail_backward for ONE image: g_out [h,w,D], g_next [h,w,256] contiguous float32 NHWC device tensors (None: zero, not
    both); params: key -> plain fp32 device tensor.  Returns (d_ll [h,w,256] tensor, grads over hg_tail_keys(stack))."""
    dev, S = tape.device, net.num_stack
    keys = hg_tail_keys(stack, S)
    grads = _check_grads(grads, keys, params, dev, accumulate)
    g_out = _check_g(g_out, (h, w, net.l[stack].cout), dev, "g_out")
    g_next = _check_g(g_next, (h, w, 256), dev, "g_next")
    if g_out is None and g_next is None:
        raise ValueError("tail_backward: both gradients are None")
    tape = _buffer(tape, tail_tape_bytes(net, h, w), dev, "tape")
    workspace = _buffer(workspace, tail_backward_workspace_bytes(net, h, w), dev, "workspace")
    ps, gs = hg_tail_struct(stack, S, params), hg_tail_struct(stack, S, grads)
    d_ll = torch.empty((h, w, 256), dtype=torch.float32, device=dev)
    check(lib().surs_encoder_tail_backward(C.byref(net), stack, C.byref(ps), _ptr(tape), h, w, _ptr(g_out), _ptr(g_next), _ptr(d_ll),
                                           C.byref(gs), 1 if accumulate else 0, _ptr(workspace), _nbytes(workspace), _stream()))
    return d_ll, grads


def filter_lr_train_forward(net, x, tape=None):
    """surs_encoder_filter_lr_train of Img x [h,w,256]: (the list of every stack's output Img [h,w,D], tape)."""
    dev, S = x.buf.device, net.num_stack
    if x.c != 256:
        raise ValueError("a map of 256 channels is expected, not %d" % x.c)
    tape = _buffer(tape, filter_lr_tape_bytes(net, x.h, x.w), dev, "tape")
    outs = [Img(x.h, x.w, net.l[s].cout, device=dev) for s in range(S)]
    ptrs = (C.c_void_p * S)(*[o.ptr() for o in outs])
    check(lib().surs_encoder_filter_lr_train(C.byref(net), x.ptr(), x.h, x.w, x.ld, ptrs, _ptr(tape), _nbytes(tape), _stream()))
    return outs, tape


def filter_lr_backward(net, depth, keys, params, tape, h, w, g_outs, grads=None, accumulate=False, workspace=None):
    """surs_encoder_filter_lr_backward for ONE image: g_outs: per stack a contiguous float32 NHWC device tensor [h,w,D] or None (zero;
    not all); keys: hg_param_keys() - the order of the returned grads; params: key -> plain fp32 device tensor.  Returns
    (d_feature_lr [h,w,256] tensor, grads)."""
    dev, S = tape.device, net.num_stack
    grads = _check_grads(grads, keys, params, dev, accumulate)
    if len(g_outs) != S:
        raise ValueError("one gradient (or None) per stack: %d for %d stacks" % (len(g_outs), S))
    g_outs = [_check_g(g, (h, w, net.l[s].cout), dev, "g_outs[%d]" % s) for s, g in enumerate(g_outs)]
    if all(g is None for g in g_outs):
        raise ValueError("filter_lr_backward: every gradient is None")
    tape = _buffer(tape, filter_lr_tape_bytes(net, h, w), dev, "tape")
    workspace = _buffer(workspace, filter_lr_backward_workspace_bytes(net, h, w), dev, "workspace")
    (ps, keep_p), (gs, keep_g) = hg_filter_struct(S, depth, params), hg_filter_struct(S, depth, grads)
    ptrs = (C.c_void_p * S)(*[None if g is None else g.data_ptr() for g in g_outs])
    dx = torch.empty((h, w, 256), dtype=torch.float32, device=dev)
    check(lib().surs_encoder_filter_lr_backward(C.byref(net), C.byref(ps), _ptr(tape), h, w, ptrs, _ptr(dx), C.byref(gs),
                                                1 if accumulate else 0, _ptr(workspace), _nbytes(workspace), _stream()))
    del keep_p, keep_g
    return dx, grads


def query_points_views(points, calibs, projection, zmul, zdiv, feat_lr, feat_hr, blob, ws, want_logits=False):
    """Multi-view / perspective query.  points [V,3,N] f32 device tensor; calibs [V,12] (host); feat_lr [V,hl,wl,256] and
    feat_hr [V,hh,wh,64] contiguous NHWC device tensors; projection 'orthogonal' | 'perspective'.
    Returns pred_hr [V,N], pred_lr [V,N][, logit_hr [N], logit_lr [N]]."""
    points = _f32c(points)
    V, _, n = points.shape
    dev = points.device
    feat_lr, feat_hr = _f32c(feat_lr), _f32c(feat_hr)
    assert feat_lr.shape[0] == V and feat_hr.shape[0] == V and feat_lr.shape[3] == 256 and feat_hr.shape[3] == 64
    phr = torch.empty((V, n), dtype=torch.float32, device=dev)
    plr = torch.empty_like(phr)
    lg = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)] if want_logits else [None, None]
    cal = np.ascontiguousarray(np.asarray(calibs, np.float32).reshape(V, -1)[:, :12])
    cbuf = (C.c_float * (12 * V))(*[float(v) for v in cal.reshape(-1)])
    w = ws.get(lib().surs_query_views_workspace_bytes(n, V))
    check(lib().surs_query_points_views(_ptr(points), n, V, {"orthogonal": 0, "perspective": 1}[projection], cbuf, float(zmul),
                                        float(zdiv), _ptr(feat_lr), feat_lr.shape[1], feat_lr.shape[2], _ptr(feat_hr),
                                        feat_hr.shape[1], feat_hr.shape[2], _ptr(blob), _ptr(w), w.numel(), _ptr(phr), _ptr(plr),
                                        _ptr(lg[0]) if want_logits else None, _ptr(lg[1]) if want_logits else None, _stream()))
    return (phr, plr, lg[0], lg[1]) if want_logits else (phr, plr)


def query_grid_views(i0, i1, ry, rz, mat, calibs, projection, zmul, zdiv, feat_lr, feat_hr, blob, ws, vol_hr=None, vol_lr=None):
    """surs_query_grid_views: the dense sweep of a multi-view / perspective model over the grid slab [i0, i1) - every voxel seen by
    every view, view 0's predictions kept (lib/mesh_util.py:20-28).  calibs [V,12] (host); feat_lr [V,hl,wl,256], feat_hr [V,hh,wh,64]
    contiguous NHWC device tensors.  Returns (vol_hr, vol_lr) [(i1-i0), ry, rz]."""
    feat_lr, feat_hr = _f32c(feat_lr), _f32c(feat_hr)
    V = feat_lr.shape[0]
    dev = blob.device
    assert feat_hr.shape[0] == V and feat_lr.shape[3] == 256 and feat_hr.shape[3] == 64
    if vol_hr is None:
        vol_hr = torch.empty((i1 - i0, ry, rz), dtype=torch.float32, device=dev)
        vol_lr = torch.empty_like(vol_hr)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = np.ascontiguousarray(np.asarray(calibs, np.float32).reshape(V, -1)[:, :12])
    cbuf = (C.c_float * (12 * V))(*[float(v) for v in cal.reshape(-1)])
    w = ws.get(lib().surs_query_grid_views_workspace_bytes(V))
    check(lib().surs_query_grid_views(i0, i1, ry, rz, m, V, {"orthogonal": 0, "perspective": 1}[projection], cbuf, float(zmul),
                                      float(zdiv), _ptr(feat_lr), feat_lr.shape[1], feat_lr.shape[2], _ptr(feat_hr), feat_hr.shape[1],
                                      feat_hr.shape[2], _ptr(blob), _ptr(w), w.numel(), _ptr(vol_hr), _ptr(vol_lr), _stream()))
    return vol_hr, vol_lr


def query_grid(i0, i1, ry, rz, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, dtype, ws, vol_hr=None, vol_lr=None, kernel=0,
               operand_parts=0):
    """Dense sweep of grid slab [i0, i1): returns (vol_hr, vol_lr) float32 device tensors [(i1-i0), ry, rz].
    kernel: column-kernel version for this call (grid_kernel_for's choice; 0 = the library's default / process setting);
    operand_parts: 2 / 3 = operand split of the fp32-grade GEMMs behind this sweep (0 = process setting).  Both travel in the
    call's SursGridOptions: no process-wide state is touched."""
    dev = blob.device
    if vol_hr is None:
        vol_hr = torch.empty((i1 - i0, ry, rz), dtype=torch.float32, device=dev)
        vol_lr = torch.empty_like(vol_hr)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    code = DTYPES[dtype] if isinstance(dtype, str) else dtype
    need = lib().surs_query_grid_workspace_bytes(ry, rz, code)
    w = ws.get(need)
    opt = _lib.GridOptions(int(kernel), int(operand_parts))
    check(lib().surs_query_grid_opt(i0, i1, ry, rz, m, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w,
                                    feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob), code, _ptr(w), w.numel(), _ptr(vol_hr),
                                    _ptr(vol_lr), C.byref(opt), _stream()))
    return vol_hr, vol_lr


# mean listed channels per tile above which the dense column kernels are the faster ones (profiles/r03_listed_sensitivity.json:
# the eight-wave bf16 / fp16 kernel still wins at 490 listed - 254 against 290 ms at 512^3 - and gains 0.3 ms per listed channel)
LISTED_DENSE_THRESHOLD = 400.0
LISTED_DENSE_THRESHOLDS = {"fp32": 400.0, "bf16": 600.0, "fp16": 600.0}
# bf16 / fp16: mean listed channels per tile up to which the streamed two-workgroup kernel (12) is used; above it the eight-wave kernel
# (10), whose chunks of 96 channels loop: kernel 12 stages 144 channels per tile and hands fuller tiles to kernel 10 one by one, which
# pays only while they are rare (bench field: 70 listed, one tile in 10^4; layer-0 depth gain 16: 212 listed, 264 against 233 ms)
LISTED_STREAM_THRESHOLD = 96.0


def probe_listed(i_plane, ry, rz, tile, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws):
    """surs_query_grid_probe: (mean listed layer-0 channels per z tile for the lr classifier, upper bound for hr), or
    (-1, -1) where the column kernels do not apply.  Synchronises the stream."""
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    need = lib().surs_query_grid_workspace_bytes(ry, rz, DTYPES["bf16"])
    w = ws.get(need)
    out = (C.c_float * 2)(-1.0, -1.0)
    check(lib().surs_query_grid_probe(int(i_plane), ry, rz, tile, m, cal, float(zmul), float(zdiv), feat_lr.ptr(), feat_lr.h,
                                      feat_lr.w, feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob), _ptr(w), w.numel(), out, _stream()))
    return float(out[0]), float(out[1])


def grid_kernel_for(rx, ry, rz, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, dtype, ws):
    """Column-kernel version for a sweep of the rx x ry x rz grid `mat` describes.  fp32: 0 (the library's default, 11: layer 1
    restated along the column) unless the probe says the sweep lists so many channels per tile that the dense kernel (5) is
    faster.  bf16 / fp16: 12 (restated, layer 1 streamed into layer 2, two workgroups per CU) while the probe's mean stays under
    LISTED_STREAM_THRESHOLD, 10 (restated, eight waves) above it, 3 (dense) above LISTED_DENSE_THRESHOLDS.  A deterministic function of the grid, the calibration, the features and
    the weights - the middle axis-0 plane of the WHOLE grid is probed, so every slab and every rank of a sharded sweep makes
    the same choice.  Probed on every call (one plane of column constants, about 0.3 ms and a stream synchronisation): the
    feature buffers are written through raw pointers into recycled allocator blocks, so nothing the host can see tells one
    subject's features from the next one's.  SURS_GRID_AUTO=0 or an explicit SURS_GRID_KERNEL / SURS_GRID_F32_KERNEL turn it
    off.  The last decision is left in ws.kernel_choice = (kernel, listed channels per tile) for reports."""
    if settings.get("SURS_GRID_AUTO") == "0" or settings.is_set("SURS_GRID_KERNEL") or settings.is_set("SURS_GRID_F32_KERNEL"):
        return 0
    if dtype not in ("fp32", "bf16", "fp16") or ry > 16384:
        return 0
    lr, _ = probe_listed(rx // 2, ry, rz, 64 if dtype == "fp32" else 128, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws)
    kern = (5 if dtype == "fp32" else 3) if lr > LISTED_DENSE_THRESHOLDS[dtype] else 0
    if kern == 0 and dtype != "fp32":
        kern = 12 if lr <= LISTED_STREAM_THRESHOLD else 10
    ws.kernel_choice = (kern, lr)
    ws.probes = getattr(ws, "probes", 0) + 1
    return kern


# ------------------------------------------------------------------ marching cubes

def marching_cubes_lewiner(vol, level, ws, want_normals=True, key=None):
    """vol: float32 device tensor [n0,n1,n2].  Returns device tensors (verts [V,3] f32, faces [F,3] i32, normals, values).
    Raises ValueError / RuntimeError like skimage.measure.marching_cubes_lewiner."""
    if vol.dim() != 3:
        raise ValueError("Input volume should be a 3D numpy array.")
    if min(vol.shape) < 2:
        raise ValueError("Input array must be at least 2x2x2.")
    vol = _f32c(vol.to(torch.float32).contiguous())
    n0, n1, n2 = vol.shape
    w = ws.get(lib().surs_mc_workspace_bytes(n0, n1, n2))
    counts = _lib.McCounts()
    dev = vol.device

    def run(cap_v, cap_f):
        verts = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((cap_f, 3), dtype=torch.int32, device=dev)
        normals = torch.empty((cap_v, 3), dtype=torch.float32, device=dev) if want_normals else None
        values = torch.empty((cap_v,), dtype=torch.float32, device=dev) if want_normals else None
        rc = lib().surs_mc_lewiner(_ptr(vol), n0, n1, n2, float(level), _ptr(w), w.numel(), _ptr(verts), _ptr(normals),
                                   _ptr(values), cap_v, _ptr(faces), cap_f, C.byref(counts), _stream())
        return rc, verts, faces, normals, values

    if ws.mc_capacity.get(key) is None:
        # first extraction with this workspace: counting pass (no outputs) to size the buffers
        check(lib().surs_mc_lewiner(_ptr(vol), n0, n1, n2, float(level), _ptr(w), w.numel(), None, None, None, 0, None, 0,
                                    C.byref(counts), _stream()))
        cap = (counts.n_verts, counts.n_faces)
    else:
        cap = ws.mc_capacity[key]
    rc, verts, faces, normals, values = run(*cap)
    if rc == -6:   # SURS_E_CAPACITY: the counts are filled in, retry with exact sizes
        rc, verts, faces, normals, values = run(counts.n_verts, counts.n_faces)
    check(rc)
    nv, nf = counts.n_verts, counts.n_faces
    ws.mc_capacity[key] = mesh_capacity(nv, nf)
    _warm_stream_buffers(ws, key)
    if key is not None and (ws.mesh_ws.get(key) is None or ws.mesh_ws[key].numel() < w.numel()):
        ws.mesh_ws[key] = torch.empty(w.numel(), dtype=torch.uint8, device=dev)   # the field's own tables (MeshStream)
    return (verts[:nv], faces[:nf], normals[:nv] if normals is not None else None,
            values[:nv] if values is not None else None)


def mesh_capacity(nv, nf):
    """Buffer sizes for the next extraction of a field that last had nv vertices / nf faces: 12.5 % head-room, rounded up
    to 2^20 vertices / 2^21 faces so that meshes of similar size ask the caching allocators (device and pinned host) for
    blocks of the same size and get the previous reconstruction's blocks back."""
    gv, gf = 1 << 20, 1 << 21
    return (-(-(int(nv * 1.125) + 1024) // gv) * gv, -(-(int(nf * 1.125) + 2048) // gf) * gf)


def _warm_stream_buffers(ws, key):
    """The streamed extraction (MeshStream) keeps its results in pinned host buffers of the capacity sizes.  Allocating
    pinned memory is slow (17 - 140 ms for the bench's 1 GB, depending on the box) and torch's caching host allocator only
    recycles blocks of a matching size: allocate and release them here, in the one-piece extraction that sizes the
    buffers, so that the first streamed reconstruction already finds them cached."""
    cap = ws.mc_capacity[key]
    warm = getattr(ws, "_pinned_warm", None)
    if warm is None:
        warm = ws._pinned_warm = {}
    if warm.get(key) == cap:
        return
    a = torch.empty((cap[0], 3), dtype=torch.float64, pin_memory=True)
    b = torch.empty((cap[1], 3), dtype=torch.int32, pin_memory=True)
    # ... and the device buffers of a MeshStream (hipMalloc is slow too, and synchronises)
    d = [torch.empty((cap[0], 3), dtype=torch.float32, device=ws.device), torch.empty((cap[0], 3), dtype=torch.float64, device=ws.device),
         torch.empty((cap[1], 3), dtype=torch.int32, device=ws.device), torch.empty((cap[0], 3), dtype=torch.float32, device=ws.device),
         torch.empty((cap[0],), dtype=torch.float32, device=ws.device)]
    del a, b, d
    warm[key] = cap
    # ... and the field's extraction stream: the first use of a HIP stream creates its hardware queue (milliseconds)
    known = len(_shared_streams)
    st = shared_stream(ws.device, ("mc", key))
    if len(_shared_streams) > known:
        with torch.cuda.stream(st):
            torch.zeros(1, device=ws.device).cpu()   # (a pageable read-back like the extraction's counts)


class MeshStream:
    """Incremental Lewiner extraction of ONE field while the dense sweep is still writing it (surs_mc_lewiner_range): after
    every advance() the new vertices are transformed to world space and they and the new faces start their way to
    pinned host memory on the workspace's copy stream, under the sweep launches that follow.  Buffers are sized from the
    field's previous extraction (ws.mc_capacity[key]); `overflow` is set if that turns out too small - the caller then
    extracts the finished volume in one piece."""

    def __init__(self, ws, key, vol, mat, level=0.5, want_normals=True, zoff=None):
        """zoff (slab mode, dist.reconstruction_sharded): `vol` is one axis-0 slab of a larger grid whose plane 0 is the grid's
        plane zoff and whose last plane is the next slab's first (halo); vertices and faces stay on the device, numbered
        locally, faces of the first cell layer referring to the slab below as surs_mc_lewiner_range_slab describes;
        finish() then returns device tensors and leaves the level-range / no-surface checks to the caller."""
        self.ws, self.key, self.vol, self.level, self.want = ws, key, vol, float(level), want_normals
        self.zoff = zoff
        if zoff is not None and want_normals:
            raise NotImplementedError("slab mode extracts vertices and faces only (normals accumulate across slabs)")
        self.n0, self.n1, self.n2 = vol.shape
        dev = vol.device
        self.cap_v, self.cap_f = ws.mc_capacity[key]
        need = lib().surs_mc_workspace_bytes(self.n0, self.n1, self.n2)
        w = ws.mesh_ws.get(key)
        if w is None or w.numel() < need:
            w = ws.mesh_ws[key] = torch.empty(int(need), dtype=torch.uint8, device=dev)   # holds the edge tables between calls
        self.w = w
        self.verts = torch.empty((self.cap_v, 3), dtype=torch.float32, device=dev)
        self.world = torch.empty((self.cap_v, 3), dtype=torch.float64, device=dev)
        self.faces = torch.empty((self.cap_f, 3), dtype=torch.int32, device=dev)
        self.normals = torch.empty((self.cap_v, 3), dtype=torch.float32, device=dev) if want_normals else None
        self.values = torch.empty((self.cap_v,), dtype=torch.float32, device=dev) if want_normals else None
        if zoff is None:
            self.h_world = torch.empty((self.cap_v, 3), dtype=torch.float64, pin_memory=True)
            self.h_faces = torch.empty((self.cap_f, 3), dtype=torch.int32, pin_memory=True)
        self.mat = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
        self.run = _lib.McCounts(0, 0, 3.4028234663852886e38, -3.4028234663852886e38)
        self.layers = 0          # cell layers (axis 0) extracted so far
        self.sent_v = self.sent_f = 0
        self.overflow = False
        self.side = shared_stream(dev, "copy")
        # the extraction runs on a stream of its own (one per field): its kernels and its count read-backs (host syncs)
        # then neither sit between two launches of the sweep nor keep the host from enqueueing the next launch
        self.mc = shared_stream(dev, ("mc", key))
        self.mc.wait_stream(torch.cuda.current_stream(dev))   # the buffers above were allocated on the caller's stream
        for t in (self.world, self.faces):
            t.record_stream(self.side)
        for t in (self.verts, self.world, self.faces, self.normals, self.values, vol):
            if t is not None:
                t.record_stream(self.mc)

    def advance(self, layer_end, after=None):
        """Extract the cell layers [self.layers, layer_end): the voxel planes up to layer_end must be final - or final once
        the event `after` (recorded on the sweep's stream) has happened."""
        with torch.cuda.stream(self.mc):
            if after is not None:
                self.mc.wait_event(after)
            self._advance(layer_end)

    def _advance(self, layer_end):
        layer_end = min(int(layer_end), self.n0 - 1)
        if self.overflow or layer_end <= self.layers:
            return
        if self.zoff is not None:
            rc = lib().surs_mc_lewiner_range_slab(_ptr(self.vol), self.n0, self.n1, self.n2, self.layers, layer_end, self.level,
                                                  _ptr(self.w), self.w.numel(), _ptr(self.verts), self.cap_v, _ptr(self.faces),
                                                  self.cap_f, C.byref(self.run), int(self.zoff), _stream())
        else:
            rc = lib().surs_mc_lewiner_range(_ptr(self.vol), self.n0, self.n1, self.n2, self.layers, layer_end, self.level,
                                             _ptr(self.w), self.w.numel(), _ptr(self.verts), _ptr(self.normals), _ptr(self.values),
                                             self.cap_v, _ptr(self.faces), self.cap_f, C.byref(self.run), _stream())
        if rc == -6:
            self.overflow = True
            return
        check(rc)
        self.layers = layer_end
        nv, nf = self.run.n_verts, self.run.n_faces
        if nv > self.sent_v:
            check(lib().surs_transform_points(self.verts[self.sent_v:].data_ptr(), nv - self.sent_v, self.mat,
                                              self.world[self.sent_v:].data_ptr(), _stream()))
        if self.zoff is None and (nv > self.sent_v or nf > self.sent_f):
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream())
            self.side.wait_event(ready)
            with torch.cuda.stream(self.side):
                if nv > self.sent_v:
                    self.h_world[self.sent_v:nv].copy_(self.world[self.sent_v:nv], non_blocking=True)
                if nf > self.sent_f:
                    self.h_faces[self.sent_f:nf].copy_(self.faces[self.sent_f:nf], non_blocking=True)
        self.sent_v, self.sent_f = nv, nf

    def finish(self, after=None):
        """Last layers, the checks of marching_cubes_lewiner, normals; -> (verts_world, faces, normals, values) numpy."""
        with torch.cuda.stream(self.mc):
            if after is not None:
                self.mc.wait_event(after)
            return self._finish()

    def _finish(self):
        self._advance(self.n0 - 1)
        if self.overflow:
            return None
        if self.zoff is not None:   # slab mode: device results, local numbering; the caller checks the whole grid's range
            nv, nf = self.run.n_verts, self.run.n_faces
            self.ws.mc_capacity[self.key] = mesh_capacity(nv, nf)
            torch.cuda.current_stream().synchronize()
            return self.world[:nv], self.faces[:nf]
        if self.level < self.run.vmin or self.level > self.run.vmax:
            raise ValueError("Surface level must be within volume data range.")
        nv, nf = self.run.n_verts, self.run.n_faces
        if nv == 0:
            raise RuntimeError("No surface found at the given iso value.")
        self.ws.mc_capacity[self.key] = mesh_capacity(nv, nf)
        extra = [None, None]
        if self.want:
            check(lib().surs_mc_normalize(_ptr(self.normals), nv, _stream()))
            extra = self.ws.to_host([self.normals[:nv], self.values[:nv]])
        self.side.synchronize()
        return self.h_world[:nv].numpy(), self.h_faces[:nf].numpy(), extra[0], extra[1]


def slab_mesh_one_piece(ws, key, vol, mat, level, zoff):
    """Slab-mode extraction of a finished slab in one piece (the first reconstruction of a workspace, or after a streamed
    extraction ran out of buffer): a counting call sizes the buffers.  Returns device tensors (verts_world float64 [V,3],
    faces int32 [F,3] in the slab's local numbering), the counts and the workspace that holds the edge tables."""
    n0, n1, n2 = vol.shape
    dev = vol.device
    need = lib().surs_mc_workspace_bytes(n0, n1, n2)
    w = ws.mesh_ws.get(key)
    if w is None or w.numel() < need:
        w = ws.mesh_ws[key] = torch.empty(int(need), dtype=torch.uint8, device=dev)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])

    def run(cap_v, cap_f):
        verts = torch.empty((max(cap_v, 1), 3), dtype=torch.float32, device=dev)
        faces = torch.empty((max(cap_f, 1), 3), dtype=torch.int32, device=dev)
        counts = _lib.McCounts(0, 0, 3.4028234663852886e38, -3.4028234663852886e38)
        rc = lib().surs_mc_lewiner_range_slab(_ptr(vol), n0, n1, n2, 0, n0 - 1, float(level), _ptr(w), w.numel(), _ptr(verts), cap_v,
                                              _ptr(faces), cap_f, C.byref(counts), int(zoff), _stream())
        return rc, verts, faces, counts

    cap = ws.mc_capacity.get(key) or (0, 0)
    rc, verts, faces, counts = run(*cap)
    if rc == -6:
        rc, verts, faces, counts = run(counts.n_verts, counts.n_faces)
    check(rc)
    nv, nf = counts.n_verts, counts.n_faces
    ws.mc_capacity[key] = mesh_capacity(nv, nf)
    world = torch.empty((nv, 3), dtype=torch.float64, device=dev)
    if nv:
        check(lib().surs_transform_points(_ptr(verts), nv, m, _ptr(world), _stream()))
    return world, faces[:nf], counts, w


def transform_points(verts, mat):
    """float64 [V,3] device tensor = mat[:3,:3] @ v + mat[:3,3] (the reference's np.matmul step, on the device)."""
    out = torch.empty((verts.shape[0], 3), dtype=torch.float64, device=verts.device)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    check(lib().surs_transform_points(_ptr(verts), verts.shape[0], m, _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------ octree sweep (lib/sdf.py:55-120)

def octree_volumes(R, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws, threshold, init_resolution=64, num_samples=None,
                   evaluate=None, device=None, columns=None, stats=None, dtype="fp32"):
    """eval_grid_octree on the device: float64 volumes (sdf_hr, sdf_lr) [R,R,R] like the reference's arrays.
    Host code only walks the levels; selection, evaluation (fp32-grade kernels), scatter and the cell pass are kernels.
    Single view, axis-aligned sweep (gen_mesh's): every level runs on the sweep's COLUMN kernel (surs_octree_level_columns: the
    lattice points of a level form columns of constant image position; a column's dirty points are evaluated 64 at a time); general
    calibrations, `columns=False` and native.wide_operands() (the retry after an f16 overflow: the column kernel carries f16
    parts) take the per-point layer kernels (surs_octree_select + surs_query_grid_indexed + surs_octree_scatter).
    evaluate(idx int64 device tensor [n]) -> (pred_hr, pred_lr) float32 [n] replaces the single-view evaluator
    (mesh_util passes the multi-view / perspective query there).
    stats: a list that receives (reso, dirty lattice points evaluated, lattice columns, 64-point tiles) per level (None, None on
    the per-point path).  dtype: "fp32" (the fp32-grade column kernel v11) | "bf16" | "fp16" (the 16-bit column kernel v10 on a blob
    packed for that precision - the octree sweep of `--precision bf16 | fp16`); the per-point fallbacks are fp32-grade in every case."""
    dev = device if device is not None else blob.device
    n3 = R * R * R
    sdf_hr = torch.zeros(n3, dtype=torch.float64, device=dev)
    sdf_lr = torch.zeros(n3, dtype=torch.float64, device=dev)
    dirty = torch.ones(n3, dtype=torch.uint8, device=dev)
    cnt_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = (C.c_float * 12)(*[float(v) for v in calib]) if evaluate is None else None
    reso = R // init_resolution
    batch = 262144
    use_cols = evaluate is None and columns is not False and not wide_operands_active() \
        and settings.get("SURS_OCTREE_COLUMNS") != "0" and (R + max(reso, 1) - 1) // max(reso, 1) <= 2048
    while reso > 0:
        if use_cols:
            w = ws.get(lib().surs_octree_columns_workspace_bytes(R))
            counts = (C.c_longlong * 3)(0, 0, 0)
            rc = lib().surs_octree_level_columns_dt(_ptr(sdf_hr), _ptr(sdf_lr), _ptr(dirty), R, reso, R // 2, m, cal, float(zmul),
                                                    float(zdiv), feat_lr.ptr(), feat_lr.h, feat_lr.w, feat_hr.ptr(), feat_hr.h,
                                                    feat_hr.w, _ptr(blob), DTYPES[dtype] if isinstance(dtype, str) else dtype, _ptr(w),
                                                    w.numel(), counts, _stream())
            if rc == -3 and columns is None:
                use_cols = False     # general calibration: the per-point kernels (nothing has been written yet)
                continue
            check(rc)
            if stats is not None:
                stats.append((reso, int(counts[0]), int(counts[1]), int(counts[2])))
        else:
            nl = (R + reso - 1) // reso
            cap = nl * nl * nl
            idx = torch.empty(cap, dtype=torch.int64, device=dev)
            cnt = C.c_int(0)
            check(lib().surs_octree_select(_ptr(dirty), R, reso, _ptr(idx), cap, _ptr(cnt_dev), C.byref(cnt), _stream()))
            n = cnt.value
            phr = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            plr = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            w = ws.get(lib().surs_query_workspace_bytes(min(n, batch))) if evaluate is None else None
            for b0 in range(0, n, batch):
                nb = min(batch, n - b0)
                if evaluate is not None:
                    a, b = evaluate(idx[b0:b0 + nb])
                    phr[b0:b0 + nb] = a
                    plr[b0:b0 + nb] = b
                    continue
                check(lib().surs_query_grid_indexed(C.c_void_p(idx.data_ptr() + 8 * b0), nb, R, R, m, cal, float(zmul), float(zdiv),
                                                    feat_lr.ptr(), feat_lr.h, feat_lr.w, feat_hr.ptr(), feat_hr.h, feat_hr.w,
                                                    _ptr(blob), _ptr(w), w.numel(), C.c_void_p(phr.data_ptr() + 4 * b0),
                                                    C.c_void_p(plr.data_ptr() + 4 * b0), _stream()))
            check(lib().surs_octree_scatter(_ptr(idx), n, _ptr(phr), _ptr(plr), _ptr(sdf_hr), _ptr(sdf_lr), _ptr(dirty), _stream()))
            if stats is not None:
                stats.append((reso, n, None, None))
        if reso <= 1:
            break
        w = ws.get(lib().surs_octree_workspace_bytes(R, reso))
        check(lib().surs_octree_cells(_ptr(sdf_hr), _ptr(sdf_lr), _ptr(dirty), R, reso, float(threshold), _ptr(w), w.numel(),
                                      _stream()))
        reso //= 2
    return sdf_hr.view(R, R, R), sdf_lr.view(R, R, R)


def octree_level_values(R, reso, idx, mat, calib, zmul, zdiv, feat_lr, feat_hr, blob, ws, columns=True, dtype="fp32"):
    """What the octree sweep assigns to the lattice points `idx` (flat voxel indices, int64 device tensor, all on the lattice of
    stride reso) at level `reso`: (pred_hr, pred_lr) float32.  columns=True: the column kernel of surs_octree_level_columns, run on
    a walk state in which exactly `idx` is dirty (a point's last bits there depend on which points of its column share its tile:
    ask for a level's whole dirty set to get the walk's bits); False: the per-point layer kernels.  The checker of
    tests/test_gpu_octree.py drives the oracle's restatement of lib/sdf.py:55-120 with it."""
    dev = idx.device
    n = idx.numel()
    m = (C.c_double * 12)(*[float(v) for v in np.asarray(mat, np.float64).reshape(-1)[:12]])
    cal = (C.c_float * 12)(*[float(v) for v in calib])
    if not columns:
        phr = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        plr = torch.empty_like(phr)
        batch = 262144
        w = ws.get(lib().surs_query_workspace_bytes(min(max(n, 1), batch)))
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            check(lib().surs_query_grid_indexed(C.c_void_p(idx.data_ptr() + 8 * b0), nb, R, R, m, cal, float(zmul), float(zdiv),
                                                feat_lr.ptr(), feat_lr.h, feat_lr.w, feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob),
                                                _ptr(w), w.numel(), C.c_void_p(phr.data_ptr() + 4 * b0),
                                                C.c_void_p(plr.data_ptr() + 4 * b0), _stream()))
        return phr[:n], plr[:n]
    # a scratch walk state in which exactly the asked points are dirty: the level call then evaluates their tiles and writes them
    n3 = R * R * R
    hr = torch.zeros(n3, dtype=torch.float64, device=dev)
    lr = torch.zeros(n3, dtype=torch.float64, device=dev)
    dirty = torch.zeros(n3, dtype=torch.uint8, device=dev)
    dirty[idx] = 1
    w = ws.get(lib().surs_octree_columns_workspace_bytes(R))
    check(lib().surs_octree_level_columns_dt(_ptr(hr), _ptr(lr), _ptr(dirty), R, reso, R // 2, m, cal, float(zmul), float(zdiv),
                                             feat_lr.ptr(), feat_lr.h, feat_lr.w, feat_hr.ptr(), feat_hr.h, feat_hr.w, _ptr(blob),
                                             DTYPES[dtype] if isinstance(dtype, str) else dtype, _ptr(w), w.numel(), None, _stream()))
    return hr[idx].float(), lr[idx].float()


def f64_to_f32(a):
    out = torch.empty(a.shape, dtype=torch.float32, device=a.device)
    check(lib().surs_f64_to_f32(_ptr(a), _ptr(out), a.numel(), _stream()))
    return out


# ------------------------------------------------------------------ training samples (include/surs.h "training samples")

class Mesh:
    """A triangle mesh on the device: verts [nv,3] float32, faces [nf,3] int32 and the float64 area cdf [nf] (surs_mesh_area_cdf),
    uploaded and computed once.  Indices are checked on the host here; the kernels clamp them."""

    def __init__(self, verts, faces, device=None):
        device = device or require_gpu()
        v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
        f = np.ascontiguousarray(np.asarray(faces, np.int64).reshape(-1, 3))
        if len(v) == 0 or len(f) == 0:
            raise ValueError("a mesh needs vertices and faces")
        if f.min() < 0 or f.max() >= len(v):
            raise ValueError("face index out of range: [%d, %d] with %d vertices" % (f.min(), f.max(), len(v)))
        if not np.isfinite(v).all():
            raise ValueError("mesh vertices must be finite")
        self.verts = torch.from_numpy(v).to(device)
        self.faces = torch.from_numpy(f.astype(np.int32)).to(device)
        self.nv, self.nf = len(v), len(f)
        self.cdf = mesh_area_cdf(self.verts, self.faces)


def mesh_area_cdf(verts, faces):
    """float64 [nf]: inclusive prefix sum of the face areas."""
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_contiguous() and faces.is_contiguous()
    cdf = torch.empty(faces.shape[0], dtype=torch.float64, device=verts.device)
    check(lib().surs_mesh_area_cdf(_ptr(verts), verts.shape[0], _ptr(faces), faces.shape[0], _ptr(cdf), _stream()))
    return cdf


def mesh_contains_parts(nf):
    return lib().surs_mesh_contains_parts(int(nf))


def mesh_contains(points, mesh, want_winding=False):
    """points [n, >= 3] float32 (rows may be wider than 3: the row stride is the kernel's ld) -> uint8 [n], 1 where the
    generalized winding number's magnitude exceeds 0.5; with want_winding also the winding numbers, float32 [n]."""
    assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] >= 3
    n = points.shape[0]
    assert n == 0 or points.stride(1) == 1, "points: unit stride along a row"
    ld = points.stride(0) if n > 1 else max(3, points.shape[1])
    assert ld >= 3
    inside = torch.empty(n, dtype=torch.uint8, device=points.device)
    winding = torch.empty(n, dtype=torch.float32, device=points.device) if want_winding else None
    if n:
        nbytes = lib().surs_mesh_contains_workspace_bytes(n, mesh.nf)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
        check(lib().surs_mesh_contains(_ptr(points), n, ld, _ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, _ptr(ws), nbytes,
                                       _ptr(inside), _ptr(winding), _stream()))
    return (inside, winding) if want_winding else inside


def mesh_sample_pool(mesh, n_surface, n_box, sigma, b_min, b_max, seed, want_faces=False, shuffle=True):
    """One item's pool [n_surface + n_box, 3] float32 from the counter PRNG's streams of `seed`: jittered surface samples,
    then box points, then - shuffle - reordered by the shuffle stream's keys (torch.sort, stable: ties by index).  Returns
    (points, order); order is None without the shuffle; with want_faces also the surface samples' faces (generation order)."""
    n = n_surface + n_box
    dev = mesh.verts.device
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    fidx = torch.empty(n_surface, dtype=torch.int32, device=dev) if want_faces else None
    lo, hi = (C.c_float * 3)(*[float(x) for x in b_min]), (C.c_float * 3)(*[float(x) for x in b_max])
    check(lib().surs_mesh_sample_pool(_ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, _ptr(mesh.cdf), int(seed) & (2 ** 64 - 1),
                                      n_surface, n_box, float(sigma), lo, hi, _ptr(pts), _ptr(keys), _ptr(fidx), _stream()))
    order = None
    if shuffle:
        order = torch.sort(keys, stable=True)[1]
        pts = pts[order]
    return (pts, order, fidx) if want_faces else (pts, order)


def sample_select(pool, inside_hr, inside_lr, n):
    """The reference's selection on the shuffled pool [P, 3] and its flags (uint8 [P]): samples_HR [3,n], labels_HR [1,n],
    samples_LR [3,n], labels_disp [1,n] and the selected counts (int32 [4], device: inside HR, outside HR, inside LR, outside LR).
    No host synchronisation."""
    assert pool.dtype == torch.float32 and pool.dim() == 2 and pool.shape[1] >= 3 and (pool.shape[0] == 0 or pool.stride(1) == 1)
    assert inside_hr.dtype == torch.uint8 and inside_lr.dtype == torch.uint8
    P = pool.shape[0]
    assert inside_hr.numel() == P and inside_lr.numel() == P and inside_hr.is_contiguous() and inside_lr.is_contiguous()
    dev = pool.device
    s_hr = torch.empty((3, n), dtype=torch.float32, device=dev)
    s_lr = torch.empty((3, n), dtype=torch.float32, device=dev)
    l_hr = torch.empty((1, n), dtype=torch.float32, device=dev)
    l_disp = torch.empty((1, n), dtype=torch.float32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ld = pool.stride(0) if P > 1 else max(3, pool.shape[1])
    check(lib().surs_sample_select(_ptr(pool), ld, P, _ptr(inside_hr), _ptr(inside_lr), int(n), _ptr(s_hr), _ptr(l_hr), _ptr(s_lr),
                                   _ptr(l_disp), _ptr(counts), _stream()))
    return s_hr, l_hr, s_lr, l_disp, counts


# ------------------------------------------------------------------ mesh distance (include/surs.h "mesh distance")

def mesh_distance(points, mesh, want_face=False):
    """points [n, >= 3] float32 (rows may be wider than 3: the row stride is the kernel's ld) -> float32 [n], each point's distance to
    the nearest triangle of `mesh`; with want_face also int32 [n], the lowest index among the nearest triangles.  A point with a
    non-finite coordinate gets +inf and -1."""
    assert points.dtype == torch.float32 and points.dim() == 2 and points.shape[1] >= 3
    n = points.shape[0]
    assert n == 0 or points.stride(1) == 1, "points: unit stride along a row"
    ld = points.stride(0) if n > 1 else max(3, points.shape[1])
    assert ld >= 3
    dist = torch.empty(n, dtype=torch.float32, device=points.device)
    face = torch.empty(n, dtype=torch.int32, device=points.device) if want_face else None
    if n:
        nbytes = lib().surs_mesh_distance_workspace_bytes(n, mesh.nf)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
        check(lib().surs_mesh_distance(_ptr(points), n, ld, _ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, _ptr(ws), nbytes,
                                       _ptr(dist), _ptr(face), _stream()))
    return (dist, face) if want_face else dist


def mesh_distance_host(points, verts, faces):
    """surs_mesh_distance_host on numpy arrays - points [n, >= 3], verts [nv, 3], faces [nf, 3] - on the HOST, no device needed:
    (dist float32 [n], face int32 [n]), the kernel's bits."""
    p = np.asarray(points, np.float32)
    if p.ndim != 2 or p.shape[1] < 3:
        raise ValueError("mesh_distance_host: points [n, >= 3] expected, not %s" % (p.shape,))
    p = np.ascontiguousarray(p)
    v = np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3))
    f = np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))
    dist, face = np.empty(len(p), np.float32), np.empty(len(p), np.int32)
    check(lib().surs_mesh_distance_host(p.ctypes.data, len(p), p.shape[1], v.ctypes.data, len(v), f.ctypes.data, len(f), dist.ctypes.data,
                                        face.ctypes.data))
    return dist, face


# ------------------------------------------------------------------ mesh raster (include/surs.h "mesh raster")

def _view12(view):
    """A view - [3,4] or [4,4], tensor or array - as its top three rows: float32 [3,4] on the host."""
    v = view.detach().cpu().numpy() if isinstance(view, torch.Tensor) else np.asarray(view)
    if v.shape not in ((3, 4), (4, 4)):
        raise ValueError("view: [3,4] or [4,4] expected, not %s" % (v.shape,))
    return np.ascontiguousarray(np.asarray(v, np.float64)[:3].astype(np.float32))


def _image_size(size):
    """size - an int (square) or (h, w) - as (h, w)."""
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


def normal_matrix(view):
    """The row-major 3 x 3 matrix that takes world normals into the frame of `view`: the inverse transpose of its linear part,
    scaled to a largest entry of 1 (float64 on the host, rounded to float32)."""
    a = np.asarray(_view12(view), np.float64)[:, :3]
    n = np.linalg.inv(a).T
    return np.ascontiguousarray((n / np.abs(n).max()).astype(np.float32))


def mesh_raster(mesh, view, size, want_depth=False, want_bary=False):
    """The mesh seen through `view` (see _view12) on an image of `size` (see _image_size): face int32 [h,w], the triangle each pixel
    centre sees (-1: background); with want_depth also its z' (float32 [h,w], NaN on background), with want_bary the weights of
    its second and third vertex (float32 [h,w,2]).  Device tensors, no host synchronisation."""
    h, w = _image_size(size)
    dev = mesh.verts.device
    m = _view12(view)
    face = torch.empty((h, w), dtype=torch.int32, device=dev)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev) if want_depth else None
    bary = torch.empty((h, w, 2), dtype=torch.float32, device=dev) if want_bary else None
    nbytes = lib().surs_mesh_raster_workspace_bytes(w, h, mesh.nf)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    check(lib().surs_mesh_raster(_ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, m.ctypes.data, w, h, _ptr(ws), nbytes, _ptr(face),
                                 _ptr(depth), _ptr(bary), _stream()))
    out = (face,) + ((depth,) if want_depth else ()) + ((bary,) if want_bary else ())
    return out if len(out) > 1 else face


def _host_mesh(verts, faces):
    return (np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3)),
            np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3)))


def mesh_raster_host(verts, faces, view, size):
    """surs_mesh_raster_host on numpy arrays, on the HOST, no device needed: (face int32 [h,w], depth float32 [h,w], bary float32
    [h,w,2]), the kernels' bits."""
    h, w = _image_size(size)
    v, f = _host_mesh(verts, faces)
    m = _view12(view)
    face, depth, bary = np.empty((h, w), np.int32), np.empty((h, w), np.float32), np.empty((h, w, 2), np.float32)
    check(lib().surs_mesh_raster_host(v.ctypes.data, len(v), f.ctypes.data, len(f), m.ctypes.data, w, h, face.ctypes.data,
                                      depth.ctypes.data, bary.ctypes.data))
    return face, depth, bary


def normal_map(mesh, view, size, vertex_normals=None):
    """The mesh's normal map through `view`: (float32 [h,w,3] - 0.5 n + 0.5 of the unit normal in the view frame, turned towards the
    camera, (0, 0, 0) on background -, bool [h,w], the covered pixels).  Flat normals of the faces, or - vertex_normals [nv,3], tensor
    or array in the mesh's frame - their barycentric blend.  Device tensors, no host synchronisation."""
    h, w = _image_size(size)
    dev = mesh.verts.device
    m = _view12(view)
    vn = nm = None
    if vertex_normals is not None:
        vn = vertex_normals if isinstance(vertex_normals, torch.Tensor) else torch.from_numpy(np.asarray(vertex_normals, np.float32))
        vn = vn.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(vn.shape) != (mesh.nv, 3):
            raise ValueError("vertex_normals: [%d, 3] expected, not %s" % (mesh.nv, tuple(vn.shape)))
        nm = normal_matrix(view)
        face, bary = mesh_raster(mesh, view, (h, w), want_bary=True)
    else:
        face, bary = mesh_raster(mesh, view, (h, w)), None
    out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    check(lib().surs_mesh_shade_normals(_ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, m.ctypes.data, _ptr(vn),
                                        nm.ctypes.data if nm is not None else None, _ptr(face), _ptr(bary), w, h, _ptr(out), _stream()))
    return out, face >= 0


def normal_map_host(verts, faces, view, size, vertex_normals=None):
    """normal_map on numpy arrays, on the HOST: (float32 [h,w,3], bool [h,w]), the kernels' bits."""
    h, w = _image_size(size)
    v, f = _host_mesh(verts, faces)
    m = _view12(view)
    face, _, bary = mesh_raster_host(v, f, view, (h, w))
    vn = nm = None
    if vertex_normals is not None:
        vn = np.ascontiguousarray(np.asarray(vertex_normals, np.float32))
        if vn.shape != (len(v), 3):
            raise ValueError("vertex_normals: [%d, 3] expected, not %s" % (len(v), vn.shape))
        nm = normal_matrix(view)
    out = np.empty((h, w, 3), np.float32)
    check(lib().surs_mesh_shade_normals_host(v.ctypes.data, len(v), f.ctypes.data, len(f), m.ctypes.data,
                                             vn.ctypes.data if vn is not None else None, nm.ctypes.data if nm is not None else None,
                                             face.ctypes.data, bary.ctypes.data, w, h, out.ctypes.data))
    return out, face >= 0


# ------------------------------------------------------------------ mesh PRT, mesh shading (include/surs.h)

def _np(a, dtype, shape_tail, what):
    a = np.ascontiguousarray(np.asarray(a, dtype))
    if a.ndim != len(shape_tail) + 1 or a.shape[1:] != tuple(shape_tail):
        raise ValueError("%s: [n, %s] expected, not %s" % (what, ", ".join(str(s) for s in shape_tail), a.shape))
    return a


def _dev_f32(a, dev, shape, what):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s expected, not %s" % (what, tuple(shape), tuple(t.shape)))
    return t


def mesh_prt(mesh, normals, dirs, offset, workspace=None, want_tests=False):
    """surs_mesh_prt: the mesh's per-vertex transfer vectors, float32 [nv, 9] on the device, for unit vertex normals [nv, 3] and unit
    directions [D, 3] (tensors or arrays); the rays start `offset` along the normal.  Once per subject.  want_tests: through
    surs_mesh_prt_counted, also the number of ray - triangle tests executed (an int: one read of the device)."""
    dev = mesh.verts.device
    n = _dev_f32(normals, dev, (mesh.nv, 3), "normals")
    d = dirs if isinstance(dirs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(dirs, np.float32)))
    d = d.to(device=dev, dtype=torch.float32).contiguous()
    if d.dim() != 2 or d.shape[1] != 3 or d.shape[0] < 1:
        raise ValueError("dirs: [D, 3] expected, not %s" % (tuple(d.shape),))
    D = d.shape[0]
    nbytes = lib().surs_mesh_prt_workspace_bytes(mesh.nv, D)
    ws = workspace if workspace is not None else torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    prt = torch.empty((mesh.nv, 9), dtype=torch.float32, device=dev)
    if want_tests:
        waves = torch.zeros((mesh.nv * D + 63) // 64, dtype=torch.int32, device=dev)
        check(lib().surs_mesh_prt_counted(_ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, _ptr(n), _ptr(d), D, float(offset),
                                          _ptr(prt), _ptr(ws), ws.numel() * ws.element_size(), _ptr(waves), _stream()))
        return prt, 64 * int(waves.to(torch.int64).sum())
    check(lib().surs_mesh_prt(_ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, _ptr(n), _ptr(d), D, float(offset), _ptr(prt),
                              _ptr(ws), ws.numel() * ws.element_size(), _stream()))
    return prt


def mesh_prt_host(verts, faces, normals, dirs, offset, want_visible=False):
    """surs_mesh_prt_host on numpy arrays, on the HOST: float32 [nv, 9], the kernels' bits; with want_visible also uint8 [nv, D], 1
    where the pair contributed (n . d > 0 and no triangle hit)."""
    v, f = _host_mesh(verts, faces)
    n = np.ascontiguousarray(np.asarray(normals, np.float32))
    d = _np(dirs, np.float32, (3,), "dirs")
    if n.shape != (len(v), 3):
        raise ValueError("normals: [%d, 3] expected, not %s" % (len(v), n.shape))
    prt = np.empty((len(v), 9), np.float32)
    vis = np.empty((len(v), len(d)), np.uint8) if want_visible else None
    check(lib().surs_mesh_prt_host(v.ctypes.data, len(v), f.ctypes.data, len(f), n.ctypes.data, d.ctypes.data, len(d), float(offset),
                                   prt.ctypes.data, vis.ctypes.data if want_visible else None))
    return (prt, vis) if want_visible else prt


class Texture:
    """A texture's packed pyramid (surs_texture_pyramid): `.levels` float32 - a device tensor, or a numpy array with host=True -, and
    `.w`, `.h` of level 0.  level(l) is a [h >> l, w >> l, 3] view."""

    def __init__(self, levels, w, h):
        self.levels, self.w, self.h = levels, w, h

    def level(self, l):
        off = sum(3 * (self.w >> i) * (self.h >> i) for i in range(l))
        return self.levels[off:off + 3 * (self.w >> l) * (self.h >> l)].reshape(self.h >> l, self.w >> l, 3)


def texture_pyramid(tex, host=False, device=None):
    """tex uint8 [h, w, 3] (row 0 the top of the image; array or tensor) -> Texture."""
    if isinstance(tex, torch.Tensor) and not host:
        t = tex.to(device=device or tex.device).contiguous()
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("texture: uint8 [h, w, 3] expected")
    else:
        t = np.ascontiguousarray(tex.cpu().numpy() if isinstance(tex, torch.Tensor) else np.asarray(tex))
        if t.dtype != np.uint8 or t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("texture: uint8 [h, w, 3] expected, not %s %s" % (t.dtype, t.shape))
        if not host:
            t = torch.from_numpy(t).to(device or require_gpu())
    h, w = int(t.shape[0]), int(t.shape[1])
    n = lib().surs_texture_pyramid_floats(w, h)
    if host:
        levels = np.empty(max(n, 1), np.float32)
        check(lib().surs_texture_pyramid_host(t.ctypes.data, w, h, levels.ctypes.data))
    else:
        levels = torch.empty(max(n, 1), dtype=torch.float32, device=t.device)
        check(lib().surs_texture_pyramid(_ptr(t), w, h, _ptr(levels), _stream()))
    return Texture(levels[:n], w, h)


def mesh_shade_prt(mesh, view, face, bary, light, prt=None, normals=None, normal_matrix=None, texture=None, faces_uv=None, uvs=None):
    """surs_mesh_shade_prt on the device: face int32 [h, w] and bary [h, w, 2] of mesh_raster(mesh, view, (h, w), want_bary=True) ->
    rgba float32 [h, w, 4].  light [9, 3]: in the mesh's frame with prt [nv, 9]; without, normals [nv, 3] and normal_matrix [3, 3] give
    the analytic transfer and light is in the frame the matrix turns into.  texture: a device Texture with faces_uv int32 [nf, 3] (the
    faces' own corner order) and uvs [nuv, 2]; None: albedo 1."""
    dev = mesh.verts.device
    h, w = int(face.shape[0]), int(face.shape[1])
    assert face.dtype == torch.int32 and face.is_contiguous() and bary.dtype == torch.float32 and bary.is_contiguous()
    assert tuple(bary.shape) == (h, w, 2)
    m = _view12(view)
    li = np.ascontiguousarray(np.asarray(light, np.float64).astype(np.float32))
    if li.shape != (9, 3):
        raise ValueError("light: [9, 3] expected, not %s" % (li.shape,))
    p = _dev_f32(prt, dev, (mesh.nv, 9), "prt") if prt is not None else None
    n = nm = None
    if p is None:
        if normals is None or normal_matrix is None:
            raise ValueError("without prt the vertex normals and the normal matrix are needed")
        n = _dev_f32(normals, dev, (mesh.nv, 3), "normals")
        nm = np.ascontiguousarray(np.asarray(normal_matrix, np.float64).astype(np.float32).reshape(3, 3))
    fu = uv = pyr = None
    tw = th = nuv = 0
    if texture is not None:
        fu = faces_uv if isinstance(faces_uv, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(faces_uv, np.int32)))
        fu = fu.to(device=dev, dtype=torch.int32).contiguous()
        if tuple(fu.shape) != (mesh.nf, 3):
            raise ValueError("faces_uv: [%d, 3] expected, not %s" % (mesh.nf, tuple(fu.shape)))
        uv = uvs if isinstance(uvs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(uvs, np.float32)))
        uv = uv.to(device=dev, dtype=torch.float32).contiguous()
        if uv.dim() != 2 or uv.shape[1] != 2 or uv.shape[0] < 1:
            raise ValueError("uvs: [nuv, 2] expected, not %s" % (tuple(uv.shape),))
        nuv, pyr, tw, th = uv.shape[0], texture.levels, texture.w, texture.h
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    check(lib().surs_mesh_shade_prt(_ptr(face), _ptr(bary), _ptr(mesh.verts), mesh.nv, _ptr(mesh.faces), mesh.nf, m.ctypes.data, _ptr(fu),
                                    _ptr(uv), nuv, _ptr(p), _ptr(n), nm.ctypes.data if nm is not None else None, li.ctypes.data,
                                    _ptr(pyr), tw, th, w, h, _ptr(rgba), _stream()))
    return rgba


def mesh_shade_prt_host(verts, faces, view, face, bary, light, prt=None, normals=None, normal_matrix=None, texture=None, faces_uv=None,
                        uvs=None, want_shading=False):
    """mesh_shade_prt on numpy arrays, on the HOST (texture: a host Texture): rgba float32 [h, w, 4], the kernel's bits; with
    want_shading also float32 [h, w, 3], the shading before the gamma."""
    v, f = _host_mesh(verts, faces)
    face = np.ascontiguousarray(np.asarray(face, np.int32))
    h, w = face.shape
    bary = np.ascontiguousarray(np.asarray(bary, np.float32)).reshape(h, w, 2)
    m = _view12(view)
    li = np.ascontiguousarray(np.asarray(light, np.float64).astype(np.float32))
    if li.shape != (9, 3):
        raise ValueError("light: [9, 3] expected, not %s" % (li.shape,))
    p = n = nm = fu = uv = pyr = None
    if prt is not None:
        p = np.ascontiguousarray(np.asarray(prt, np.float32))
        if p.shape != (len(v), 9):
            raise ValueError("prt: [%d, 9] expected, not %s" % (len(v), p.shape))
    else:
        if normals is None or normal_matrix is None:
            raise ValueError("without prt the vertex normals and the normal matrix are needed")
        n = np.ascontiguousarray(np.asarray(normals, np.float32))
        if n.shape != (len(v), 3):
            raise ValueError("normals: [%d, 3] expected, not %s" % (len(v), n.shape))
        nm = np.ascontiguousarray(np.asarray(normal_matrix, np.float64).astype(np.float32).reshape(3, 3))
    tw = th = nuv = 0
    if texture is not None:
        fu = np.ascontiguousarray(np.asarray(faces_uv, np.int32))
        if fu.shape != (len(f), 3):
            raise ValueError("faces_uv: [%d, 3] expected, not %s" % (len(f), fu.shape))
        uv = _np(uvs, np.float32, (2,), "uvs")
        nuv, pyr, tw, th = len(uv), np.ascontiguousarray(texture.levels), texture.w, texture.h
    rgba = np.empty((h, w, 4), np.float32)
    shading = np.empty((h, w, 3), np.float32) if want_shading else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    check(lib().surs_mesh_shade_prt_host(face.ctypes.data, bary.ctypes.data, v.ctypes.data, len(v), f.ctypes.data, len(f), m.ctypes.data,
                                         ptr(fu), ptr(uv), nuv, ptr(p), ptr(n), ptr(nm), li.ctypes.data, ptr(pyr), tw, th, w, h,
                                         rgba.ctypes.data, ptr(shading)))
    return (rgba, shading) if want_shading else rgba


def image_resolve(rgba, m, host=False):
    """surs_image_resolve: rgba float32 [h m, w m, 4] -> (rgb uint8 [h, w, 3], mask uint8 [h, w]), the mean of each pixel's m x m
    sub-samples in bytes.  A device tensor, or - host - a numpy array through the host twin."""
    m = int(m)
    H, W = int(rgba.shape[0]), int(rgba.shape[1])
    if m < 1 or H % m or W % m or tuple(rgba.shape[2:]) != (4,):
        raise ValueError("image_resolve: rgba [h m, w m, 4] expected at m = %d, not %s" % (m, tuple(rgba.shape)))
    h, w = H // m, W // m
    if host:
        a = np.ascontiguousarray(np.asarray(rgba, np.float32))
        rgb, mask = np.empty((h, w, 3), np.uint8), np.empty((h, w), np.uint8)
        check(lib().surs_image_resolve_host(a.ctypes.data, w, h, m, rgb.ctypes.data, mask.ctypes.data))
        return rgb, mask
    assert rgba.dtype == torch.float32 and rgba.is_contiguous()
    rgb = torch.empty((h, w, 3), dtype=torch.uint8, device=rgba.device)
    mask = torch.empty((h, w), dtype=torch.uint8, device=rgba.device)
    check(lib().surs_image_resolve(_ptr(rgba), w, h, m, _ptr(rgb), _ptr(mask), _stream()))
    return rgb, mask


# ------------------------------------------------------------------ training images

class ImagePlan:
    """A SursTrainImagePlan (`.plan`, the ctypes struct) with its HOST tables (`.tables`, numpy uint8): what
    surs_train_image_plan fills from one view's drawn parameters."""

    def __init__(self, plan, tables):
        self.plan, self.tables = plan, tables

    @property
    def size(self):
        """(h, w) of the HR image."""
        return self.plan.h, self.plan.w


def _jitter_args(jitter):
    order, vals = ((0, 1, 2, 3), (None,) * 4) if jitter is None else (tuple(jitter[0]), tuple(jitter[1:]))
    if len(order) != 4 or len(vals) != 4:
        raise ValueError("jitter: (order, brightness, contrast, saturation, hue) expected, a factor None where the op is off")
    factors = (C.c_double * 4)(*[0.0 if v is None else float(v) for v in vals])
    return (C.c_int * 4)(*[int(k) for k in order]), factors, sum(1 << k for k, v in enumerate(vals) if v is not None)


def train_image_plan(src_size, augment=True, pad=0, flip=False, full=None, window=None, jitter=None, blur=0.0):
    """The plan of one view (surs_train_image_plan).  src_size (h, w) of the decoded image; pad, flip; full (h, w): the size the
    padded image is resized to (default: its own); window (x0, y0, w, h): the crop (default: all of it); jitter: what
    data.jitter_params returns, (order, b, c, s, h) with None for an op that is off; blur: GaussianBlur's radius.  augment False:
    the half-size pair only (phase test)."""
    h, w = (int(v) for v in src_size)
    full_h, full_w = (h + 2 * pad, w + 2 * pad) if full is None else (int(v) for v in full)
    x0, y0, ow, oh = (0, 0, full_w, full_h) if window is None else (int(v) for v in window)
    order, factors, active = _jitter_args(jitter)
    plan = _lib.TrainImagePlan()
    args = (w, h, int(bool(augment)), int(pad), int(bool(flip)), full_w, full_h, x0, y0, ow, oh, order, factors, active, float(blur))
    check(lib().surs_train_image_plan(*args, C.byref(plan), None, 0))
    tables = np.zeros(int(plan.tables_bytes), np.uint8)
    check(lib().surs_train_image_plan(*args, C.byref(plan), tables.ctypes.data, tables.nbytes))
    return ImagePlan(plan, tables)


def _u8_host(a, shape_tail):
    a = np.ascontiguousarray(np.asarray(a, np.uint8))
    if a.ndim != 2 + len(shape_tail) or a.shape[2:] != shape_tail:
        raise ValueError("uint8 image of shape [h, w%s] expected, not %s" % ("".join(", %d" % s for s in shape_tail), a.shape))
    return a


def _u8_dev(t, shape_tail):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 2 + len(shape_tail)
            and tuple(t.shape[2:]) == shape_tail):
        raise ValueError("contiguous uint8 device tensor of shape [h, w%s] expected" % "".join(", %d" % s for s in shape_tail))
    return t


def _dev_tables(tables, device):
    return torch.from_numpy(tables).to(device)


def _check_pair(hr, lr, h, w, dtype):
    if tuple(hr.shape) != (h, w, 3) or tuple(lr.shape) != (h // 2, w // 2, 3) or hr.dtype != dtype or lr.dtype != dtype:
        raise ValueError("out: float32 (img_hr [%d,%d,3], img_lr [%d,%d,3]) expected" % (h, w, h // 2, w // 2))


def train_images(plan, rgb, mask, host=False, tables=None, workspace=None, out=None):
    """surs_train_images: (img_hr float32 [h,w,3], img_lr float32 [h/2,w/2,3]) of one view, NHWC.  rgb [H,W,3], mask [H,W] uint8:
    device tensors (tables: the plan's tables on the device, uploaded here when None; workspace: a uint8 device tensor to reuse),
    or with host=True numpy arrays through surs_train_images_host.  out: (img_hr, img_lr) to write into, contiguous, of the kind
    returned."""
    p = plan.plan
    h, w = plan.size
    src = (p.geo.src_h, p.geo.src_w) if p.augment else (h, w)
    if host:
        rgb, mask = _u8_host(rgb, (3,)), _u8_host(mask, ())
        if rgb.shape[:2] != src or mask.shape != src:
            raise ValueError("the plan is for a source of %s, not rgb %s / mask %s" % (src, rgb.shape, mask.shape))
        hr, lr = (np.empty((h, w, 3), np.float32), np.empty((h // 2, w // 2, 3), np.float32)) if out is None else out
        _check_pair(hr, lr, h, w, np.float32)
        if not (hr.flags.c_contiguous and lr.flags.c_contiguous):
            raise ValueError("out: contiguous arrays expected")
        check(lib().surs_train_images_host(C.byref(p), plan.tables.ctypes.data, rgb.ctypes.data, mask.ctypes.data, hr.ctypes.data,
                                           lr.ctypes.data))
        return hr, lr
    rgb, mask = _u8_dev(rgb, (3,)), _u8_dev(mask, ())
    if tuple(rgb.shape[:2]) != src or tuple(mask.shape) != src:
        raise ValueError("the plan is for a source of %s, not rgb %s / mask %s" % (src, tuple(rgb.shape), tuple(mask.shape)))
    dev = rgb.device
    if tables is None:
        tables = _dev_tables(plan.tables, dev)
    nbytes = lib().surs_train_images_workspace_bytes(C.byref(p))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    if out is None:
        out = (torch.empty((h, w, 3), dtype=torch.float32, device=dev), torch.empty((h // 2, w // 2, 3), dtype=torch.float32, device=dev))
    hr, lr = out
    _check_pair(hr, lr, h, w, torch.float32)
    if not (hr.is_cuda and lr.is_cuda and hr.is_contiguous() and lr.is_contiguous()):
        raise ValueError("out: contiguous device tensors expected")
    check(lib().surs_train_images(C.byref(p), _ptr(tables), _ptr(rgb), _ptr(mask), _ptr(workspace), workspace.numel(), _ptr(hr), _ptr(lr),
                                  _stream()))
    return hr, lr


def _resample_plan(src_size, size, filter, window, pad, flip):
    h, w = (int(v) for v in src_size)
    full_h, full_w = (int(v) for v in size)
    x0, y0, ow, oh = (0, 0, full_w, full_h) if window is None else (int(v) for v in window)
    r, used = _lib.ImageResample(), C.c_size_t(0)
    args = (w, h, int(pad), int(bool(flip)), full_w, full_h, int(filter), x0, y0, ow, oh)
    check(lib().surs_image_resample_plan(*args, C.byref(r), None, 0, 0, C.byref(used)))
    tables = np.zeros(used.value, np.uint8)
    check(lib().surs_image_resample_plan(*args, C.byref(r), tables.ctypes.data, tables.nbytes, 0, None))
    return r, tables


def _resample_stage(name, tail, img, size, filter, window, pad, flip, host):
    img = _u8_host(img, tail) if host else _u8_dev(img, tail)
    r, tables = _resample_plan(img.shape[:2], size, filter, window, pad, flip)
    shape = (r.out_h, r.out_w) + tail
    if host:
        out = np.empty(shape, np.uint8)
        check(getattr(lib(), name + "_host")(C.byref(r), tables.ctypes.data, img.ctypes.data, out.ctypes.data))
        return out
    out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    d_tables = _dev_tables(tables, img.device)
    check(getattr(lib(), name)(C.byref(r), _ptr(d_tables), _ptr(img), _ptr(out), _stream()))
    return out


def image_resample(img, size, filter=_lib.FILTER_BILINEAR, window=None, pad=0, flip=False, host=False):
    """Pillow's img.resize(size, filter) of an RGB image [h,w,3] uint8 (after a zero border of `pad` and a horizontal flip), of
    which only window (x0, y0, w, h) is computed - zeros where it lies outside.  size (h, w); FILTER_BILINEAR or FILTER_BICUBIC.
    A device tensor, or with host=True a numpy array through the host twin."""
    return _resample_stage("surs_image_resample", (3,), img, size, filter, window, pad, flip, host)


def image_nearest(img, size, window=None, pad=0, flip=False, host=False):
    """Pillow's img.resize(size, NEAREST) of an 8-bit mask [h,w], with the window, pad and flip of image_resample."""
    return _resample_stage("surs_image_nearest", (), img, size, _lib.FILTER_BILINEAR, window, pad, flip, host)


def image_jitter(img, jitter, host=False):
    """torchvision's ColorJitter with drawn parameters on an RGB image [h,w,3] uint8: jitter = (order, b, c, s, h), a factor None
    where the op is off (data.jitter_params)."""
    img = _u8_host(img, (3,)) if host else _u8_dev(img, (3,))
    h, w = img.shape[:2]
    plan = train_image_plan((h, w), jitter=jitter)
    if host:
        out = np.empty((h, w, 3), np.uint8)
        check(lib().surs_image_jitter_host(C.byref(plan.plan), img.ctypes.data, w, h, out.ctypes.data))
        return out
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
    nbytes = lib().surs_train_images_workspace_bytes(C.byref(plan.plan))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    check(lib().surs_image_jitter(C.byref(plan.plan), _ptr(img), w, h, _ptr(ws), nbytes, _ptr(out), _stream()))
    return out


def image_blur(img, radius, host=False):
    """Pillow's img.filter(GaussianBlur(radius)) of an RGB image [h,w,3] uint8."""
    img = _u8_host(img, (3,)) if host else _u8_dev(img, (3,))
    h, w = img.shape[:2]
    plan = train_image_plan((h, w), blur=radius)
    if host:
        out = np.empty((h, w, 3), np.uint8)
        check(lib().surs_image_blur_host(C.byref(plan.plan), img.ctypes.data, w, h, out.ctypes.data))
        return out
    out, tmp = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device), torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
    check(lib().surs_image_blur(C.byref(plan.plan), _ptr(img), w, h, _ptr(tmp), _ptr(out), _stream()))
    return out


def image_hsv_host(pixels, inverse=False):
    """RGB -> Pillow's 8-bit HSV (inverse: back) on [..., 3] uint8, on the host."""
    a = np.ascontiguousarray(np.asarray(pixels, np.uint8))
    out = np.empty_like(a)
    check(lib().surs_image_hsv_host(a.ctypes.data, a.size // 3, int(bool(inverse)), out.ctypes.data))
    return out


# TI_TILE (the side of a resample and of a blur tile) and TI_JITTER_PIXELS (pixels of one partial sum) of csrc/surs_train_image.h
IMAGE_TILE, JITTER_GROUP_PIXELS = 32, 1024
