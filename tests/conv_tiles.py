"""Shared by the GPU tests of the 3x3 convolution's tiles (import only inside @pytest.mark.gpu modules): the fixture that forces
conv_x3_tile()'s choice through the library options, and one call of the sum-in-the-epilogue entry points."""
import ctypes as C

import pytest
import torch

# conv_tall_min_wg, conv_wide_min_wg: the workgroup counts from which a stride-1 launch takes 8 rows / 8 rows x 64 channels
TILE_OPTIONS = ("conv_tall_min_wg", "conv_wide_min_wg")
TILES = {"4x32": (0, 0), "8x32": (1, 0), "8x64": (1, 1), "defaults": (256, 512)}


def tile_of(name, parts=2):
    """(rows, channels) a stride-1 launch runs under the forced tile `name`: the one-part kernel has no 64-channel form."""
    rows, chans = int(name[0]), int(name[2:])
    return (rows, 32) if parts == 1 else (rows, chans)


@pytest.fixture
def force_tile():
    """force_tile(name) sets both options (they are process-wide); both are back at their entry values when the test ends."""
    from surs_amd import native
    saved = [native.get_option(k) for k in TILE_OPTIONS]

    def force(name):
        for k, v in zip(TILE_OPTIONS, TILES[name]):
            native.set_option(k, v)
    try:
        yield force
    finally:
        for k, v in zip(TILE_OPTIONS, saved):
            native.set_option(k, v)


def hwc(t):
    """An Img's values as a [h, w, c] view of its buffer."""
    return torch.as_strided(t.buf, (t.h, t.w, t.c), (t.w * t.ld, t.ld, 1), t.buf.storage_offset() + t.off)


def fold(buf, slots, pitch=None):
    """Partial sums [32][pitch][2] with `slots` of each row filled, folded on the host: [32][2] float64."""
    pitch = slots if pitch is None else pitch
    return buf[:64 * pitch].view(32, pitch, 2)[:, :slots].sum(dim=1).cpu().numpy()


class ConvSum:
    """surs_conv2d_nhwc_gn_sum (or, with stats=False, surs_conv2d_nhwc_sum) on its own: x (with the statistics its producer left)
    through GroupNorm(gamma, beta) + ReLU and the 3x3 convolution `cw`; the value goes to `raw` (None: nowhere), value + residual to
    `out2`; the statistics of the value to sb1, those of the sum to groups [g0, g0 + cout / cg) of sb2, whose rows lie `cap` slots
    apart."""

    def __init__(self, x, cw, gamma, beta, cap, parts=2):
        from surs_amd import _lib
        self.x, self.cw, self.gamma, self.beta, self.cap, self.parts = x, cw, gamma, beta, cap, parts
        dev = x.buf.device
        self.s_in = _lib.GnStats(x.stats.buf.data_ptr(), x.stats.slots, 0, 0, (C.c_int * 3)(x.stats.slots, 0, 0))
        self.sb1 = torch.zeros(32 * cap * 2, dtype=torch.float64, device=dev)
        self.sb2 = torch.zeros(32 * cap * 2, dtype=torch.float64, device=dev)
        self.s_out = _lib.GnStats(self.sb1.data_ptr(), cap, 0, 0, (C.c_int * 3)(0, 0, 0))
        self.slots = C.c_int(0)

    def __call__(self, raw, residual, out2, g0, cg, h=None, stats=True, raw_stats=True):
        from surs_amd import native
        x, cw = self.x, self.cw
        h, cout = (x.h if h is None else h), cw.cout
        rawp, raw_ld = (raw.ptr(), raw.ld) if raw is not None else (None, 0)
        if not stats:
            sc, sh = native.groupnorm_coeffs(x, self.gamma, self.beta)
            native.check(native.lib().surs_conv2d_nhwc_sum(self.parts, x.ptr(), h, x.w, x.c, x.ld, native._ptr(cw.w3), None, native._ptr(sc),
                                                           native._ptr(sh), rawp, cout, raw_ld, residual.ptr(), residual.ld, out2.ptr(),
                                                           out2.ld, native._stream()))
            return 0
        native.check(native.lib().surs_conv2d_nhwc_gn_sum(self.parts, x.ptr(), h, x.w, x.c, x.ld, native._ptr(cw.w3), None, C.byref(self.s_in),
                                                          None, None, native._ptr(self.gamma), native._ptr(self.beta), 1e-5, rawp, cout,
                                                          raw_ld, C.byref(self.s_out) if raw_stats else None, residual.ptr(), residual.ld,
                                                          out2.ptr(), out2.ld, native._ptr(self.sb2), self.cap, g0, cg, C.byref(self.slots),
                                                          native._stream()))
        return self.slots.value
