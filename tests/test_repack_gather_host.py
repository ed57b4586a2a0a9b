"""The gather form of the blob packers (csrc/surs_repack_gather.h: one destination element from its index - what the device repack
kernels run with one lane per element) against the host packers of csrc/surs_pack.cpp, on the host: surs_mlp_repack_host /
surs_mlp_repack_generic_host loop the same functions over every index.  Destination pre-filled with 0xA5; every byte behind the first
256 equals the host pack's, except the alignment gaps between sections, which the gather form does not write and the host packer
leaves zero (a repack rewrites an existing blob, where they already are)."""
import ctypes as C

import numpy as np
import pytest

import grad_common as gc
from repack_common import mlp_sd
from surs_amd import native


def _tables(sd, shapes):
    keep, out = [], []
    for m, p in enumerate(("mlp_lr.", "mlp_hr.")):
        L = len(shapes[m][0]) - 1
        ws, bs = (C.c_void_p * L)(), (C.c_void_p * L)()
        for l in range(L):
            w = np.ascontiguousarray(sd[p + "conv%d.weight" % l].reshape(shapes[m][0][l + 1], -1))
            b = np.ascontiguousarray(sd[p + "conv%d.bias" % l])
            keep += [w, b]
            ws[l], bs[l] = w.ctypes.data, b.ctypes.data
        out += [ws, bs]
    return out, keep


def _compare(got, want, max_gap_bytes):
    assert got.size == want.size
    differ = got[256:] != want[256:]
    gaps = differ & (got[256:] == 0xA5) & (want[256:] == 0)
    wrong = np.flatnonzero(differ & ~gaps)
    assert wrong.size == 0, "%d bytes differ, first at %d" % (wrong.size, wrong[0] + 256)
    # (what stays unwritten is alignment padding only: less than 256 bytes per section)
    assert 0 < int(gaps.sum()) <= max_gap_bytes, int(gaps.sum())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gather_form_equals_surs_mlp_pack(dtype):
    sd = mlp_sd("released", 5, dtype)
    want, core = native.pack_mlp(sd, dtype, "cpu")
    (wl, bl, wh, bh), keep = _tables(sd, native.DEFAULT_MLP_SHAPES)
    got = np.full(want.numel(), 0xA5, np.uint8)
    native.check(native.lib().surs_mlp_repack_host(core, wl, bl, wh, bh, got.ctypes.data_as(C.c_void_p)))
    _compare(got, want.numpy(), 70 * 255)


@pytest.mark.parametrize("name", ["tiny", "odd", "d48", "res0", "nores"])
def test_gather_form_equals_surs_mlp_pack_generic(name):
    sd = mlp_sd(name, 6)
    shapes = gc.shapes_of(sd)
    want, _ = native.pack_mlp_generic_host(sd, shapes)
    (wl, bl, wh, bh), keep = _tables(sd, shapes)
    lr, hr = (native._shape_struct(*s) for s in shapes)
    got = np.full(want.size, 0xA5, np.uint8)
    native.check(native.lib().surs_mlp_repack_generic_host(C.byref(lr), wl, bl, C.byref(hr), wh, bh, got.ctypes.data_as(C.c_void_p)))
    _compare(got, want, 64 * 255)
