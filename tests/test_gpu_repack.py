"""GPU checks of the device repack primitives (include/surs.h, "device repack"; csrc/surs_repack.hip): every image byte for byte
against the host packers of csrc/surs_pack.cpp on the same values, destinations pre-filled with 0xA5; the stack joint's merge against
numpy float64 within a derived bound.

Values: seeded uniform with the corner cases of the two splits planted in every tensor - +-0, an fp32 subnormal, 6e-8 and 3e-5 (f16
subnormal hi), 1e-3 (f16 subnormal lo), 1 + 2^-11 and 1 + 3 2^-11 (f16 ties of both parities), 1 + 2^-8 (a bf16 tie), 65503.9.  No NaN
and nothing at or above 65504: the documented operand range."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_common as gc

pytestmark = pytest.mark.gpu

from repack_common import mlp_sd as _mlp_sd, values as _values


def _host_images(w):
    """(packed, x2, x3) of the three host pack helpers as uint8 arrays."""
    from surs_amd import native
    lib = native.lib()
    cout, cin, k = w.shape[:3]
    out = []
    for fn, unit in ((lib.surs_conv_pack_weights, 4), (lib.surs_conv_pack_weights_x2, 1), (lib.surs_conv_pack_weights_x3, 1)):
        n = fn(None, cout, cin, k, None) * unit
        buf = np.empty(n, np.uint8)
        fn(w.ctypes.data_as(C.c_void_p), cout, cin, k, buf.ctypes.data_as(C.c_void_p))
        out.append(buf)
    return out


def _garbage(n, dev):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)


def _entry(w, dev):
    """(table entry over garbage-filled destinations, the host images) of one convolution."""
    from surs_amd import native  # noqa: F401
    host = _host_images(w)
    wd = torch.from_numpy(w).to(dev)
    dst = [_garbage(h.size, dev) for h in host]
    return (wd, w.shape[0], w.shape[1], w.shape[2], dst[0].view(torch.float32), dst[1], dst[2]), dst, host


CONV_SHAPES = [(3, 32, 3), (32, 3, 3), (64, 64, 1), (65, 17, 3), (128, 256, 3), (16, 256, 1), (256, 16, 1), (512, 512, 3)]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "%dx%dk%d" % s)
def test_conv_repack_bytes(shape):
    import gpu_common as g
    from surs_amd import native
    cout, cin, k = shape
    w = _values((cout, cin, k, k), seed=cout * 1000 + cin * 10 + k)
    entry, dst, host = _entry(w, g.dev())
    table = native.RepackTable([entry], g.dev())
    assert table.tiles == native.lib().surs_conv_repack_tiles(cout, cin, k) > 0
    native.conv_repack(table)
    for name, d, h in zip(("packed", "x2", "x3"), dst, host):
        got = d.cpu().numpy()
        assert got.size == h.size
        bad = np.flatnonzero(got != h)
        assert bad.size == 0, "%s: %d of %d bytes differ, first at %d" % (name, bad.size, h.size, bad[0])


def test_conv_repack_table_of_five_in_one_call():
    """Five mixed items - both kernel sizes, ragged and padded shapes, one without a three-part image, one with only that - in ONE
    surs_conv_repack: every workgroup finds its item through the tile prefix."""
    import gpu_common as g
    from surs_amd import native
    shapes = [(65, 17, 3), (16, 256, 1), (3, 32, 3), (256, 80, 1), (32, 48, 3)]
    entries, checks = [], []
    for i, (cout, cin, k) in enumerate(shapes):
        entry, dst, host = _entry(_values((cout, cin, k, k), seed=70 + i), g.dev())
        entry = list(entry)
        if i == 1:
            entry[6] = None          # no x3
        if i == 4:
            entry[4] = entry[5] = None   # x3 only: the wide image packed on first use
        entries.append(tuple(entry))
        checks.append((entry, dst, host))
    table = native.RepackTable(entries, g.dev())
    assert table.n == 5 and table.tiles == sum(native.lib().surs_conv_repack_tiles(*s) for s in shapes)
    native.conv_repack(table)
    for i, (entry, dst, host) in enumerate(checks):
        for j, (d, h) in enumerate(zip(dst, host)):
            got = d.cpu().numpy()
            if entry[4 + j] is None:
                assert (got == 0xA5).all(), (i, j)     # an image the item does not name is not touched
            else:
                assert np.array_equal(got, h), (i, j)


@pytest.mark.parametrize("d", [16, 48, 256])
def test_conv1x1_merge(d):
    """W = W_bl + W_al W_l, b = b_bl + W_al b_l + b_al against numpy float64: per element |dev - ref| <= 2^-23 |ref| + 2^-45 sum |terms|.
    The first term is the fp32 rounding of the result (half an ulp is at most 2^-24 |x|, taken of a double that is not the reference's),
    the second the reordering of at most 257 double additions of exact products (256 2^-53 sum |terms|): numpy's matmul fixes no
    summation order, so the comparison is not bitwise.  Derived, not measured; the worst ratio seen is recorded in NOTES.md."""
    import gpu_common as g
    from surs_amd import native
    t = {n: _values(s, seed=d + i) for i, (n, s) in enumerate((("w_bl", (256, 256, 1, 1)), ("b_bl", (256,)), ("w_al", (256, d, 1, 1)),
                                                                 ("b_al", (256,)), ("w_l", (d, 256, 1, 1)), ("b_l", (d,))))}
    dev = {n: torch.from_numpy(v).to(g.dev()) for n, v in t.items()}
    w_out, b_out = _garbage(256 * 256 * 4, g.dev()).view(torch.float32), _garbage(256 * 4, g.dev()).view(torch.float32)
    native.conv1x1_merge(dev["w_bl"], dev["b_bl"], dev["w_al"], dev["b_al"], dev["w_l"], dev["b_l"], w_out, b_out)
    f = {n: v.astype(np.float64).reshape(v.shape[:2]) if v.ndim == 4 else v.astype(np.float64) for n, v in t.items()}
    w_ref = f["w_bl"] + f["w_al"] @ f["w_l"]
    w_mag = np.abs(f["w_bl"]) + np.abs(f["w_al"]) @ np.abs(f["w_l"])
    b_ref = f["b_bl"] + f["w_al"] @ f["b_l"] + f["b_al"]
    b_mag = np.abs(f["b_bl"]) + np.abs(f["w_al"]) @ np.abs(f["b_l"]) + np.abs(f["b_al"])
    for name, got, ref, mag in (("W", w_out.cpu().numpy().reshape(256, 256), w_ref, w_mag), ("b", b_out.cpu().numpy(), b_ref, b_mag)):
        bound = 2.0 ** -23 * np.abs(ref) + 2.0 ** -45 * mag
        ratio = np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)
        print("merge d=%d %s: worst |dev - ref| / bound = %.4f" % (d, name, float(ratio.max())))
        assert (ratio <= 1.0).all(), (name, float(ratio.max()))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mlp_repack_bytes(dtype):
    """Blob of state dict A packed on the host and uploaded; repacked on the device from the tensors of B; the whole blob equals the
    host pack of B."""
    import gpu_common as g
    from surs_amd import native
    a, b = _mlp_sd("released", 1, dtype), _mlp_sd("released", 2, dtype)
    blob, core = native.pack_mlp(a, dtype, g.dev())
    want, _ = native.pack_mlp(b, dtype, torch.device("cpu"))
    assert not torch.equal(blob.cpu(), want)
    params = native.MlpParams(b, g.dev())
    ptr = blob.data_ptr()
    native.mlp_repack(params, blob, core)
    got = blob.cpu().numpy()
    bad = np.flatnonzero(got != want.numpy())
    assert blob.data_ptr() == ptr and bad.size == 0, "%d of %d bytes differ, first at %d" % (bad.size, got.size, bad[0])


@pytest.mark.parametrize("name", ["tiny", "odd", "d48", "res0", "nores"])
def test_mlp_repack_generic_bytes(name):
    import gpu_common as g
    from surs_amd import native
    a, b = _mlp_sd(name, 3), _mlp_sd(name, 4)
    shapes = gc.shapes_of(a)
    gm = native.pack_mlp_generic(a, g.dev(), shapes)
    want, _ = native.pack_mlp_generic_host(b, shapes)
    params = native.MlpParams(b, g.dev(), shapes)
    native.mlp_repack_generic(params, gm)
    got = gm.blob.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d bytes differ, first at %d" % (name, bad.size, got.size, bad[0])
    assert not np.array_equal(want, native.pack_mlp_generic_host(a, shapes)[0])
