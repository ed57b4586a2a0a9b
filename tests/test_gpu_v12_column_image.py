"""Column kernel 12 builds the affine layer-1 A fragments of a column ONCE, into its workgroup's image in global memory, and every
wave reads them back in every z tile (surs_grid_v12.inc).  tests/test_gpu_column_bits.py runs 16 columns: no workgroup ever meets a
second one.  Here every workgroup runs several columns in succession and rewrites its image while its own L1 still holds the previous
column's lines - a stale or torn fragment shows as a wrong word, and every word is compared with kernel 10's, which reads the
column's R vectors directly and is bit-identical by design.

Grid: 10 planes x 256 columns x rz = 168 voxels (one full 128-voxel z tile and a ragged 40): 2560 columns, at least four per
workgroup of the 2 x CU-count launch.  The planes are the ten middle ones of a 512^3 lattice over [-0.5, 0.5]^3 (the voxel size of
the headline sweep, so a z tile lists fewer layer-0 channels than the 296-lattice of the recorded fixture does), the 256 columns span
y, the 168 voxels are centred in z.  Inputs as in column_bits: common.state_dict(), weights.body_features(32, 128), common.CALIB.
Gain 1: kernel 12 evaluates the tiles itself (case A).  Gain 60: it hands them to kernel 10's tile mode - the image is built and never
read (case B)."""
import numpy as np
import pytest

import column_bits as cb

pytestmark = pytest.mark.gpu

LATTICE, PLANES, RY, RZ = 512, 10, 256, 168
I0 = LATTICE // 2 - PLANES // 2


def matrix():
    m = np.zeros((3, 4))
    m[0, 0], m[1, 1], m[2, 2] = 1.0 / LATTICE, 1.0 / RY, 1.0 / LATTICE
    m[:, 3] = (-0.5 + 0.5 / LATTICE, -0.5 + 0.5 / RY, (0.5 - 0.5 * RZ) / LATTICE)
    return m.reshape(-1)


@pytest.fixture(scope="module")
def ctx():
    return cb.Context()


def listed(c, gain, plane):
    return c.native.probe_listed(plane, RY, RZ, 128, matrix(), c.cal, cb.ZMUL, cb.ZDIV, c.Fl, c.Fh, c.blob(gain, "bf16"), c.ws)


def bits(c, gain, prec, kv):
    vh, vl = c.native.query_grid(I0, I0 + PLANES, RY, RZ, matrix(), c.cal, cb.ZMUL, cb.ZDIV, c.Fl, c.Fh, c.blob(gain, prec), prec, c.ws,
                                 kernel=kv)
    return np.stack([vh.cpu().numpy(), vl.cpu().numpy()]).view(np.uint32)


def check_equal(c, gain, prec):
    got, want = bits(c, gain, prec, 12), bits(c, gain, prec, 10)
    assert got.shape == want.shape == (2, PLANES, RY, RZ)
    assert np.isfinite(want.view(np.float32)).all() and len(np.unique(want)) > 64     # a field, not a constant
    differing = int((got != want).sum())
    print("gain %d %s: %d of %d words of kernel 12 differ from kernel 10's" % (gain, prec, differing, got.size))
    assert differing == 0


def test_every_workgroup_runs_several_columns(ctx):
    import torch
    cus = torch.cuda.get_device_properties(ctx.dev).multi_processor_count
    assert PLANES * RY >= 4 * 2 * cus, (PLANES * RY, cus)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_reused_image_gives_kernel_10s_words(ctx, prec):
    for plane in (I0, I0 + PLANES - 1):
        lr, hr = listed(ctx, 1, plane)
        print("plane %d: listed layer-0 channels per 128-voxel tile: lr %.1f (hr bound %.1f)" % (plane, lr, hr))
        assert 0 < lr < 128 and 0 < hr < 128, (plane, lr, hr)     # kernel 12 evaluates the tiles itself
    check_equal(ctx, 1, prec)


def test_image_built_and_never_read_when_the_tiles_are_handed_over(ctx):
    lr, hr = listed(ctx, 60, I0)
    print("gain 60: listed layer-0 channels per 128-voxel tile: lr %.1f (hr bound %.1f)" % (lr, hr))
    assert lr > 128 and hr > 128, (lr, hr)
    check_equal(ctx, 60, "bf16")
