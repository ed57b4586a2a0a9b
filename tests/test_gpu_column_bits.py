"""Every column kernel reproduces, bit for bit, the volumes recorded from the library BEFORE the canonicalising v_max_f32 was taken
out of their LeakyReLUs (tests/golden/column_bits_r296.npz, written by tools/gen_golden_column_bits.py under that library):
kernels 12 / 10 / 3 for bf16 and fp16, 11 / 5 for fp32, on 2 planes x 8 columns x 296 voxels (full z tiles and a ragged one), with
layer 0's depth weights x 1 (kernel 12 evaluates every tile) and x 60 (kernel 12 hands nearly every tile to kernel 10's tile mode).
tests/test_gpu_fullvolume.py holds the kernels against EACH OTHER; this holds each of them against what it computed before."""
import os

import numpy as np
import pytest

import column_bits as cb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return cb.Context()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    z = np.load(os.path.join(golden_dir, cb.FIXTURE))
    return {k: z[k] for k in z.files}


def test_the_two_weight_sets_lie_on_either_side_of_the_hand_over(ctx):
    c = ctx
    lr1, hr1 = c.listed(1)
    lr60, hr60 = c.listed(60)
    print("listed layer-0 channels per 128-voxel tile: x1 lr %.1f (hr bound %.1f), x60 lr %.1f (hr bound %.1f)" % (lr1, hr1, lr60, hr60))
    assert 0 < lr1 < 128 and 0 < hr1 < 128, (lr1, hr1)
    assert lr60 > 128 and hr60 > 128, (lr60, hr60)


@pytest.mark.parametrize("gain,prec,kv", cb.CASES, ids=str)
def test_column_kernel_reproduces_the_recorded_bits(ctx, recorded, gain, prec, kv):
    c = ctx
    want = recorded[cb.key(gain, prec, kv)]
    got = c.bits(gain, prec, kv)
    assert got.shape == want.shape == (2, cb.PLANES, cb.RY, cb.RZ) and want.dtype == np.uint32
    assert np.isfinite(got.view(np.float32)).all() and len(np.unique(got)) > 64     # a field, not a constant
    differing = int((got != want).sum())
    print("gain %d %s kernel %d: %d of %d words differ" % (gain, prec, kv, differing, got.size))
    assert differing == 0
