"""The bf16 sweep's R vectors of batches of more than 1024 columns come from ONE kernel that forms the g-scaled operand itself
(rvec_fused_kernel, csrc/surs_gemm.inc) instead of colsum_prepare_kernel's image and two launches of the tiled GEMM.  Same products,
same order, same instruction: every case runs the sweep with the library option r_fused = 1 and = 0 and compares both volumes word
for word - 0 words may differ, no tolerance.

Grids (planes x rows x voxels, a lattice of voxel centres over [-0.5, 0.5]^3; seeded synthetic weights and features as
tests/column_bits.py uses):
  A  36 x 32 x 168: 1152 columns, padded to 1280 = 20 point tiles of 64 columns, the last one half padding; 168 voxels = one full
     128-voxel z tile and a ragged one;
  B  129 x 256 x 128: 33 024 columns = one full batch of 32 768 on the fused kernel (1024 workgroups: four rounds of the device),
     then 256 columns on rvec_small_kernel;
  C  grid A with layer 0's depth column x 60 (bench.py's listed_sensitivity): most channels are on the 0.01 branch at mid column and
     kernel 12 hands nearly every tile to kernel 10's tile mode.
Each with column kernel 12 and 10.  The fp16 and fp32 sweeps never take the fused kernel: their volumes must not depend on the
switch at all."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 512, 200.0
GRIDS = {"A": (36, 32, 168, 1), "B": (129, 256, 128, 1), "C": (36, 32, 168, 60)}


def matrix(planes, ry, rz):
    m = np.zeros((3, 4))
    m[0, 0], m[1, 1], m[2, 2] = 1.0 / planes, 1.0 / ry, 1.0 / rz
    m[:, 3] = (-0.5 + 0.5 / planes, -0.5 + 0.5 / ry, -0.5 + 0.5 / rz)
    return m.reshape(-1)


class Context:
    def __init__(self):
        import gpu_common as g
        from surs_amd import native, weights
        self.native, self.dev = native, g.dev()
        fl, fh = weights.body_features(32, 128)
        self.Fl, self.Fh = g.upload_nhwc(fl), g.upload_nhwc(fh)
        self.ws = native.Workspace(self.dev)
        self.cal = common.CALIB.reshape(-1)[:12]
        self._blobs = {}

    def blob(self, gain, prec):
        if (gain, prec) not in self._blobs:
            sd = {k: np.array(v, copy=True) for k, v in common.state_dict().items() if k.startswith("mlp_")}
            for m in ("mlp_lr.", "mlp_hr."):
                sd[m + "conv0.weight"][:, 320] *= float(gain)
            self._blobs[gain, prec] = self.native.pack_mlp(sd, prec, self.dev)[0]
        return self._blobs[gain, prec]

    def bits(self, grid, prec, kv, fused):
        """uint32 [2 (hr, lr), planes, ry, rz]: the two volumes as stored, with r_fused = fused."""
        planes, ry, rz, gain = GRIDS[grid]
        nat = self.native
        old = nat.get_option("r_fused")
        nat.set_option("r_fused", fused)
        try:
            vh, vl = nat.query_grid(0, planes, ry, rz, matrix(planes, ry, rz), self.cal, ZMUL, ZDIV, self.Fl, self.Fh,
                                    self.blob(gain, prec), prec, self.ws, kernel=kv)
            return np.stack([vh.cpu().numpy(), vl.cpu().numpy()]).view(np.uint32)
        finally:
            nat.set_option("r_fused", old)


@pytest.fixture(scope="module")
def ctx():
    return Context()


def _compare(c, grid, prec, kv):
    planes, ry, rz, _ = GRIDS[grid]
    got = c.bits(grid, prec, kv, 1)
    want = c.bits(grid, prec, kv, 0)
    assert got.shape == want.shape == (2, planes, ry, rz)
    assert np.isfinite(want.view(np.float32)).all() and len(np.unique(want)) > 64     # a field, not a constant
    differing = int((got != want).sum())
    print("grid %s %s kernel %d: %d of %d words differ" % (grid, prec, kv, differing, got.size))
    assert differing == 0


def test_the_switch_is_on_by_default(ctx):
    assert ctx.native.get_option("r_fused") == 1 and ctx.native.get_option("SURS_R_FUSED") == 1


@pytest.mark.parametrize("kv", [12, 10])
@pytest.mark.parametrize("grid", ["A", "B", "C"])
def test_fused_r_kernel_gives_the_bits_of_the_image_and_two_gemms(ctx, grid, kv):
    _compare(ctx, grid, "bf16", kv)


def test_fp16_and_fp32_sweeps_do_not_depend_on_the_switch(ctx):
    _compare(ctx, "A", "fp16", 0)
    _compare(ctx, "A", "fp32", 0)
