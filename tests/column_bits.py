"""The cases of tests/test_gpu_column_bits.py and of its fixture's generator (tools/gen_golden_column_bits.py): every column kernel
on one small grid, as raw bits.  Importing needs no GPU; Context does.

Grid: 2 planes x 8 columns x rz = 296 voxels - two full 128-voxel z tiles and a ragged 40 for kernels 12 / 10 / 3, four 64-voxel
tiles and 40 for kernels 11 / 5.  The planes are the two middle ones of a 296^3 lattice over [-0.5, 0.5]^3, the 8 columns span y.
Inputs: common.state_dict(), weights.body_features(32, 128), common.CALIB.  Two weight sets: layer 0's depth column
conv0.weight[:, 320] x 1 (no tile lists more than 128 layer-0 channels: kernel 12 evaluates every tile itself) and x 60 (nearly every
tile lists more: kernel 12 hands them over to kernel 10's tile mode)."""
import numpy as np

import common

PLANES, RY, RZ = 2, 8, 296
I0 = RZ // 2 - 1
GAINS = (1, 60)
KERNELS = {"bf16": (12, 10, 3), "fp16": (12, 10, 3), "fp32": (11, 5)}
CASES = [(gain, prec, kv) for gain in GAINS for prec, kvs in KERNELS.items() for kv in kvs]
ZMUL, ZDIV = 512, 200.0
FIXTURE = "column_bits_r296.npz"


def key(gain, prec, kv):
    return "g%d_%s_k%d" % (gain, prec, kv)


def matrix():
    """index (i, j, k) -> world: voxel centres of 296 steps along x and z, of RY steps along y, over [-0.5, 0.5]."""
    m = np.zeros((3, 4))
    m[0, 0], m[1, 1], m[2, 2] = 1.0 / RZ, 1.0 / RY, 1.0 / RZ
    m[:, 3] = (-0.5 + 0.5 / RZ, -0.5 + 0.5 / RY, -0.5 + 0.5 / RZ)
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

    def mlp(self, gain):
        sd = {k: np.array(v, copy=True) for k, v in common.state_dict().items() if k.startswith("mlp_")}
        for m in ("mlp_lr.", "mlp_hr."):
            sd[m + "conv0.weight"][:, 320] *= float(gain)
        return sd

    def blob(self, gain, prec):
        if (gain, prec) not in self._blobs:
            self._blobs[gain, prec] = self.native.pack_mlp(self.mlp(gain), prec, self.dev)[0]
        return self._blobs[gain, prec]

    def listed(self, gain):
        """(mean listed layer-0 channels per 128-voxel tile of the lr classifier, upper bound for hr) on the first plane."""
        return self.native.probe_listed(I0, RY, RZ, 128, matrix(), self.cal, ZMUL, ZDIV, self.Fl, self.Fh, self.blob(gain, "bf16"), self.ws)

    def bits(self, gain, prec, kv):
        """uint32 [2 (hr, lr), PLANES, RY, RZ]: the two volumes of kernel kv as stored."""
        vh, vl = self.native.query_grid(I0, I0 + PLANES, RY, RZ, matrix(), self.cal, ZMUL, ZDIV, self.Fl, self.Fh, self.blob(gain, prec),
                                        prec, self.ws, kernel=kv)
        return np.stack([vh.cpu().numpy(), vl.cpu().numpy()]).view(np.uint32)
