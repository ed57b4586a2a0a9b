"""The cases of tests/test_gpu_sweep_digests.py and of its fixture's generator (tools/gen_golden_sweep_digests.py): the paths of the
column sweep's host sequence that the 16-column grid of tests/column_bits.py cannot reach, each as the SHA-256 digest of the raw
bytes it returns.  Importing needs no GPU; Context does.

Inputs: common.state_dict(), weights.body_features(32, 128), common.CALIB; grids are lattices of voxel centres over [-0.5, 0.5]^3
(test_gpu_rvec_fused.matrix).  Layer 0's depth column conv0.weight[:, 320] x 1, or x 60 where kernel 12 is to hand nearly every
tile over to kernel 10.

  dense  A 36 x 32 x 168: 1152 columns, padded to 1280 - a large batch for the R vectors -, one full 128-voxel tile and a ragged one
         A128 36 x 32 x 128: whole 64-voxel tiles, so kernel 11 runs its lr pass, then its hr pass on vol_lr
         B 129 x 256 x 128: 33 024 columns = one full batch and a second one of 256 columns in the same workspace
  octree one level on the column path: R = 64, stride 2, a seeded tenth of the 32^3 lattice points dirty
  runs   3200 points as 32 runs of 100 (x, y bit-equal within a run, z ascending), the same array twice: the second call enqueues
         its batch from the first call's counts
  probe  native.probe_listed on the first plane of grid A, tile 128: two floats, compared bit for bit"""
import hashlib

import numpy as np

import common
from test_gpu_rvec_fused import matrix

ZMUL, ZDIV = 512, 200.0
FIXTURE = "sweep_digests.json"
GRIDS = {"A": (36, 32, 168), "A128": (36, 32, 128), "B": (129, 256, 128)}
# (name, grid, depth gain, precision, column kernel)
DENSE = [("A_bf16_k12", "A", 1, "bf16", 12),          # fused R kernel, kernel 12's overlay on the g image, empty hand-over
         ("A_g60_bf16_k12", "A", 60, "bf16", 12),     # nearly every tile handed over to kernel 10
         ("A_fp16_k12", "A", 1, "fp16", 12),          # R on the tiled GEMM in two parts
         ("A_fp16_k10", "A", 1, "fp16", 10),
         ("A_fp32_k11", "A", 1, "fp32", 11),          # 168 is no multiple of 64: one pass
         ("A_bf16_k3", "A", 1, "bf16", 3),
         ("A_fp32_k5", "A", 1, "fp32", 5),
         ("A128_fp32_k11", "A128", 1, "fp32", 11),    # two passes
         ("B_bf16_k12", "B", 1, "bf16", 12)]          # the batch loop
OCTREE_R, OCTREE_RESO = 64, 2
OCTREE = [("octree_fp32", "fp32"), ("octree_bf16", "bf16")]
RUNS, RUN_LEN = 32, 100
POINT_RUNS = [("runs_fp32", "fp32"), ("runs_bf16", "bf16")]
PROBE = [("probe_g1", 1), ("probe_g60", 60)]
DIGEST_CASES = [c[0] for c in DENSE] + [c[0] for c in OCTREE] + [n + s for n, _ in POINT_RUNS for s in ("_call1", "_call2")]
MIN_DISTINCT = 64


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()


def is_a_field(words):
    """finite everywhere and not (nearly) constant: what a recorded or compared output must be."""
    return bool(np.isfinite(words.view(np.float32)).all()) and len(np.unique(words)) >= MIN_DISTINCT


def dirty_points():
    """flat voxel indices (ascending) of a seeded tenth of the lattice of stride OCTREE_RESO in the OCTREE_R^3 grid."""
    nl = OCTREE_R // OCTREE_RESO
    pick = np.sort(np.random.RandomState(64).choice(nl ** 3, nl ** 3 // 10, replace=False)).astype(np.int64)
    i, j, k = pick // (nl * nl), (pick // nl) % nl, pick % nl
    return ((i * OCTREE_R + j) * OCTREE_R) * OCTREE_RESO + k * OCTREE_RESO


def run_points():
    """float32 [3, RUNS * RUN_LEN]: run r sits at one (x, y) of a seeded set, its z ascends over [-0.45, 0.45]."""
    rng = np.random.RandomState(3200)
    xy = rng.uniform(-0.4, 0.4, size=(RUNS, 2)).astype(np.float32)
    z = np.linspace(-0.45, 0.45, RUN_LEN).astype(np.float32)
    p = np.empty((3, RUNS, RUN_LEN), np.float32)
    p[0], p[1], p[2] = xy[:, 0:1], xy[:, 1:2], z[None]
    return p.reshape(3, -1)


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

    def _words(self, hr, lr):
        return np.stack([hr.cpu().numpy(), lr.cpu().numpy()]).view(np.uint32)

    def dense(self, grid, gain, prec, kv):
        """uint32 [2 (hr, lr), planes, ry, rz]: the two volumes as stored."""
        planes, ry, rz = GRIDS[grid]
        return self._words(*self.native.query_grid(0, planes, ry, rz, matrix(planes, ry, rz), self.cal, ZMUL, ZDIV, self.Fl, self.Fh,
                                                   self.blob(gain, prec), prec, self.ws, kernel=kv))

    def octree(self, prec):
        """uint32 [2, points]: the level's values at the dirty points."""
        import torch
        R = OCTREE_R
        idx = torch.from_numpy(dirty_points()).to(self.dev)
        return self._words(*self.native.octree_level_values(R, OCTREE_RESO, idx, matrix(R, R, R), self.cal, ZMUL, ZDIV, self.Fl, self.Fh,
                                                            self.blob(1, prec), self.ws, columns=True, dtype=prec))

    def point_runs(self, prec):
        """[uint32 [2, points]] of two calls on the same array; None in place of a call the library answered with 0 columns."""
        import torch
        p = torch.from_numpy(run_points()).to(self.dev)
        out = []
        for _ in range(2):
            got = self.native.query_points_columns(p, self.cal, ZMUL, ZDIV, self.Fl, self.Fh, self.blob(1, prec), prec, self.ws)
            out.append(None if got is None else self._words(*got))
        return out

    def probe(self, gain):
        """uint32 [2]: the bits of (listed lr, hr bound) on the first plane of grid A."""
        planes, ry, rz = GRIDS["A"]
        lr, hr = self.native.probe_listed(0, ry, rz, 128, matrix(planes, ry, rz), self.cal, ZMUL, ZDIV, self.Fl, self.Fh,
                                          self.blob(gain, "bf16"), self.ws)
        return np.array([lr, hr], np.float32).view(np.uint32)

    def outputs(self):
        """yields (case name, uint32 words or None) for every digest case, in DIGEST_CASES' order."""
        for name, grid, gain, prec, kv in DENSE:
            yield name, self.dense(grid, gain, prec, kv)
        for name, prec in OCTREE:
            yield name, self.octree(prec)
        for name, prec in POINT_RUNS:
            first, second = self.point_runs(prec)
            yield name + "_call1", first
            yield name + "_call2", second
