"""Values of the device-repack tests (tests/test_gpu_repack.py, tests/test_repack_gather_host.py): seeded uniform with the corner cases
of the two operand splits planted in every tensor."""
import numpy as np

import grad_common as gc

PLANTED = np.array([0.0, -0.0, 1e-40, 6e-8, 3e-5, 1e-3, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 65503.9], np.float32)


def values(shape, seed):
    """Seeded uniform [-1, 1) with PLANTED (and its negatives where the tensor has room) at seeded places."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    flat = v.reshape(-1)
    plant = np.concatenate([PLANTED, -PLANTED]) if flat.size >= 4 * PLANTED.size else PLANTED[:flat.size]
    flat[rng.permutation(flat.size)[:plant.size]] = plant
    return v


def mlp_sd(name, seed, dtype=None):
    """The classifier entries of a case's state dict (tests/grad_common.py) with seeded values of their own, weights [out,in,1] as the
    state dict has them.  dtype "fp16" (the released blob in f16): its b1frag section holds f16(4096 b) of the layer-1 bias, so that
    tensor's operand range ends at 65504 / 4096 and its planted largest value is 65503.9 / 4096 - beyond it both packers form
    inf - inf, whose NaN sign differs between host and device.  Every other case keeps the full range."""
    sd = gc.mlp_state(name)
    out = {k: values(v.shape, seed=seed * 1000 + i) for i, (k, v) in enumerate(sd.items())}
    if name == "released" and dtype == "fp16":
        for k in ("mlp_lr.conv1.bias", "mlp_hr.conv1.bias"):
            big = np.abs(out[k]) > 16.0
            out[k][big] = out[k][big] / np.float32(4096.0)
    return out
