"""The seeded points and probabilities behind tests/golden/samples_prob.ply (tools/gen_golden_train_step.py)."""
import numpy as np

from surs_amd import prng

N = 257


def samples():
    """(points [N,3] float32, prob [N,1] float32): values on both sides of 0.5, exactly 0.5, 0 and 1, and coordinates that round in the
    sixth decimal, are negative, or print as -0.000000."""
    pts = prng.uniform("samples_ply_points", 3, (N, 3), -1.0, 1.0).astype(np.float32)
    prob = prng.uniform("samples_ply_prob", 5, (N, 1), 0.0, 1.0).astype(np.float32)
    prob[:4, 0] = [0.5, 0.0, 1.0, 0.50000006]
    pts[:3] = [[0.0000005, -0.0000005, -1e-9], [123.4567895, -0.5, 1e-7], [0.0, -0.0, 1.0]]
    return pts, prob
