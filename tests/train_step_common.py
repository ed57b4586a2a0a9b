"""Cases, inputs and the fixture format of the whole-network training-step tests (tests/golden/train_step_<case>.npz,
tools/gen_golden_train_step.py), and the tables of the non-finite guard's tests.

What the fixture pins is the WIRING of forward_backward(encoder=True), through the loss itself, which is continuous at every kink of the
network (per-tensor gradients rest on the module fixtures: mlp_grads_*, feat_grads_*, sr_grads_*, hg_grads_*, tail_grads_*).  Per
case, per loss-weight variant and per parameter set (mlp, sr, hg, all) it holds the reference's error, in float64 and in float32,
before and after ONE plain SGD step (momentum 0) on that set alone, with the learning rate the generator chose:

    r   = FACTOR * max(|e32 - e64| over the two error values, 2^-20 |e64|)     the resolution: sr_grad_common's factor and floor
    lr  = the smallest of LADDER with |e64 after - e64 before| >= STEP_RATIO r  (asserted by the generator)

A step along a wrong gradient of that set - a missing path, a swapped upstream, a wrong sign or scale - moves the error somewhere
else than the reference's step does, by a multiple of r; a test holds both error values within r of the float64 ones.  Everything on
the input side comes from seeds; the weights are weights.synthetic_state_dict's, as in the sibling fixtures."""
import json
import os
from collections import OrderedDict

import numpy as np

import common
import grad_common as gc
from surs_amd import options, prng, weights

FACTOR, FLOOR = 8.0, 2.0 ** -20
STEP_RATIO = 256.0
LADDER = (0.01, 0.1, 1.0, 10.0)
SETS = ("mlp", "sr", "hg", "all")
# --mlp1 --mlp2 --srweight --dispweight
VARIANTS = OrderedDict([("w1111", (1, 1, 1, 1)), ("w1101", (1, 1, 0, 1)), ("w0010", (0, 0, 1, 0))])
_TWO = ["--num_stack_lr", "2"]
_NO_RESIDUAL_FLAGS = [f for f in common.FLAGS if f != "--residual"]
# name -> (flags, (h, w) of images_lr, B, N per point set)
CASES = OrderedDict([
    ("tiny", (common.FLAGS + _TWO + ["--hg_depth", "1"], (4, 8), 2, 300)),
    # feature_lr is half the image and is halved hg_depth times: 8 x 8 is the smallest image --hg_depth 2 admits
    ("d2", (_NO_RESIDUAL_FLAGS + _TWO + ["--hg_depth", "2", "--hg_dim", "48"] + gc._dims("lr", [113, 64, 32, 1])
            + gc._dims("hr", [114, 64, 32, 1]) + gc._res("lr", [1]) + gc._res("hr", [1]), (8, 8), 1, 300)),
])


def flags(case, variant):
    w = VARIANTS[variant]
    return CASES[case][0] + [x for k, v in zip(("--mlp1", "--mlp2", "--srweight", "--dispweight"), w) for x in (k, str(v))]


def opt(case, variant):
    return options.BaseOptions().parse(flags(case, variant))


_sd_cache = {}


def state_dict(case):
    if case not in _sd_cache:
        _sd_cache[case] = weights.synthetic_state_dict(opt(case, "w1111"), seed=0)
    return _sd_cache[case]


def inputs(case):
    """forward()'s arguments as numpy arrays: other points and other labels for the two point sets."""
    _, (h, w), B, N = CASES[case]
    tag = "train_step_" + case
    return dict(
        images_lr=prng.uniform(tag + "_lr", 1, (B, 3, h, w), -1.0, 1.0).astype(np.float32),
        images_hr=prng.uniform(tag + "_hr", 7, (B, 3, 2 * h, 2 * w), -1.0, 1.0).astype(np.float32),
        points_hr=np.stack([weights.synthetic_points(N, seed=30 + b, lo=-0.55, hi=0.55) for b in range(B)]),
        points_lr=np.stack([weights.synthetic_points(N, seed=40 + b, lo=-0.55, hi=0.55) for b in range(B)]),
        calibs=np.stack([common.CALIB] * B),
        labels_hr=(prng.uniform(tag + "_lab_hr", 1, (B, 1, N), 0.0, 1.0) > 0.5).astype(np.float32),
        labels_lr=(prng.uniform(tag + "_lab_lr", 1, (B, 1, N), 0.0, 1.0) > 0.5).astype(np.float32),
    )


def set_keys(case, which):
    """The state-dict keys of a parameter set, in state_dict() order: what mlp_parameters(), sr_parameters(), hg_parameters() hold."""
    from surs_amd import native
    sd, o = state_dict(case), opt(case, "w1111")
    keys = dict(mlp=[k for k in sd if k.startswith("mlp_")], sr=native.sr_param_keys(sd, o.n_block),
                hg=native.hg_param_keys(sd, o.num_stack_lr, o.hg_depth))
    if which == "all":
        want = set(keys["mlp"]) | set(keys["sr"]) | set(keys["hg"])
        return [k for k in sd if k in want]
    return keys[which]


def fixture_path(golden_dir, case):
    return os.path.join(golden_dir, "train_step_%s.npz" % case)


def load_fixture(golden_dir, case):
    """{(variant, set): dict(lr=, e64=[before, after], e32=[before, after], ratio=, live=)}."""
    f = np.load(fixture_path(golden_dir, case))
    rows = json.loads(str(f["rows"]))
    return OrderedDict(((r["variant"], r["set"]), r) for r in rows)


def resolution(row, factor=FACTOR):
    e64, e32 = np.asarray(row["e64"], np.float64), np.asarray(row["e32"], np.float64)
    return factor * max(float(np.abs(e32 - e64).max()), FLOOR * float(np.abs(e64).max()))


def live(variant, which):
    """Does the error of `variant` depend on the parameters of set `which`?  With only the image term (w0010) the classifiers and the
    hourglass have no gradient: a step on them must change nothing, bit for bit."""
    return not (variant == "w0010" and which in ("mlp", "hg"))


# ------------------------------------------------------------------ the guard's tables
GUARD_SIZES = (4097, 1, 4095, 4096, 4097)     # tensors that end before, at and beyond a chunk boundary, and a 1-element one
# name -> [(tensor, element, value)], and the expected answer
GUARD_POISON = OrderedDict([
    ("clean", ([], -1)),
    ("nan_last", ([(4, 4096, np.nan)], 4)),                      # the last element of the last tensor: a chunk of one element
    ("inf_4096", ([(0, 4096, np.inf)], 0)),                      # index 4096 of the first tensor: the first element of its chunk 1
    ("both", ([(4, 4096, np.nan), (0, 4096, np.inf)], 0)),       # the lowest index wins
    ("neg_inf_single", ([(1, 0, -np.inf)], 1)),
    ("nan_tail", ([(2, 4094, np.nan)], 2)),                      # in the n % 4 tail of a chunk
])


def guard_table(name):
    """(the arrays of one poisoned table, the index the guard must give)."""
    rng = np.random.default_rng(11)
    arrays = [rng.normal(0.0, 1.0, n).astype(np.float32) for n in GUARD_SIZES]
    arrays[3][:8] = [0.0, -0.0, 3.4028235e38, -3.4028235e38, 1e-45, -1e-45, 1.17549435e-38, 65504.0]    # finite extremes
    poison, want = GUARD_POISON[name]
    for t, e, v in poison:
        arrays[t][e] = v
    return arrays, want
