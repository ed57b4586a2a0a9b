"""Shared by tests/test_optim_ranks_host.py and tests/test_gpu_optim_ranks.py: the seeded tables of the data-parallel optimiser step
(surs_optim_step_ranks) and of surs_tensors_pack, and the numpy model of the rank-ordered mean.

ONE table: items of SIZES elements - tensors that end before, at and beyond a 4096-element chunk boundary, a 1-element one, an empty
one and one with an n % 4 tail - at 16-byte-aligned offsets of a gathered [R, stride] float32 buffer, as Optimizer._offset places
them.  stride is the slab's length (a multiple of 4: the kernel's 16-byte path) or one more (no multiple of 4: its scalar path).
The expected values are surs_optim_step_host's on the gradient numpy forms in fp32, left to right from rank 0, times
np.float32(1 / R): the sum's order and the one product are what is pinned; the update itself is tests/optim_common.py's subject."""
import numpy as np

import optim_common as oc

SIZES = (4097, 1, 4095, 4096, 0, 7)
RANKS = (1, 2, 3, 8)
STEPS = 2                                # the first step (SGD's buf = g) and one after it
CASES = oc.CASES                         # all four kinds, SGD with and without momentum
WD = 1e-2


def offsets(sizes=SIZES):
    """(offset per item, slab length): Optimizer._offset's rule."""
    off, total = [], 0
    for n in sizes:
        off.append(total)
        total += (n + 3) // 4 * 4
    return off, total


def gathered(R, step, pad=0, sizes=SIZES, seed=5):
    """A [R, total + pad] float32 buffer: row r the slab of rank r (seeded normals with a few signed zeros and tiny values, zeros in
    the padding between items)."""
    off, total = offsets(sizes)
    buf = np.zeros((R, total + pad), np.float32)
    for r in range(R):
        for o, g in zip(off, oc.gradients(step, sizes, seed=seed + 17 * r)):
            buf[r, o:o + g.size] = g
    return buf


def rank_mean(buf, o, n):
    """((g_0 + g_1) + ... + g_{R-1}) * fp32(1 / R) of one item, every operation one fp32 rounding; R = 1: g_0 itself."""
    acc = buf[0, o:o + n].copy()
    for r in range(1, buf.shape[0]):
        acc = (acc + buf[r, o:o + n]).astype(np.float32)
    if buf.shape[0] > 1:
        acc = (acc * np.float32(1.0 / buf.shape[0])).astype(np.float32)
    return acc


def hyper(case, t):
    from surs_amd import native
    kind, momentum = CASES[case]
    return native.optim_hyper(kind, t + 1, oc.LR, WD, momentum, oc.BETAS, oc.EPS, oc.ALPHA, first_step=t == 0)


def fresh(case, sizes=SIZES):
    """(p, [state arrays per state name]) of a new run."""
    kind, momentum = CASES[case]
    p = oc.initial(sizes)
    return p, [[np.zeros_like(x) for x in p] for _ in oc.state_names(kind, momentum)]


def rows(p, g, st):
    return [(p[i], g[i]) + tuple(s[i] for s in st) + (None,) * (3 - len(st)) for i in range(len(p))]


_expected = {}


def expected(case, R):
    """Per step ([p], [[state]]) of surs_optim_step_host fed rank_mean of gathered(R, step): computed once, never changed."""
    from surs_amd import native
    key = (case, R)
    if key not in _expected:
        off, _ = offsets()
        p, st = fresh(case)
        out = []
        for t in range(STEPS):
            buf = gathered(R, t)
            g = [rank_mean(buf, o, n) for o, n in zip(off, SIZES)]
            native.optim_step_host(rows(p, g, st), hyper(case, t))
            out.append(([x.copy() for x in p], [[x.copy() for x in s] for s in st]))
        _expected[key] = out
    return _expected[key]


def scale_of(R):
    return 1.0 if R == 1 else float(np.float32(1.0 / R))


def assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert oc.same_bits(a, b), (what, "p", i)
    for s, (ga, wa) in enumerate(zip(got[1], want[1])):
        for i, (a, b) in enumerate(zip(ga, wa)):
            assert oc.same_bits(a, b), (what, "state %d" % s, i)
