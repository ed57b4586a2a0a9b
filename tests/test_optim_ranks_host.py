"""The data-parallel optimiser step without a device: surs_optim_step_ranks_host - ou_rank_sum of csrc/surs_optim_update.h, the loop
the kernel runs, on host pointers - against surs_optim_step_host fed the rank-ordered fp32 mean numpy forms
(tests/optim_ranks_common.py), bit for bit; surs_tensors_pack's host twin and check; dist.shard_indices."""
import ctypes as C

import numpy as np
import pytest

import optim_common as oc
import optim_ranks_common as rc

CASE_R = [(c, R, pad) for c in rc.CASES for R in rc.RANKS for pad in (0, 1)]


def _run_ranks_host(case, R, pad):
    from surs_amd import native
    off, total = rc.offsets()
    p, st = rc.fresh(case)
    out = []
    for t in range(rc.STEPS):
        buf = rc.gathered(R, t, pad)
        g = [buf[0, o:o + n] for o, n in zip(off, rc.SIZES)]       # views into row 0: the other rows are read through the stride
        native.optim_step_ranks_host(rc.rows(p, g, st), rc.hyper(case, t), R, total + pad, rc.scale_of(R))
        out.append(([x.copy() for x in p], [[x.copy() for x in s] for s in st]))
    return out


@pytest.mark.parametrize("case,R,pad", CASE_R)
def test_ranks_host_equals_the_plain_step_on_the_rank_ordered_mean(case, R, pad):
    """R = 1 (scale 1): surs_optim_step_host's bits on the slab itself.  R > 1: its bits on ((g_0 + g_1) + ...) * fp32(1 / R) formed by
    numpy in fp32, left to right.  pad = 1: a rank_stride that is no multiple of 4."""
    got, want = _run_ranks_host(case, R, pad), rc.expected(case, R)
    for t in range(rc.STEPS):
        rc.assert_same(got[t], want[t], "%s R=%d pad=%d step %d" % (case, R, pad, t + 1))
    assert all(not np.array_equal(a, b) for a, b in zip(got[-1][0], oc.initial(rc.SIZES)) if a.size)


def test_the_sum_starts_from_rank_0_and_is_ordered():
    """-0 + -0 stays -0 only if the sum starts from g_0, not from +0; and (a + b) + c with a = 1, b = 2^-24, c = 2^-24 differs from
    a + (b + c): the order is rank order."""
    from surs_amd import native
    h = native.optim_hyper("SGD", 1, 1.0, 0.0, 0.0)
    buf = np.zeros((3, 4), np.float32)
    buf[:, 0] = -0.0
    buf[:, 1] = [1.0, 2.0 ** -24, 2.0 ** -24]
    buf[:, 2] = [2.0 ** -24, 2.0 ** -24, 1.0]
    p = np.full(4, -0.0, np.float32)                     # plain SGD, lr 1: p = fma(-1, g, -0) = -g + -0, which is +0 for g = -0 only
    native.optim_step_ranks_host([(p, buf[0], None, None, None)], h, 3, 4, 1.0)
    acc = buf[0].copy()
    for r in (1, 2):
        acc = acc + buf[r]
    assert np.signbit(acc[0]) and acc[1] == np.float32(1.0) and acc[2] == np.float32(1.0 + 2.0 ** -23)     # what the order decides
    assert oc.same_bits(p, -acc + np.float32(-0.0)) and not np.signbit(p[0]) and np.signbit(p[3])


def test_a_nan_of_rank_2_reaches_the_parameter():
    """Non-finite gradients of any rank propagate, as in torch: the guard is a separate pass."""
    from surs_amd import native
    off, total = rc.offsets()
    for case in ("SGD", "ADAM"):
        p, st = rc.fresh(case)
        buf = rc.gathered(3, 0)
        buf[2, off[2] + 4094] = np.nan
        g = [buf[0, o:o + n] for o, n in zip(off, rc.SIZES)]
        native.optim_step_ranks_host(rc.rows(p, g, st), rc.hyper(case, 0), 3, total, rc.scale_of(3))
        assert np.isnan(p[2][4094]) and np.isfinite(np.delete(p[2], 4094)).all()
        assert all(np.isfinite(x).all() for i, x in enumerate(p) if i != 2)


def test_ranks_host_refuses_before_it_writes():
    from surs_amd import native
    off, total = rc.offsets()
    p, st = rc.fresh("ADAM")
    before = [x.copy() for x in p]
    buf = rc.gathered(2, 0)
    g = [buf[0, o:o + n] for o, n in zip(off, rc.SIZES)]
    for R, stride, scale in ((0, total, 1.0), (65, total, 1.0), (2, -4, 0.5), (2, total, float("nan"))):
        with pytest.raises(native._lib.SursError):
            native.optim_step_ranks_host(rc.rows(p, g, st), rc.hyper("ADAM", 0), R, stride, scale)
    h = rc.hyper("ADAM", 0)
    h.kind = 9
    with pytest.raises(native._lib.SursError):
        native.optim_step_ranks_host(rc.rows(p, g, st), h, 2, total, 0.5)
    assert all(oc.same_bits(a, b) for a, b in zip(p, before))
    # the kernel entry checks its arguments before any launch: no device is touched by a refusal
    for R, stride, scale in ((0, total, 1.0), (65, total, 1.0), (2, -4, 0.5), (2, total, float("nan"))):
        assert native.lib().surs_optim_step_ranks(None, 0, C.byref(rc.hyper("ADAM", 0)), R, stride, scale, None) != 0


def test_pack_host_equals_slicing():
    from surs_amd import native
    off, total = rc.offsets()
    src = oc.gradients(0, rc.SIZES, seed=9)
    slab = np.zeros(total, np.float32)
    native.tensors_pack_host([(s, slab[o:o + s.size]) for s, o in zip(src, off)])
    want = np.zeros(total, np.float32)
    for s, o in zip(src, off):
        want[o:o + s.size] = s
    assert oc.same_bits(slab, want)


def test_pack_check_refuses_bad_tables_before_anything_is_written():
    from surs_amd import native
    src, dst = np.ones(5000, np.float32), np.zeros(5000, np.float32)
    with pytest.raises(native._lib.SursError):
        native.pack_items([(src.ctypes.data, None, 5000)])
    with pytest.raises(native._lib.SursError):
        native.pack_items([(None, dst.ctypes.data, 5000)])
    with pytest.raises(native._lib.SursError):
        native.pack_items([(src.ctypes.data, dst.ctypes.data, -1)])
    items = native.pack_items([(src.ctypes.data, dst.ctypes.data, 5000), (src.ctypes.data, dst.ctypes.data, 0)])
    assert [it.chunk_end for it in items] == [2, 2]
    items[0].chunk_end = 1                                           # no prefix sum
    assert native.lib().surs_tensors_pack_check(C.cast(items, C.c_void_p), 2) != 0
    assert native.lib().surs_tensors_pack_host(C.cast(items, C.c_void_p), 2) != 0
    assert native.lib().surs_tensors_pack_check(None, 1) != 0 and native.lib().surs_tensors_pack(None, 1, None) != 0
    assert not dst.any()


@pytest.mark.parametrize("n,world", [(5, 2), (7, 3), (8, 4), (3, 4), (6, 1), (0, 2)])
def test_shard_indices(n, world):
    """Disjoint shards of n // world batches out of ONE permutation, the tail dropped; the same on every call."""
    from surs_amd.dist import shard_indices
    shards = [shard_indices(n, r, world, seed=3) for r in range(world)]
    assert all(len(s) == n // world for s in shards)
    flat = [i for s in shards for i in s]
    assert len(set(flat)) == len(flat) == n // world * world and all(0 <= i < n for i in flat)
    perm = np.random.default_rng(3).permutation(n)
    assert [i for t in zip(*shards) for i in t] == [int(i) for i in perm[:n // world * world]]     # one permutation, dealt in rounds
    assert shards == [shard_indices(n, r, world, seed=3) for r in range(world)]
    plain = [shard_indices(n, r, world, shuffle=False) for r in range(world)]
    assert plain == [list(range(r, n // world * world, world)) for r in range(world)]
    with pytest.raises(ValueError):
        shard_indices(n, world, world)


def test_the_new_flags_default_to_one_process():
    from surs_amd import options
    opt = options.BaseOptions().parse([])
    assert (opt.world_size, opt.rank, opt.dist_backend) == (1, -1, "nccl") and opt.dist_url.startswith("tcp://")
    opt = options.BaseOptions().parse(["--world_size", "4", "--rank", "3", "--dist_backend", "gloo", "--dist_url", "tcp://127.0.0.1:1"])
    assert (opt.world_size, opt.rank, opt.dist_backend, opt.dist_url) == (4, 3, "gloo", "tcp://127.0.0.1:1")
