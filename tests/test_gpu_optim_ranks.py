"""The data-parallel optimiser step on the device: surs_optim_step_ranks against its host twin's expected bits
(tests/optim_ranks_common.py: the table, kinds and R of tests/test_optim_ranks_host.py) on the 16-byte and the scalar path;
Optimizer.step(ranks=) at R = 1 against the plain step; surs_tensors_pack against slicing; the guard over a gathered buffer."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import optim_common as oc
import optim_ranks_common as rc

pytestmark = pytest.mark.gpu


def _dev():
    import gpu_common as g
    return g.dev()


def _up(a, off=0):
    """numpy -> device tensor at a 16-byte-aligned address (off = 1: 4 bytes beyond one)."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.zeros(a.size + 4 + off, dtype=torch.float32, device=_dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size]
    t.copy_(torch.from_numpy(a))
    return t


def _run_device(case, R, pad, off=0):
    """rc.STEPS steps of surs_optim_step_ranks over the shared table; per step ([p], [[state]]) as numpy."""
    from surs_amd import native
    offs, total = rc.offsets()
    stride = total + pad
    p0, st0 = rc.fresh(case)
    p = [_up(x, off) for x in p0]
    st = [[_up(x, off) for x in s] for s in st0]
    gbuf = torch.zeros(R * stride + 4, dtype=torch.float32, device=_dev())
    assert gbuf.data_ptr() % 16 == 0
    rows = []
    for i, (o, n) in enumerate(zip(offs, rc.SIZES)):
        s = [x[i].data_ptr() for x in st] + [None] * (3 - len(st))
        rows.append((p[i].data_ptr(), gbuf.data_ptr() + 4 * o, s[0], s[1], s[2], n))
    items = native.optim_items(rows)
    native.optim_check(items, len(rows), rc.hyper(case, 0))
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(_dev())
    out = []
    for t in range(rc.STEPS):
        gbuf[:R * stride].copy_(torch.from_numpy(rc.gathered(R, t, pad).reshape(-1)))
        native.optim_step_ranks(table, len(rows), rc.hyper(case, t), R, stride, rc.scale_of(R))
        out.append(([x.cpu().numpy() for x in p], [[x.cpu().numpy() for x in s] for s in st]))
    return out


@pytest.mark.parametrize("pad", [0, 1], ids=["vector", "scalar_stride"])
@pytest.mark.parametrize("R", rc.RANKS)
@pytest.mark.parametrize("case", list(rc.CASES))
def test_kernel_equals_the_host_twin_bit_for_bit(case, R, pad):
    """Every kind, R = 1, 2, 3, 8, on the 16-byte path (rank_stride a multiple of 4) and with a rank_stride that is not (scalar
    access): p and every state tensor carry the expected bits after each step."""
    got, want = _run_device(case, R, pad), rc.expected(case, R)
    for t in range(rc.STEPS):
        rc.assert_same(got[t], want[t], "%s R=%d pad=%d step %d" % (case, R, pad, t + 1))


@pytest.mark.parametrize("case", ["SGD", "AMSgrad"])
def test_misaligned_state_takes_the_scalar_path(case):
    """p and state 4 bytes beyond 16-byte alignment (the gathered buffer aligned): scalar access, the same bits."""
    got, want = _run_device(case, 3, 0, off=1), rc.expected(case, 3)
    rc.assert_same(got[-1], want[-1], case)


def test_r1_with_a_scale_runs_the_ranks_kernel():
    """num_ranks == 1 with scale == 1 launches the plain kernel (the R = 1 cases above); with another scale the ranks kernel runs on
    one row: g * scale, against the host twin."""
    from surs_amd import native
    offs, total = rc.offsets()
    p0, st0 = rc.fresh("ADAM")
    buf = rc.gathered(1, 0)
    g = [buf[0, o:o + n] for o, n in zip(offs, rc.SIZES)]
    native.optim_step_ranks_host(rc.rows(p0, g, st0), rc.hyper("ADAM", 0), 1, total, 0.25)
    p = [_up(x) for x in rc.fresh("ADAM")[0]]
    st = [[_up(np.zeros(n, np.float32)) for n in rc.SIZES] for _ in st0]
    gbuf = _up(buf)
    rows = [(p[i].data_ptr(), gbuf.data_ptr() + 4 * o, st[0][i].data_ptr(), st[1][i].data_ptr(), None, n)
            for i, (o, n) in enumerate(zip(offs, rc.SIZES))]
    table = torch.frombuffer(bytearray(bytes(native.optim_items(rows))), dtype=torch.uint8).to(_dev())
    native.optim_step_ranks(table, len(rows), rc.hyper("ADAM", 0), 1, total, 0.25)
    rc.assert_same(([x.cpu().numpy() for x in p], [[x.cpu().numpy() for x in s] for s in st]), (p0, st0), "R=1 scale 0.25")


def test_pack_equals_the_twin():
    """surs_tensors_pack of the shared sizes into a slab at the optimiser's offsets, aligned and 4 bytes off: the host twin's bytes."""
    from surs_amd import native
    offs, total = rc.offsets()
    src = oc.gradients(0, rc.SIZES, seed=9)
    want = np.zeros(total, np.float32)
    native.tensors_pack_host([(s, want[o:o + s.size]) for s, o in zip(src, offs)])
    for off in (0, 1):
        slab = torch.zeros(total + 4, dtype=torch.float32, device=_dev())
        d = [_up(s, off) for s in src]
        items = native.pack_items([(t.data_ptr(), slab.data_ptr() + 4 * o, t.numel()) for t, o in zip(d, offs)])
        table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(_dev())
        native.tensors_pack(table, len(d))
        assert oc.same_bits(slab[:total].cpu().numpy(), want), off
        assert not slab[total:].any()


def test_the_guard_over_a_gathered_buffer_names_the_lowest_poisoned_rank():
    """surs_tensors_nonfinite over R refs of `total` floats each: -1 on a clean buffer, else the lowest rank holding a NaN or an
    infinity - in a tensor's last element, in the n % 4 tail, in rank R - 1 alone."""
    from surs_amd import native
    _, total = rc.offsets()
    R = 4
    buf = torch.from_numpy(rc.gathered(R, 0)).to(_dev())

    def answer():
        return int(native.tensors_nonfinite_device([buf[r] for r in range(R)]).item())
    assert answer() == -1
    buf[3, total - 1] = float("nan")
    assert answer() == 3
    buf[1, 4096] = float("-inf")
    assert answer() == 1
    buf[1, 4096] = 0.0
    buf[2, 4097 + 3 + 1] = float("inf")
    assert answer() == 2


# ------------------------------------------------------------------ Optimizer.step(ranks=)
def _net():
    import forward_common as fc
    from surs_amd import model, options, weights
    opt = options.BaseOptions().parse(fc.flags("s1"))
    sd = OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in weights.synthetic_state_dict(opt, seed=0).items())
    net = model.SuRSNet(opt).to(device=_dev())
    net.load_state_dict(sd)
    net.train()
    return net


def _state_bits(o):
    sd = o.state_dict()
    return OrderedDict(((i, n), v.cpu().numpy().copy() if torch.is_tensor(v) else v) for i, s in sd["state"].items() for n, v in s.items())


@pytest.mark.parametrize("kind", ["SGD", "ADAM"])
def test_optimizer_ranks_at_r1_equals_the_plain_step(kind):
    """Two steps on two nets from the same weights: step(grads) on one; on the other the gradients packed by dist.TrainGroup into its
    slab (surs_tensors_pack at Optimizer._offset) and step(ranks=(slab [1, total], 1)).  Masters, state_dict() and step count agree
    bit for bit; a key without a gradient is untouched on both."""
    import forward_common as fc
    from surs_amd import dist as sdist, optim
    x = {k: torch.from_numpy(v).to(_dev()) for k, v in fc.inputs().items()}
    args = (x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"])
    kw = dict(labels_lr=x["labels_lr"], labels_hr=x["labels_hr"])
    a, b = _net(), _net()
    oa, ob = optim.Optimizer(a, kind, lr=1e-2, weight_decay=1e-2), optim.Optimizer(b, kind, lr=1e-2, weight_decay=1e-2)
    tg = sdist.TrainGroup(b, ob)
    assert (tg.world, tg.rank) == (1, 0)
    for step in range(2):
        ga = a.forward_backward(*args, **kw)[3]
        gb = b.forward_backward(*args, **kw)[3]
        assert list(ga) == list(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
        assert oa.step(ga, guard=True) is True
        assert tg.step(gb, guard=True) is True
        for k in oa._masters:
            assert torch.equal(oa._masters[k].view(torch.int32), ob._masters[k].view(torch.int32)), (step, k)
    assert oa._t == ob._t == 2 and oa._seen == ob._seen and 0 < len(oa._seen) < len(oa._keys)
    sa, sb = _state_bits(oa), _state_bits(ob)
    assert list(sa) == list(sb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    # a poisoned slab: nothing moves, the rank is named
    before = [m.clone() for m in ob._masters.values()]
    gb = OrderedDict((k, v.clone()) for k, v in gb.items())
    next(iter(gb.values())).reshape(-1)[0] = float("nan")
    assert tg.step(gb, guard=True) is False
    assert (ob.skipped, ob.last_skipped_rank, ob._t) == (1, 0, 2)
    assert all(torch.equal(m.view(torch.int32), w.view(torch.int32)) for m, w in zip(ob._masters.values(), before))
    assert tg.fail() is False and ob.skipped == 2 and not tg._send.any()
