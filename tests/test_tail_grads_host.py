"""CPU-only checks of the stack-tail and whole-filter gradients: the binding, the size queries, the refusals that need no device, and
the fixtures (tests/golden/tail_grads_*.npz) against the project's own float64 restatement of the tail (tail_grad_common.forward +
torch autograd on the CPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_common as gc
import tail_grad_common as tg
from surs_amd import _lib, autograd, model, native, options

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["surs_tail_joint_grad", "surs_encoder_tail_tape_bytes", "surs_encoder_tail_backward_workspace_bytes", "surs_encoder_tail_train",
       "surs_encoder_tail_backward", "surs_encoder_filter_lr_tape_bytes", "surs_encoder_filter_lr_backward_workspace_bytes",
       "surs_encoder_filter_lr_train", "surs_encoder_filter_lr_backward"]
SIZES = ("tail_tape_bytes", "tail_backward_workspace_bytes", "filter_lr_tape_bytes", "filter_lr_backward_workspace_bytes")
FAKE = C.c_void_p(4096)   # a non-null pointer for calls that are refused before anything is read


def test_abi_has_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "surs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert "SursHgTailParams" in hdr and "SursHgFilterParams" in hdr
    for name in ("tail_joint_grad", "tail_train_forward", "tail_backward", "filter_lr_train_forward", "filter_lr_backward") + SIZES:
        assert callable(getattr(native, name)), name
    for name in ("stack_tail_train", "stack_tail_backward", "filter_lr_train", "filter_lr_backward"):
        assert callable(getattr(model.SuRSNet, name)), name
    assert callable(autograd.stack_tail) and callable(autograd.filter_lr)


def _host_net(stacks=2, depth=1, d=256, parts=2, batch=False):
    """A SursEncoderNet with image_filter_lr's shapes and fake pointers behind them: enough for the size queries and refusals."""
    cv = lambda cin, cout, k=3: _lib.Conv(FAKE, FAKE, None if k == 3 else FAKE, cin, cout, k, 0)
    blk = lambda: _lib.ConvBlock((_lib.Conv * 3)(cv(256, 128), cv(128, 64), cv(64, 64)),
                                 (_lib.GroupNorm * 3)(*[_lib.GroupNorm(FAKE, FAKE) for _ in range(3)]))
    n = _lib.EncoderNet()
    n.residual, n.num_stack, n.hg_depth, n.parts, n.flags = 1, stacks, depth, parts, 0
    n.n_block = (C.c_int * 3)(1, 1, 1)
    n.conv2 = blk()
    per = 3 * depth + 1
    keep = [(_lib.ConvBlock * (stacks * per))(*[blk() for _ in range(stacks * per)]),
            (_lib.ConvBlock * stacks)(*[blk() for _ in range(stacks)]),
            (_lib.Conv * stacks)(*[cv(256, 256, 1) for _ in range(stacks)]),
            (_lib.Conv * stacks)(*[cv(256, d, 1) for _ in range(stacks)]),
            (_lib.Conv * stacks)(*[cv(256, 256, 1) for _ in range(stacks)]),
            (_lib.GroupNorm * stacks)(*[_lib.GroupNorm(FAKE, FAKE) for _ in range(stacks)])]
    n.hg, n.top_m, n.conv_last, n.l, n.next, n.bn_end = keep
    if batch:
        n.flags |= _lib.ENC_EXTENDED
        n.norm, n.sr_scale = _lib.NORM_BATCH, 2
    return n, keep


def test_size_queries_depend_on_net_and_size_only():
    n, keep = _host_net()
    for what in SIZES:
        q = getattr(native, what)
        a, b = q(n, 8, 8), q(n, 16, 16)
        assert a > 0 and a % 256 == 0 and q(n, 8, 8) == a, what
        assert b > a, what
        assert a < q(n, 8, 12) < b, what                                  # monotone in either direction
    assert native.filter_lr_tape_bytes(n, 8, 8) > native.tail_tape_bytes(n, 8, 8)
    n48, keep48 = _host_net(d=48)
    assert native.tail_tape_bytes(n48, 8, 8) < native.tail_tape_bytes(n, 8, 8)
    n3, keep3 = _host_net(stacks=3)
    assert native.filter_lr_tape_bytes(n3, 8, 8) > native.filter_lr_tape_bytes(n, 8, 8)
    assert native.tail_tape_bytes(n3, 8, 8) == native.tail_tape_bytes(n, 8, 8)
    # a tail runs on any map; the filter needs multiples of 2^hg_depth
    assert native.tail_tape_bytes(n, 5, 7) > 0 and native.tail_backward_workspace_bytes(n, 5, 7) > 0
    lib = _lib.lib()
    assert lib.surs_encoder_filter_lr_tape_bytes(C.byref(n), 5, 8) == 0
    assert lib.surs_encoder_filter_lr_backward_workspace_bytes(C.byref(n), 8, 7) == 0


def test_size_queries_are_zero_where_refused():
    lib = _lib.lib()
    nb, keepb = _host_net(batch=True)
    n1, keep1 = _host_net(parts=1)
    for what in SIZES:
        for net in (nb, n1):
            assert getattr(lib, "surs_encoder_" + what)(C.byref(net), 8, 8) == 0, what
    with pytest.raises(ValueError, match="--norm group only"):
        native.tail_tape_bytes(nb, 8, 8)
    with pytest.raises(ValueError, match="--norm group only"):
        native.filter_lr_backward_workspace_bytes(nb, 8, 8)


def test_refusals_carry_the_librarys_message():
    lib = _lib.lib()
    n, keep = _host_net()
    tp = _lib.HgTailParams()
    with pytest.raises(_lib.SursError, match="both gradients are missing"):
        _lib.check(lib.surs_tail_joint_grad(None, 0, None, 0, FAKE, FAKE, FAKE, 35, 256, FAKE, 256, FAKE, 256, None))
    with pytest.raises(_lib.SursError, match="D: 1 .. 512"):
        _lib.check(lib.surs_tail_joint_grad(FAKE, 600, None, 0, FAKE, FAKE, FAKE, 35, 600, FAKE, 600, FAKE, 256, None))
    with pytest.raises(_lib.SursError, match="pitch below the channel count"):
        _lib.check(lib.surs_tail_joint_grad(FAKE, 40, None, 0, FAKE, FAKE, FAKE, 35, 48, FAKE, 48, FAKE, 256, None))
    with pytest.raises(_lib.SursError, match="multiple of 4"):
        _lib.check(lib.surs_tail_joint_grad(None, 0, FAKE, 258, FAKE, FAKE, FAKE, 35, 48, FAKE, 48, FAKE, 256, None))
    with pytest.raises(_lib.SursError, match="stack 2 of 2"):
        _lib.check(lib.surs_encoder_tail_train(C.byref(n), 2, FAKE, 256, FAKE, 256, 5, 7, FAKE, FAKE, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="every stack but the last"):
        _lib.check(lib.surs_encoder_tail_train(C.byref(n), 1, FAKE, 256, FAKE, 256, 5, 7, FAKE, FAKE, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="every stack but the last"):
        _lib.check(lib.surs_encoder_tail_train(C.byref(n), 0, FAKE, 256, None, 0, 5, 7, FAKE, None, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="tape too small"):
        _lib.check(lib.surs_encoder_tail_train(C.byref(n), 0, FAKE, 256, FAKE, 256, 5, 7, FAKE, FAKE, FAKE, 1024, None))
    with pytest.raises(_lib.SursError, match="256-byte aligned"):
        _lib.check(lib.surs_encoder_tail_train(C.byref(n), 0, FAKE, 256, FAKE, 256, 5, 7, FAKE, FAKE, C.c_void_p(4096 + 64), 1 << 30, None))
    with pytest.raises(_lib.SursError, match="both gradients are missing"):
        _lib.check(lib.surs_encoder_tail_backward(C.byref(n), 0, C.byref(tp), FAKE, 5, 7, None, None, FAKE, C.byref(tp), 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="the last stack has no next"):
        _lib.check(lib.surs_encoder_tail_backward(C.byref(n), 1, C.byref(tp), FAKE, 5, 7, FAKE, FAKE, FAKE, C.byref(tp), 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="null pointer in params"):
        _lib.check(lib.surs_encoder_tail_backward(C.byref(n), 0, C.byref(tp), FAKE, 5, 7, FAKE, None, FAKE, C.byref(tp), 0, FAKE, 1 << 30, None))
    outs = (C.c_void_p * 2)(FAKE, None)
    with pytest.raises(_lib.SursError, match="every stack's output"):
        _lib.check(lib.surs_encoder_filter_lr_train(C.byref(n), FAKE, 8, 8, 256, outs, FAKE, 1 << 30, None))
    fp = _lib.HgFilterParams()
    with pytest.raises(_lib.SursError, match="every gradient is missing"):
        _lib.check(lib.surs_encoder_filter_lr_backward(C.byref(n), C.byref(fp), FAKE, 8, 8, (C.c_void_p * 2)(None, None), FAKE, C.byref(fp), 0,
                                                       FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="not a multiple of 2\\^1"):
        _lib.check(lib.surs_encoder_filter_lr_backward(C.byref(n), C.byref(fp), FAKE, 7, 8, outs, FAKE, C.byref(fp), 0, FAKE, 1 << 30, None))


def test_norm_batch_raises_not_implemented():
    o = options.BaseOptions().parse(tg.flags("joint57") + ["--norm", "batch"])
    net = model.SuRSNet(o)
    z = torch.zeros(1, 256, 4, 4)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.stack_tail_train(0, z, z)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.stack_tail_backward(0, z)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.filter_lr_train(z)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.filter_lr_backward([z, None])


def test_argument_errors_need_no_device():
    net = model.SuRSNet(tg.opt("joint57"))
    z = torch.zeros(1, 256, 5, 7)
    with pytest.raises(RuntimeError, match="needs a preceding stack_tail_train"):
        net.stack_tail_backward(0, torch.zeros(1, 256, 5, 7), z)
    with pytest.raises(RuntimeError, match="needs a preceding filter_lr_train"):
        net.filter_lr_backward([torch.zeros(1, 256, 8, 8), None])
    with pytest.raises(RuntimeError, match="every stack but the last"):
        net.stack_tail_train(1, z, z)                       # previous given for the last stack
    with pytest.raises(RuntimeError, match="every stack but the last"):
        net.stack_tail_train(0, z)                          # ... and missing for another
    with pytest.raises(RuntimeError, match="both are None"):
        net.stack_tail_backward(0)
    with pytest.raises(RuntimeError, match="the last stack has no next"):
        net.stack_tail_backward(1, None, z)
    with pytest.raises(RuntimeError, match="all are None"):
        net.filter_lr_backward([None, None])
    with pytest.raises(ValueError, match="per stack"):
        net.filter_lr_backward([z])
    with pytest.raises(ValueError, match="stack 2 of 2"):
        net.stack_tail_train(2, z, z)
    with pytest.raises(ValueError, match="256,h,w"):
        net.filter_lr_train(torch.zeros(1, 64, 8, 8))


def test_tail_keys_follow_the_state_dict():
    for name in tg.CASES:
        o, sd = tg.opt(name), tg.state_dict(name)
        keys = native.hg_tail_keys(tg.stack(name), o.num_stack_lr)
        assert sorted(keys) == sorted(tg.param_keys(name))
        assert len(keys) == (6 if tg.is_last(name) else 10)
        assert set(keys) <= set(native.hg_param_keys(sd, o.num_stack_lr, o.hg_depth))
        assert tuple(sd[tg.P + "l%d.weight" % tg.stack(name)].shape) == (o.hg_dim, 256, 1, 1)


@pytest.mark.parametrize("name", list(tg.CASES))
def test_restatement_reproduces_the_fixture(golden_dir, name):
    gold = tg.load_fixture(golden_dir, name)
    assert float(gold["margin"]) >= tg.KINK_FACTOR
    ll = tg.inputs(name, int(gold["seed"]))
    g64, L, z64 = tg.grads_of(name, ll, torch.float64, want_sites=True)
    _, _, z32 = tg.grads_of(name, ll, torch.float32, want_sites=True)
    margin, count = tg.kink_margin(z64, z32)
    assert count == int(gold["sites"]) == int(np.prod(tg.shapes(name)[0]))
    assert margin >= tg.KINK_FACTOR, margin        # (the restatement's own float32 run, not the reference's: the same condition)
    assert abs(L - float(gold["L"])) <= 1e-12 * abs(float(gold["L"]))
    assert list(g64) == tg.param_keys(name) + [tg.INPUT_KEY] + ([] if tg.is_last(name) else [tg.PREVIOUS_KEY])
    worst = 0.0
    for key, g in g64.items():
        for qname, got in gc.quantities(key, g):
            ref = gold[qname]
            dev = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
            worst = max(worst, dev)
            assert dev <= 1e-12, (qname, dev)
            assert 0.0 <= float(gold[qname + "|e_ref"]) < 1e-4, qname
    print(name, "worst deviation of the restatement", worst, "margin", margin)


def test_fixture_files_stay_small(golden_dir):
    found = [f for f in os.listdir(golden_dir) if f.startswith("tail_grads_")]
    assert len(found) >= len(tg.CASES)
    for f in found:
        assert os.path.getsize(os.path.join(golden_dir, f)) < 1 << 20, f
