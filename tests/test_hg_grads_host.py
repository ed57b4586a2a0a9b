"""CPU-only checks of the hourglass gradients: the binding, the refusals that need no device, and the fixtures
(tests/golden/hg_grads_*.npz) against the project's own float64 restatement of the modules (hg_grad_common.forward + torch autograd on
the CPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_common as gc
import hg_grad_common as hg
from surs_amd import _lib, model, native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["surs_groupnorm_fold", "surs_groupnorm_relu_grad_workspace_bytes", "surs_groupnorm_relu_grad", "surs_avgpool2_grad",
       "surs_bicubic_up2_grad", "surs_encoder_convblock_tape_bytes", "surs_encoder_convblock_backward_workspace_bytes",
       "surs_encoder_hourglass_tape_bytes", "surs_encoder_hourglass_backward_workspace_bytes", "surs_encoder_convblock_train",
       "surs_encoder_convblock_backward", "surs_encoder_hourglass_train", "surs_encoder_hourglass_backward"]
FAKE = C.c_void_p(4096)   # a non-null pointer for calls that are refused before anything is read


def test_abi_has_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "surs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert "SursHgBlockParams" in hdr


def _host_net(depth=2, parts=2, batch=False):
    """A SursEncoderNet with image_filter_lr's block shapes and fake pointers behind them: enough for the size queries and refusals."""
    cv = lambda cin, cout: _lib.Conv(FAKE, FAKE, None, cin, cout, 3, 0)
    blk = lambda: _lib.ConvBlock((_lib.Conv * 3)(cv(256, 128), cv(128, 64), cv(64, 64)),
                                 (_lib.GroupNorm * 3)(*[_lib.GroupNorm(FAKE, FAKE) for _ in range(3)]))
    n = _lib.EncoderNet()
    n.residual, n.num_stack, n.hg_depth, n.parts, n.flags = 1, 1, depth, parts, 0
    n.n_block = (C.c_int * 3)(1, 1, 1)
    n.conv2 = blk()
    arr = (_lib.ConvBlock * (3 * depth + 1))(*[blk() for _ in range(3 * depth + 1)])
    n.hg = arr
    if batch:
        n.flags |= _lib.ENC_EXTENDED
        n.norm, n.sr_scale = _lib.NORM_BATCH, 2
    return n, arr


def test_size_queries_depend_on_net_and_size_only():
    n, keep = _host_net()
    for hourglass in (False, True):
        a, b = native.hg_tape_bytes(n, 8, 12, hourglass), native.hg_backward_workspace_bytes(n, 8, 12, hourglass)
        assert a > 0 and b > 0 and a % 256 == 0
        assert native.hg_tape_bytes(n, 8, 12, hourglass) == a and native.hg_backward_workspace_bytes(n, 8, 12, hourglass) == b
        assert native.hg_tape_bytes(n, 16, 12, hourglass) > a
    assert native.hg_tape_bytes(n, 8, 12, True) > native.hg_tape_bytes(n, 8, 12, False)
    n1, keep1 = _host_net(depth=1)
    assert native.hg_tape_bytes(n1, 8, 12, True) < native.hg_tape_bytes(n, 8, 12, True)


def test_size_queries_refuse_sizes_not_divisible_by_two_to_the_depth():
    lib = _lib.lib()
    n, keep = _host_net(depth=2)
    for h, w in ((6, 8), (8, 6), (7, 8), (0, 8)):
        assert lib.surs_encoder_hourglass_tape_bytes(C.byref(n), h, w) == 0, (h, w)
        assert lib.surs_encoder_hourglass_backward_workspace_bytes(C.byref(n), h, w) == 0, (h, w)
    assert lib.surs_encoder_hourglass_tape_bytes(C.byref(n), 8, 12) > 0
    # a single block has no such rule
    assert lib.surs_encoder_convblock_tape_bytes(C.byref(n), 3, 5) > 0
    assert lib.surs_encoder_convblock_backward_workspace_bytes(C.byref(n), 3, 5) > 0
    with pytest.raises(ValueError, match="not a multiple of 2\\^2"):
        native.hg_tape_bytes(n, 6, 8, True)
    # the calls themselves: SURS_E_INVALID before anything is read
    ps = (_lib.HgBlockParams * 7)()
    with pytest.raises(_lib.SursError, match="not a multiple of 2\\^2"):
        _lib.check(lib.surs_encoder_hourglass_train(C.byref(n), 0, FAKE, 6, 8, 256, FAKE, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="not a multiple of 2\\^2"):
        _lib.check(lib.surs_encoder_hourglass_backward(C.byref(n), 0, ps, FAKE, 6, 8, FAKE, FAKE, ps, 0, FAKE, 1 << 30, None))


def test_refusals_carry_the_librarys_message():
    lib = _lib.lib()
    n, keep = _host_net()
    n1, keep1 = _host_net(parts=1)
    nb, keepb = _host_net(batch=True)
    with pytest.raises(ValueError, match="parts == 1"):
        native.hg_tape_bytes(n1, 8, 8, True)
    with pytest.raises(ValueError, match="--norm group only"):
        native.hg_tape_bytes(nb, 8, 8, False)
    ps = (_lib.HgBlockParams * 7)()
    with pytest.raises(_lib.SursError, match="null pointer in params"):
        _lib.check(lib.surs_encoder_convblock_backward(C.byref(n), C.byref(n.conv2), ps, FAKE, 4, 6, FAKE, FAKE, ps, 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="256-byte aligned"):
        _lib.check(lib.surs_encoder_convblock_train(C.byref(n), C.byref(n.conv2), FAKE, 4, 6, 256, FAKE, C.c_void_p(4096 + 64), 1 << 30, None))
    with pytest.raises(_lib.SursError, match="tape too small"):
        _lib.check(lib.surs_encoder_convblock_train(C.byref(n), C.byref(n.conv2), FAKE, 4, 6, 256, FAKE, FAKE, 1024, None))
    with pytest.raises(_lib.SursError, match="stack 3 of 1"):
        _lib.check(lib.surs_encoder_hourglass_train(C.byref(n), 3, FAKE, 8, 8, 256, FAKE, FAKE, 1 << 30, None))
    # the primitives
    with pytest.raises(_lib.SursError, match="64, 128 and 256"):
        _lib.check(lib.surs_groupnorm_relu_grad(FAKE, 96, FAKE, 96, 6, 96, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 96, 0, FAKE, FAKE, 0, FAKE, 1 << 20,
                                                None))
    with pytest.raises(_lib.SursError, match="pitches of at least c"):
        _lib.check(lib.surs_groupnorm_relu_grad(FAKE, 64, FAKE, 62, 6, 64, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 64, 0, FAKE, FAKE, 0, FAKE, 1 << 20,
                                                None))
    with pytest.raises(_lib.SursError, match="workspace too small"):
        _lib.check(lib.surs_groupnorm_relu_grad(FAKE, 64, FAKE, 64, 6, 64, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 64, 0, FAKE, FAKE, 0, FAKE, 16, None))
    assert lib.surs_groupnorm_relu_grad_workspace_bytes(6, 96) == 0
    with pytest.raises(_lib.SursError, match="multiple of 4"):
        _lib.check(lib.surs_avgpool2_grad(FAKE, 2, 3, 6, 8, FAKE, 8, 0, None))
    with pytest.raises(_lib.SursError, match="pitches of at least c"):
        _lib.check(lib.surs_bicubic_up2_grad(FAKE, 2, 3, 8, 6, FAKE, 8, 0, None))


def test_norm_batch_raises_not_implemented():
    from surs_amd import options
    o = options.BaseOptions().parse(hg.flags("cb_tiny") + ["--norm", "batch"])
    net = model.SuRSNet(o)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.conv_block_train("conv2", torch.zeros(1, 256, 4, 6))
    with pytest.raises(NotImplementedError, match="--norm group only"):
        net.hourglass_backward(0, torch.zeros(1, 256, 4, 4))


def test_param_keys_follow_the_state_dict():
    for name in hg.CASES:
        sd, o = hg.state_dict(name), hg.opt(name)
        keys = native.hg_param_keys(sd, o.num_stack_lr, o.hg_depth)
        assert keys == [k for k in sd if k in set(keys)]                      # state_dict() order
        assert all(k.startswith("image_filter_lr.") for k in keys) and not any(".bn4." in k for k in keys)
        n_blocks = 1 + o.num_stack_lr * (3 * o.hg_depth + 2)
        assert len(keys) == 9 * n_blocks + 6 * o.num_stack_lr + 4 * (o.num_stack_lr - 1)
        assert set(hg.param_keys(name)) <= set(keys)
        assert native.hg_block_prefixes(0, o.hg_depth) == hg.hourglass_blocks(0, o.hg_depth)
        for p in hg.hourglass_blocks(0, o.hg_depth):
            assert native.hg_block_keys(p) == hg.block_keys(p)


@pytest.mark.parametrize("name", list(hg.CASES))
def test_restatement_reproduces_the_fixture(golden_dir, name):
    gold = hg.load_fixture(golden_dir, name)
    assert float(gold["margin"]) >= hg.KINK_FACTOR
    x = hg.inputs(name, int(gold["seed"]))
    g64, L, z64 = hg.grads_of(name, x, hg.upstream(name), torch.float64, want_sites=True)
    _, _, z32 = hg.grads_of(name, x, hg.upstream(name), torch.float32, want_sites=True)
    margin, count = hg.kink_margin(z64, z32)
    assert count == int(gold["sites"])
    assert margin >= hg.KINK_FACTOR, margin        # (the restatement's own float32 run, not the reference's: the same condition)
    assert abs(L - float(gold["L"])) <= 1e-12 * abs(float(gold["L"]))
    assert list(g64) == hg.param_keys(name) + [hg.INPUT_KEY]
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
    found = [f for f in os.listdir(golden_dir) if f.startswith("hg_grads_")]
    assert found
    for f in found:
        assert os.path.getsize(os.path.join(golden_dir, f)) < 1 << 20, f
