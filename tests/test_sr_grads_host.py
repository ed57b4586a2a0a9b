"""CPU-only checks of the super-resolution gradients: the binding, the refusals that need no device, and the fixtures
(tests/golden/sr_grads_*.npz) against the project's own float64 restatement of the network (sr_grad_common.forward + torch autograd
on the CPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_common as gc
import sr_grad_common as sg
from surs_amd import _lib, model, native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["surs_conv_grad_weight_workspace_bytes", "surs_conv_grad_weight", "surs_conv_grad_input", "surs_pixel_unshuffle2_grad",
       "surs_encoder_sr_tape_bytes", "surs_encoder_sr_backward_workspace_bytes", "surs_encoder_super_res_train",
       "surs_encoder_super_res_backward"]
FAKE = C.c_void_p(4096)   # a non-null pointer for calls that are refused before anything is read


def test_abi_has_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "surs.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert "SursSrParams" in hdr and "SursSrParam" in hdr


def _host_net(parts=2, n_block=(1, 1, 1), residual=1):
    """A SursEncoderNet with the shapes of SuRSSR_v3 and no weights behind it: enough for the size queries and the refusals."""
    cv = lambda cin, cout, k=3: _lib.Conv(None, None, None, cin, cout, k, 0)
    n = _lib.EncoderNet()
    n.residual, n.num_stack, n.hg_depth, n.parts, n.flags = residual, 1, 2, parts, 0
    n.n_block = (C.c_int * 3)(*n_block)
    n.head = cv(3, 32)
    n.down = (_lib.Conv * 3)(cv(32, 32), cv(64, 64), cv(128, 128))
    n.tail0 = (_lib.Conv * 3)(cv(32, 32), cv(64, 64), cv(128, 128))
    n.tail2 = (_lib.Conv * 3)(cv(32, 64), cv(64, 128), cv(128, 256))
    n.bottleneck, n.bott2, n.ups2, n.ups3, n.ups4 = cv(256, 256), cv(512, 512), cv(256, 256), cv(128, 128), cv(64, 64)
    n.last0, n.last2, n.conv5 = cv(64, 32), cv(32, 3), cv(64, 64, 1)
    body = [cv(c, c) for c, nb in zip((32, 64, 128), n_block) for _ in range(2 * nb)]
    arr = (_lib.Conv * max(1, len(body)))(*body)
    n.body = arr
    return n, arr


def test_size_queries_depend_on_net_and_size_only():
    n, keep = _host_net()
    a, b = native.sr_tape_bytes(n, 4, 8), native.sr_backward_workspace_bytes(n, 4, 8)
    assert a > 0 and b > 0 and a % 256 == 0
    assert native.sr_tape_bytes(n, 4, 8) == a and native.sr_backward_workspace_bytes(n, 4, 8) == b
    assert native.sr_tape_bytes(n, 8, 8) > a
    n2, keep2 = _host_net(n_block=(2, 0, 1))
    assert native.sr_tape_bytes(n2, 4, 8) != a
    n3, keep3 = _host_net(residual=0)          # the blocks do not run: no buffers for them
    assert native.sr_tape_bytes(n3, 4, 8) < a


def test_refusals_carry_the_librarys_message():
    lib = _lib.lib()
    n1, keep1 = _host_net(parts=1)
    with pytest.raises(ValueError, match="parts == 1"):
        native.sr_tape_bytes(n1, 4, 8)
    with pytest.raises(ValueError, match="parts == 1"):
        native.sr_backward_workspace_bytes(n1, 4, 8)
    n, keep = _host_net()
    with pytest.raises(ValueError, match="multiples of 4"):
        native.sr_tape_bytes(n, 5, 8)
    with pytest.raises(ValueError, match="refused"):
        native.conv_grad_weight_workspace_bytes(4, 4, 8, 8, 5)
    # the primitives: refused before any pointer is read
    with pytest.raises(_lib.SursError, match="kernel size 5"):
        _lib.check(lib.surs_conv_grad_weight(FAKE, 4, 4, 8, 8, None, 0, 1.0, FAKE, 4, 4, 8, 8, 5, 1, FAKE, FAKE, 0, FAKE, 1 << 20, None))
    with pytest.raises(_lib.SursError, match="stride 2 with a 1 x 1"):
        _lib.check(lib.surs_conv_grad_input(FAKE, 2, 2, 8, 8, None, 0, 1.0, FAKE, 8, 1, 2, FAKE, 4, 4, 8, 0, None))
    with pytest.raises(_lib.SursError, match="gives a 2 x 4 output, not 4 x 8"):
        _lib.check(lib.surs_conv_grad_input(FAKE, 4, 8, 8, 8, None, 0, 1.0, FAKE, 8, 3, 2, FAKE, 4, 8, 8, 0, None))
    with pytest.raises(_lib.SursError, match="pitch below the channel count"):
        _lib.check(lib.surs_conv_grad_weight(FAKE, 4, 4, 8, 7, None, 0, 1.0, FAKE, 4, 4, 8, 8, 3, 1, FAKE, FAKE, 0, FAKE, 1 << 20, None))
    with pytest.raises(_lib.SursError, match="workspace too small"):
        _lib.check(lib.surs_conv_grad_weight(FAKE, 4, 4, 8, 8, None, 0, 1.0, FAKE, 4, 4, 8, 8, 3, 1, FAKE, FAKE, 0, FAKE, 16, None))
    with pytest.raises(_lib.SursError, match="pitch below the channel count"):
        _lib.check(lib.surs_pixel_unshuffle2_grad(FAKE, 2, 2, 8, 8, FAKE, 8, 0.04, FAKE, 31, None))
    # the network: every upstream gradient missing, a null parameter, a tape that is not aligned
    ps = _lib.SrParamsStruct()
    with pytest.raises(_lib.SursError, match="no upstream gradient"):
        _lib.check(lib.surs_encoder_super_res_backward(C.byref(n), C.byref(ps), FAKE, 4, 8, None, None, None, C.byref(ps), 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="null weight or bias"):
        _lib.check(lib.surs_encoder_super_res_backward(C.byref(n), C.byref(ps), FAKE, 4, 8, FAKE, None, None, C.byref(ps), 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="parts == 1"):
        _lib.check(lib.surs_encoder_super_res_backward(C.byref(n1), C.byref(ps), FAKE, 4, 8, FAKE, None, None, C.byref(ps), 0, FAKE, 1 << 30, None))
    with pytest.raises(_lib.SursError, match="256-byte aligned"):
        _lib.check(lib.surs_encoder_super_res_train(C.byref(n), FAKE, 4, 8, 3, FAKE, FAKE, FAKE, FAKE, C.c_void_p(4096 + 64), 1 << 30, None))
    with pytest.raises(_lib.SursError, match="tape too small"):
        _lib.check(lib.surs_encoder_super_res_train(C.byref(n), FAKE, 4, 8, 3, FAKE, FAKE, FAKE, FAKE, FAKE, 1024, None))


def test_param_keys_follow_the_state_dict():
    for name in sg.CASES:
        sd, o = sg.state_dict(name), sg.opt(name)
        keys = native.sr_param_keys(sd, o.n_block)
        assert keys == sg.param_keys(name)
        assert keys == [k for k in sd if k in set(keys)]                       # state_dict() order
        assert not any("sub_mean" in k or "add_mean" in k for k in keys)
        assert "image_filter_hr.conv5.weight" in keys and "image_filter_hr.conv5.bias" in keys
        assert len(keys) == 2 * (17 + 2 * sum(o.n_block) + 1)     # head, 3 x (down, tail.0, tail.2), 7 more, the blocks, conv5
        # SursEncoderNet's order names every convolution exactly once
        names = ["super_resolution." + m for _, _, m in native.sr_conv_names(o.n_block)]
        assert sorted(names + ["image_filter_hr.conv5"]) == sorted({k.rsplit(".", 1)[0] for k in keys})


def test_backward_without_a_tape_raises():
    net = model.SuRSNet(sg.opt("tiny"))
    with pytest.raises(RuntimeError, match="super_res_train"):
        net.super_res_backward(grad_img_SR=torch.zeros(1, 3, 8, 16))


@pytest.mark.parametrize("name", list(sg.CASES))
def test_restatement_reproduces_the_fixture(golden_dir, name):
    gold = sg.load_fixture(golden_dir, name)
    assert float(gold["margin"]) >= sg.KINK_FACTOR
    x = sg.images(name, int(gold["seed"]))
    g64, L, z64 = sg.grads_of(name, x, sg.upstream(name), torch.float64, want_sites=True)
    _, _, z32 = sg.grads_of(name, x, sg.upstream(name), torch.float32, want_sites=True)
    margin, count = sg.kink_margin(z64, z32)
    assert count == int(gold["sites"])
    assert margin >= sg.KINK_FACTOR, margin        # (the restatement's own float32 run, not the reference's: the same condition)
    assert abs(L - float(gold["L"])) <= 1e-10 * abs(float(gold["L"]))
    assert list(g64) == sg.param_keys(name)
    worst = 0.0
    for key, g in g64.items():
        for qname, got in gc.quantities(key, g):
            ref = gold[qname]
            top = float(np.abs(ref).max())
            dev = float(np.abs(got - ref).max()) / top if top > 0 else float(np.abs(got).max())
            worst = max(worst, dev)
            assert dev <= 1e-10, (qname, dev)
            assert 0.0 <= float(gold[qname + "|e_ref"]) < 1e-4, qname
    print(name, "worst deviation of the restatement", worst, "margin", margin)


def test_fixture_files_stay_small(golden_dir):
    for f in os.listdir(golden_dir):
        if f.startswith("sr_grads_"):
            assert os.path.getsize(os.path.join(golden_dir, f)) < 1 << 20, f
