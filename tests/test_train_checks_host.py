"""CPU-only checks of what the backward wrappers of native.py - sr_backward, hg_backward, tail_backward, filter_lr_backward - refuse before
any library call: a `grads` that does not match the parameters and an upstream gradient that does not match the output.  One validator
of each kind serves the four, so CPU tensors and the host-built nets of the three *_grads_host modules are enough."""
import re
from collections import OrderedDict

import pytest
import torch

import hg_grad_common as hg
import sr_grad_common as sg
import tail_grad_common as tg
import test_hg_grads_host as hg_host
import test_sr_grads_host as sr_host
import test_tail_grads_host as tail_host
from surs_amd import native

TAPE = torch.empty(256, dtype=torch.uint8)      # never read: every case below is refused before the tape is looked at


def _sr():
    o = sg.opt("tiny")
    n, keep = sr_host._host_net(n_block=tuple(o.n_block))
    p = native.SrParams(sg.state_dict("tiny"), o.n_block, "cpu")
    call = lambda g, **kw: native.sr_backward(n, p, TAPE, 4, 8, g_img_sr=g, **kw)
    return keep, call, p.keys, p.tensors, (8, 16, 3), "g_img_sr"


def _hg():
    o = hg.opt("cb_tiny")
    n, keep = hg_host._host_net(depth=o.hg_depth)
    p = native.HgParams(hg.state_dict("cb_tiny"), o.num_stack_lr, o.hg_depth, "cpu").tensors
    prefixes = [native.HG + "conv2."]
    call = lambda g, **kw: native.hg_backward(n, n.conv2, prefixes, p, TAPE, 4, 6, g, **kw)
    return keep, call, native.hg_block_keys(prefixes[0]), p, (4, 6, 256), "g"


def _tail_net():
    o = tg.opt("joint57")
    n, keep = tail_host._host_net(stacks=o.num_stack_lr, depth=o.hg_depth, d=o.hg_dim)
    return o, n, keep, native.HgParams(tg.state_dict("joint57"), o.num_stack_lr, o.hg_depth, "cpu")


def _tail():
    o, n, keep, p = _tail_net()
    call = lambda g, **kw: native.tail_backward(n, 0, p.tensors, TAPE, 5, 7, g_out=g, **kw)
    return keep, call, native.hg_tail_keys(0, o.num_stack_lr), p.tensors, (5, 7, o.hg_dim), "g_out"


def _filter():
    o, n, keep, p = _tail_net()
    rest = [None] * (o.num_stack_lr - 1)
    call = lambda g, **kw: native.filter_lr_backward(n, o.hg_depth, p.keys, p.tensors, TAPE, 8, 8, [g] + rest, **kw)
    return keep, call, p.keys, p.tensors, (8, 8, o.hg_dim), "g_outs[0]"


@pytest.mark.parametrize("wrapper", [_sr, _hg, _tail, _filter], ids=["sr_backward", "hg_backward", "tail_backward", "filter_lr_backward"])
def test_grads_and_upstream_gradients_are_checked_before_the_library(wrapper):
    keep, call, keys, params, shape, arg = wrapper()
    g = torch.zeros(shape)
    full = lambda: OrderedDict((k, torch.zeros_like(params[k])) for k in keys)
    key = next(k for k in keys if params[k].dim() == 4 and params[k].shape[0] > 1 and params[k].shape[1] > 1)
    named = re.escape("grads[%r]" % key)
    with pytest.raises(ValueError, match="accumulate needs the grads"):
        call(g, accumulate=True)
    grads = full()
    del grads[key]
    with pytest.raises(ValueError, match=named):
        call(g, grads=grads)
    grads = full()
    grads[key] = torch.zeros(tuple(params[key].shape[:-1]) + (2,))
    with pytest.raises(ValueError, match=named):
        call(g, grads=grads)
    grads = full()
    grads[key] = torch.zeros_like(params[key], dtype=torch.float64)
    with pytest.raises(ValueError, match=named):
        call(g, grads=grads)
    grads = full()
    grads[key] = torch.zeros_like(params[key].transpose(0, 1).contiguous()).transpose(0, 1)
    assert tuple(grads[key].shape) == tuple(params[key].shape) and not grads[key].is_contiguous()
    with pytest.raises(ValueError, match=named):
        call(g, grads=grads)
    with pytest.raises(ValueError, match=re.escape(arg) + " must be"):
        call(torch.zeros(shape[:2] + (shape[2] + 1,)), grads=full())
    # the same gradient and grads pass both checks: the next refusal is the tape's
    with pytest.raises(ValueError, match="tape: "):
        call(g, grads=full())
