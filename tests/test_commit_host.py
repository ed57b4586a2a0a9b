"""Host-only checks of SuRSNet.commit() and what goes with it: the refusals that need no device, and a state_dict() that nothing has
been committed into."""
import pytest
import torch

import common
from surs_amd import _lib, model, options


def _net(more=()):
    return model.SuRSNet(options.BaseOptions().parse(common.FLAGS + list(more)))


def test_commit_refusals_without_a_device():
    net = _net()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.commit()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.commit(("mlp",))
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.mlp_parameters()
    with pytest.raises(ValueError, match="unknown parameter set"):
        net.commit(("mlp", "filters"))
    with pytest.raises(ValueError, match="unknown parameter set"):
        net.commit("encoder")
    with pytest.raises(NotImplementedError, match="--norm group only"):
        _net(["--norm", "batch"]).commit(("hg",))
    with pytest.raises(RuntimeError, match="no CPU path"):      # (the other sets are not refused for the norm)
        _net(["--norm", "batch"]).commit(("sr",))


def test_state_dict_untouched_when_nothing_was_committed():
    net = _net()
    sd0 = common.state_dict()
    net.load_state_dict(sd0)
    assert net._stale == set()
    sd = net.state_dict()
    assert list(sd) == [k for k, _, _ in net._spec] == list(sd0)
    for k, v in sd.items():
        assert torch.equal(v, torch.as_tensor(sd0[k])), k
    held = dict(net._sd)
    net.to(torch.device("cpu"))
    assert all(net._sd[k] is held[k] for k in held)          # (to() writes nothing back: the tensors are the loaded ones)
    assert [p.data_ptr() for p in net.parameters()] == [v.data_ptr() for v in held.values()]
    net.load_state_dict(sd0)
    assert net._stale == set()


def test_repack_entries_are_bound():
    """The binding covers the device-repack entries; SursRepackItem is the header's struct (five ints and pointers, 48 bytes)."""
    import ctypes as C
    for name in ("surs_conv_repack", "surs_conv_repack_tiles", "surs_conv1x1_merge", "surs_mlp_repack", "surs_mlp_repack_generic"):
        assert name in _lib.EXPORTS, name
    assert C.sizeof(_lib.RepackItem) == 48 and _lib.RepackItem.packed.offset == 24
    tiles = _lib.lib().surs_conv_repack_tiles
    assert tiles(64, 16, 3) == 1 and tiles(65, 17, 3) == 4 and tiles(256, 16, 1) == 4 and tiles(16, 256, 1) == 4
    assert tiles(512, 512, 3) == 8 * 32 and tiles(64, 64, 2) == 0 and tiles(0, 16, 3) == 0
