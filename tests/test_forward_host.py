"""CPU checks of the validation forward (SuRSNet.forward, tests/golden/forward_h64.npz): the fixture against its own float64
restatement, the conditions the fixture's inputs must meet, the refusals, the loss weights, and the new kernels' code objects."""
import json
import os

import numpy as np
import pytest
import torch

import common
import forward_common as fc
from surs_amd import model, native, options


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "forward_h64.npz"))


CASES = [(n, m) for n in fc.SHAPES for m in fc.MODES]


@pytest.mark.parametrize("name,mode", CASES)
def test_fixture_self_check(gold, name, mode):
    """The four terms and the total in float64 numpy from the fixture's own predictions, with forward()'s crossing of the label
    arguments (SuRSNet.py:249-250), against the reference's float32 values: 1e-6 (measured 2e-9 .. 1.1e-7)."""
    x, tag = fc.inputs(), "%s_%s_" % (name, mode)
    e, total = fc.terms_f64(gold[tag + "pred_lr"], gold[tag + "pred_hr"], x["labels_lr"], x["labels_hr"], gold["img_sr"], x["images_hr"])
    d = np.abs(e - gold[tag + "terms"].astype(np.float64))
    print(tag, "term differences", d, "total difference", abs(total - float(gold[tag + "total"])))
    assert d.max() < 1e-6
    assert abs(total - float(gold[tag + "total"])) < 1e-6
    # the uncrossed labels give another loss: the crossing is visible in the fixture
    e2, _ = fc.terms_f64(gold[tag + "pred_lr"], gold[tag + "pred_hr"], x["labels_hr"], x["labels_lr"], gold["img_sr"], x["images_hr"])
    assert np.abs(e2[:2] - gold[tag + "terms"][:2]).max() > 1e-3


def test_fixture_conditions(gold):
    meta = json.loads(str(gold["meta"]))
    assert (meta["B"], meta["H"], meta["N"]) == (fc.B, fc.H, fc.N) and tuple(meta["loss_weights"]) == fc.LOSS_WEIGHTS
    assert len(set(fc.LOSS_WEIGHTS)) == 4
    for name in fc.SHAPES:
        assert meta["flags"][name] == fc.flags(name)
        tr, ev = gold[name + "_train_pred_lr"], gold[name + "_eval_pred_lr"]
        assert tr.shape == (3, fc.B, fc.N) and gold[name + "_train_pred_hr"].shape == (3, fc.B, fc.N)
        assert ev.shape == (1, fc.B, fc.N) and gold[name + "_eval_pred_hr"].shape == (1, fc.B, fc.N)
        for s in range(2):   # a kernel that evaluates the wrong map cannot pass
            assert np.abs(tr[s] - tr[2]).max() > 0.05
        for k in ("_train_pred_lr", "_train_pred_hr", "_eval_pred_lr", "_eval_pred_hr"):
            outside = float(np.mean(gold[name + k][-1] == 0))   # (a masked prediction is exactly 0, a sigmoid never)
            assert 0.05 < outside < 0.5, (name, k, outside)
    x = fc.inputs()
    assert set(np.unique(x["labels_lr"])) == {0.0, 1.0} and set(np.unique(x["labels_hr"])) == {0.0, 1.0}
    assert not np.array_equal(x["labels_lr"], x["labels_hr"]) and not np.array_equal(x["points_lr"], x["points_hr"])
    assert gold["img_sr"].shape == x["images_hr"].shape


def _forward_args():
    x = fc.inputs()
    T = lambda k: torch.from_numpy(x[k])
    return (T("images_lr"), T("images_hr"), T("points_lr"), T("points_hr"), T("calibs")), dict(labels_lr=T("labels_lr"),
                                                                                                 labels_hr=T("labels_hr"))


def test_forward_refuses_multi_view_and_perspective():
    a, k = _forward_args()
    net = model.SuRSNet(options.BaseOptions().parse(fc.flags("released", ["--num_views", "2"])))
    with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal projection only"):
        net.forward(*a, **k)
    net = model.SuRSNet(options.BaseOptions().parse(fc.flags("released")), projection_mode="perspective")
    with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal projection only"):
        net.forward(*a, **k)
    # every kept stack outside forward(): the same limit, named the same way
    net.im_feat_list_lr = [torch.zeros(1, 256, 4, 4)] * 3
    net.im_feat_list_hr = [torch.zeros(1, 64, 16, 16)]
    with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal projection only"):
        net.query_mr(a[3][:1], a[4][:1])


def test_forward_needs_labels():
    a, _ = _forward_args()
    with pytest.raises(ValueError, match="labels_lr and labels_hr"):
        model.SuRSNet(common.opt()).forward(*a)


def test_loss_weights_come_from_the_options(monkeypatch):
    d = options.BaseOptions().parse(common.FLAGS)
    assert (d.mlp1, d.mlp2, d.srweight, d.dispweight) == (1.0, 1.0, 1.0, 1.0)     # the reference's defaults (lib/options.py)
    opt = options.BaseOptions().parse(fc.flags("released"))
    assert (opt.mlp1, opt.mlp2, opt.srweight, opt.dispweight) == fc.LOSS_WEIGHTS
    net = model.SuRSNet(opt)
    seen = {}

    def fake(**kw):
        seen.update(kw)
        return torch.zeros(4), torch.zeros(())
    monkeypatch.setattr(native, "forward_losses", fake)
    monkeypatch.setattr(net, "_device", lambda: torch.device("cpu"))
    net.intermediate_preds_list_lr = [torch.rand(2, 1, 5) for _ in range(3)]
    net.intermediate_preds_list_hr = [torch.rand(2, 1, 5) for _ in range(3)]
    net.labels_lr, net.labels_hr = torch.ones(2, 1, 5), torch.zeros(2, 1, 5)
    net.loss_terms(torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4))
    assert tuple(seen["weights"]) == fc.LOSS_WEIGHTS
    assert tuple(seen["pred_lr"].shape) == (3, 10) and tuple(seen["pred_hr"].shape) == (3, 10)
    assert torch.equal(seen["lab_lr"], torch.ones(10)) and torch.equal(seen["lab_hr"], torch.zeros(10))
    net.opt.dispweight = 7.0
    net.loss_terms(torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4))
    assert tuple(seen["weights"]) == fc.LOSS_WEIGHTS[:3] + (7.0,)


def test_labels_are_stored_as_the_reference_stores_them(monkeypatch):
    """query_mr(labels=) -> labels_lr, query_sr(labels=) -> labels_hr (SuRSNet.py:134-136, 164-165); forward crosses them."""
    net = model.SuRSNet(common.opt())
    calls = []
    monkeypatch.setattr(net, "super_res", lambda im: (im, im, im))
    monkeypatch.setattr(net, "filter_lr", lambda f: None)
    monkeypatch.setattr(net, "filter_hr", lambda f: None)
    monkeypatch.setattr(net, "_query_stacks", lambda p, c, t, p_lr=None, lr_only=False: (calls.append((p, p_lr is not None, lr_only)),
                        (None if lr_only else [torch.zeros(1, 1, 3)], [torch.zeros(1, 1, 3)] if p_lr is None else None))[1])
    monkeypatch.setattr(net, "_query", lambda p, c, t, p_lr=None: (calls.append((p, p_lr is not None, False)),
                        (torch.zeros(1, 1, 3), torch.zeros(1, 1, 3)))[1])
    monkeypatch.setattr(net, "loss_terms", lambda sr, hr: (torch.zeros(4), torch.zeros(())))
    net.im_feat_list_lr = [torch.zeros(1, 256, 4, 4)]
    p_lr, p_hr = torch.zeros(1, 3, 3), torch.ones(1, 3, 3)
    l_lr, l_hr = torch.zeros(1, 1, 3), torch.ones(1, 1, 3)
    net.forward(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 16, 16), p_lr, p_hr, torch.eye(4)[None], labels_lr=l_lr, labels_hr=l_hr)
    assert net.labels_lr is l_hr and net.labels_hr is l_lr
    # an lr-only pass on points_hr, then the hr classifier alone on points_lr
    assert [(c[0] is p_hr, c[1], c[2]) for c in calls] == [(True, False, True), (False, True, False)] and calls[1][0] is p_lr


def test_stacks_kernels_use_no_scratch(tmp_path):
    """The compiler's resource usage of the stacks instantiations (3 operand splits x 2 tile sizes x both / lr-only, for D = 256 and
    for any other D) and of the two loss kernels in the shipped code object, read as
    tests/test_mlp_shapes_host.py::test_fused_kernels_use_no_scratch reads it."""
    import isa
    meta = {}
    for co in isa.code_objects(workdir=str(tmp_path)):
        meta.update(isa.kernel_metadata(co))
    for tag, count in (("mlp_stacks_kernel", 12), ("mlp_stacks_anyd_kernel", 12)):
        ks = {k: v for k, v in meta.items() if tag in k}
        assert len(ks) == count, sorted(ks)
        for name, m in ks.items():
            assert m[".private_segment_fixed_size"] == 0, name
            assert m[".vgpr_count"] + m.get(".agpr_count", 0) <= 256, name
            assert m[".group_segment_fixed_size"] == 0, name
    loss = {k: v for k, v in meta.items() if "loss_partial_kernel" in k or "loss_final_kernel" in k}
    assert len(loss) == 2, sorted(loss)
    for name, m in loss.items():
        assert m[".private_segment_fixed_size"] == 0, name
