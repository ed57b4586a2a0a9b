"""Host checks of the classifier gradients: grad_common.grads_f64 - the float64 numpy restatement the GPU tests lean on, written from
the formulas - against the reference's own float64 gradients (tests/golden/mlp_grads_*.npz, tools/gen_golden_grads.py), the
kink-safety of the stored point sets, the refusals of SuRSNet.forward_backward / classifier_grads, the binding's declarations."""
import numpy as np
import pytest
import torch

import grad_common as gc


@pytest.mark.parametrize("name", list(gc.CASES))
def test_restatement_reproduces_fixture(golden_dir, name):
    """Both sides are float64: 1e-9 of each quantity's max-abs is four orders above the rounding of these sums."""
    gold = gc.load_fixture(golden_dir, name)
    _, S, B, N = gc.CASES[name]
    assert tuple(gold["keep"].shape) == (B, N)
    assert all((np.diff(gold["keep"][b]) > 0).all() and gold["keep"][b].max() < gc.N_CAND for b in range(B))
    sd = gc.mlp_state(name)
    grads, info = gc.grads_f64(sd, gc.kept(gc.inputs(name), gold["keep"]))
    assert list(grads) == list(sd) and all(grads[k].shape == sd[k].shape for k in sd)
    res = gc.compare(gold, grads)
    worst = max(res, key=lambda r: r[1])
    print(name, "quantities", len(res), "worst", worst[0], worst[1], "error", info["error"], float(gold["error"]))
    assert all(dev <= 1e-9 for _, dev, _ in res), worst
    assert abs(info["error"] - float(gold["error"])) <= 1e-12 * abs(float(gold["error"]))
    # every stored quantity has its yardstick: the reference's own fp32 distance from float64
    assert all(np.isfinite(gold[q + "|e_ref"]) and gold[q + "|e_ref"] < 1e-4 for q, _, _ in res)
    # the stored index sets are kink-safe, and the masked points take part
    print(name, "margin", float(info["margin"].min()), "edge", float(info["edge"].min()))
    assert (info["margin"] >= gc.KINK_REL).all() and (info["edge"] >= gc.EDGE).all()
    if N > 1:
        assert (info["pred_lr"] == 0).any() and (info["pred_hr"] == 0).any()


def _net(more=(), projection="orthogonal"):
    from surs_amd import model, options
    import common
    return model.SuRSNet(options.BaseOptions().parse(common.FLAGS + list(more)), projection)


def _args(V=1):
    z = torch.zeros
    return (z(V, 3, 64, 64), z(V, 3, 128, 128), z(V, 3, 8), z(V, 3, 8), torch.eye(4)[None].repeat(V, 1, 1))


def test_refuses_multi_view_and_perspective():
    lab = dict(labels_lr=torch.zeros(1, 1, 8), labels_hr=torch.zeros(1, 1, 8))
    for net in (_net(["--num_views", "2"]), _net(projection="perspective")):
        with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal projection only"):
            net.forward_backward(*_args(net.num_views), **lab)
        with pytest.raises(NotImplementedError, match=r"classifier gradients \(forward_backward\(\), classifier_grads\(\)\)"):
            net.classifier_grads()


def test_classifier_grads_names_what_is_missing():
    net = _net()
    with pytest.raises(RuntimeError, match=r"preceding query_mr\(labels=\.\.\.\)"):
        net.classifier_grads()
    net._mr_points, net._mr_args = torch.zeros(1, 3, 8), (torch.eye(4)[None], None)
    with pytest.raises(RuntimeError, match=r"preceding query_sr\(labels=\.\.\.\)"):
        net.classifier_grads()
    net._sr_points, net._sr_args = torch.zeros(1, 3, 8), (torch.eye(4)[None], None)
    with pytest.raises(RuntimeError, match="labels_lr is not set: pass labels= to query_mr"):
        net.classifier_grads()
    net.labels_lr = torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError, match="labels_hr is not set: pass labels= to query_sr"):
        net.classifier_grads()
    net.labels_hr = torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):   # everything is there: the next thing it needs is the device
        net.classifier_grads()


def test_binding_declares_the_new_entries():
    from surs_amd import _lib, native
    assert "surs_mlp_grad" in _lib.EXPORTS and "surs_mlp_grad_workspace_bytes" in _lib.EXPORTS
    assert callable(native.mlp_grads) and callable(native.mlp_grad_workspace_bytes)
    sd = gc.mlp_state("mixed")
    assert native.mlp_param_keys(gc.shapes_of(sd)) == list(sd)
    assert gc.shapes_of(sd) == native.mlp_shapes(sd, gc.opt("mixed"))
    assert gc.shapes_of(gc.mlp_state("res0")) == native.mlp_shapes(gc.mlp_state("res0"), gc.opt("res0"))
    assert gc.shapes_of(gc.mlp_state("d48")) == native.mlp_shapes(gc.mlp_state("d48"), gc.opt("d48"))
