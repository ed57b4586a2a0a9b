"""Host checks of the feature-map gradients: feat_grad_common.map_grads_f64 - the float64 restatement the GPU tests lean on, d X of
grad_common.mlp_backward scattered through grad_common.bilinear's taps - against the reference's own float64 gradients
(tests/golden/feat_grads_*.npz, tools/gen_golden_feat_grads.py) and against finite differences of grad_common.grads_f64's error; what
the stored point sets must exercise; the refusals; the binding's declarations."""
import numpy as np
import pytest
import torch

import feat_grad_common as fg
import grad_common as gc

_memo = {}


def _case(golden_dir, name):
    if name not in _memo:
        gold, x = fg.kept_inputs(golden_dir, name)
        sd = gc.mlp_state(name)
        _memo[name] = (gold, x, sd, fg.map_grads_f64(sd, x))
    return _memo[name]


@pytest.mark.parametrize("name", list(fg.CASES))
def test_restatement_reproduces_fixture(golden_dir, name):
    """Both sides are float64: 1e-9 of each tensor's max-abs is orders above the rounding of these sums."""
    gold, x, sd, (g_lr, g_hr, error) = _case(golden_dir, name)
    S, B, N, (hl, wl), (hh, wh) = fg.CASES[name]
    D = fg.opt(name).hg_dim
    assert tuple(gold["keep"].shape) == (B, N)
    assert all((np.diff(gold["keep"][b]) > 0).all() and gold["keep"][b].max() < gc.N_CAND for b in range(B))
    got = fg.named(g_lr, g_hr)
    assert list(got) == fg.tensor_names(name)
    assert all(got["lr%d" % s].shape == (B, D, hl, wl) == gold["lr%d" % s].shape for s in range(S))
    assert got["hr"].shape == (B, 64, hh, wh) == gold["hr"].shape
    res = fg.compare(gold, got)
    worst = max(res, key=lambda r: r[1])
    print(name, "tensors", len(res), "worst", worst[0], worst[1], "error", error, float(gold["error"]))
    assert all(dev <= 1e-9 for _, dev, _ in res), worst
    assert abs(error - float(gold["error"])) <= 1e-12 * abs(float(gold["error"]))
    assert all(np.isfinite(gold[k + "|e_ref"]) and gold[k + "|e_ref"] < 1e-4 for k in got)


@pytest.mark.parametrize("name", list(fg.CASES))
def test_stored_point_sets(golden_dir, name):
    """Kink-safe (grad_common's definition, on the kept points' own layer maxima), masked points take part, and the generator's
    coverage conditions hold on the stored indices."""
    gold, x, sd, _ = _case(golden_dir, name)
    _, info = gc.grads_f64(sd, x)
    print(name, "margin", float(info["margin"].min()), "edge", float(info["edge"].min()))
    assert (info["margin"] >= gc.KINK_REL).all() and (info["edge"] >= gc.EDGE).all()
    assert (info["pred_lr"] == 0).any() and (info["pred_hr"] == 0).any()
    assert abs(info["error"] - float(gold["error"])) <= 1e-12 * abs(float(gold["error"]))
    cov = fg.coverage(name, x)
    print(name, "coverage", cov)
    fg.check_coverage(name, cov)
    if name == "d48":
        # the pixels that receive nothing hold exact zeros in the reference's gradient too
        assert int((np.abs(gold["hr"][0]).max(0) == 0).sum()) == cov["hr_empty"] >= 1


def test_scatter_is_the_transpose_of_the_gather():
    """<bilinear(F), d> == <F, scatter(d)> for random F, d on a non-square map, with points outside, on the border and on pixel
    centres."""
    rng = np.random.RandomState(5)
    C, H, W = 3, 5, 7
    x = np.concatenate([rng.uniform(-1.2, 1.2, 40), [-1.0, 1.0, 1.0, 0.0, 1.0 / 3.0]])
    y = np.concatenate([rng.uniform(-1.2, 1.2, 40), [1.0, -1.0, 1.0, 0.5, -1.0]])
    F, d = rng.standard_normal((C, H, W)), rng.standard_normal((C, x.size))
    lhs, rhs = float((gc.bilinear(F, x, y) * d).sum()), float((F * fg.scatter(C, H, W, x, y, d)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # a point on x = 1: the upper tap lies at W - it has no weight and the clamped pixel it names receives exactly nothing from it
    one = fg.taps(H, W, np.array([1.0]), np.array([0.2]))
    assert not one[1][2][0] and one[1][1][0] == 0.0 and one[0][2][0] and one[0][1][0] > 0.0


@pytest.mark.parametrize("name", ["tiny", "res0"])
def test_restatement_against_finite_differences(golden_dir, name):
    """Central differences of grad_common.grads_f64's error in a handful of map elements (the largest gradient element of every
    tensor and seeded others).  The error is linear in a map element up to the LeakyReLU kinks, and the points are kink-safe: h =
    1e-6 moves no pre-activation across 0 (margin 1e-5 of the layer maximum), so the error is smooth over the step.  The difference
    quotient then carries the cancellation error 2^-52 |error| / h ~ 4e-10 (error ~ 1.7) and a curvature term ~ h^2; the tensors'
    maxima are 1e-3 and above, so it is good to ~ 4e-7 of a maximum; 1e-6 is asked."""
    gold, x, sd, (g_lr, g_hr, _) = _case(golden_dir, name)
    S, B = fg.CASES[name][:2]
    h = 1e-6
    rng = np.random.RandomState(11)

    def err(key, s, b, idx, delta):
        maps = x[key]
        arr = (maps[b][s] if key == "feat_lr" else maps[b]).astype(np.float64)
        arr[idx] += delta
        x2 = dict(x)
        if key == "feat_lr":
            x2[key] = [[arr if (bb, ss) == (b, s) else maps[bb][ss] for ss in range(S)] for bb in range(B)]
        else:
            x2[key] = [arr if bb == b else maps[bb] for bb in range(B)]
        return gc.grads_f64(sd, x2)[1]["error"]

    for key, s, g in [("feat_lr", s, g_lr[s]) for s in range(S)] + [("feat_hr", 0, g_hr)]:
        top = np.unravel_index(np.abs(g).argmax(), g.shape)
        picks = [top] + [tuple(rng.randint(0, n) for n in g.shape) for _ in range(2)]
        for b, *idx in picks:
            idx = tuple(idx)
            fd = (err(key, s, b, idx, h) - err(key, s, b, idx, -h)) / (2 * h)
            dev = abs(fd - g[(b,) + idx]) / np.abs(g).max()
            print(name, key, s, (b,) + idx, "restated", g[(b,) + idx], "difference quotient", fd, "dev", dev)
            assert dev <= 1e-6


def _net(more=(), projection="orthogonal"):
    from surs_amd import model, options
    import common
    return model.SuRSNet(options.BaseOptions().parse(common.FLAGS + list(more)), projection)


def test_refuses_multi_view_and_perspective():
    from surs_amd import autograd
    z = torch.zeros
    lab = dict(labels_lr=z(1, 1, 8), labels_hr=z(1, 1, 8))
    for net in (_net(["--num_views", "2"]), _net(projection="perspective")):
        V = net.num_views
        args = (z(V, 3, 64, 64), z(V, 3, 128, 128), z(V, 3, 8), z(V, 3, 8), torch.eye(4)[None].repeat(V, 1, 1))
        with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal projection only"):
            net.forward_backward(*args, features=True, **lab)
        with pytest.raises(NotImplementedError, match=r"classifier gradients \(forward_backward\(\), classifier_grads\(\)\)"):
            net.classifier_grads(features=True)
        with pytest.raises(NotImplementedError, match=r"classifier gradients \(forward_backward\(\), classifier_grads\(\)\)"):
            autograd.point_loss(net, [z(V, 256, 4, 4)], z(V, 64, 8, 8), z(V, 3, 8), z(V, 3, 8), torch.eye(4)[None].repeat(V, 1, 1),
                                z(V, 1, 8), z(V, 1, 8))


def test_names_what_is_missing():
    net = _net()
    with pytest.raises(RuntimeError, match=r"preceding query_mr\(labels=\.\.\.\)"):
        net.classifier_grads(features=True)
    net._mr_points, net._mr_args = torch.zeros(1, 3, 8), (torch.eye(4)[None], None)
    with pytest.raises(RuntimeError, match=r"preceding query_sr\(labels=\.\.\.\)"):
        net.classifier_grads(features=True)
    net._sr_points, net._sr_args = torch.zeros(1, 3, 8), (torch.eye(4)[None], None)
    with pytest.raises(RuntimeError, match="labels_lr is not set: pass labels= to query_mr"):
        net.classifier_grads(features=True)
    net.labels_lr = torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError, match="labels_hr is not set: pass labels= to query_sr"):
        net.classifier_grads(features=True)


def test_binding_declares_the_new_entries():
    import inspect
    from surs_amd import _lib, autograd, model, native
    assert "surs_mlp_grad_features" in _lib.EXPORTS and "surs_mlp_grad_features_workspace_bytes" in _lib.EXPORTS
    assert "surs_mlp_grad" in _lib.EXPORTS and "surs_mlp_grad_workspace_bytes" in _lib.EXPORTS
    # surs_mlp_grad's arguments plus gfeat_lr, gfeat_hr, accumulate_features, in front of the workspace
    old, new = _lib._SIGS["surs_mlp_grad"][1], _lib._SIGS["surs_mlp_grad_features"][1]
    assert len(new) == len(old) + 3 and new[:len(old) - 3] == old[:-3] and new[-3:] == old[-3:]
    assert callable(native.mlp_grad_features_workspace_bytes) and callable(autograd.point_loss)
    p = inspect.signature(native.mlp_grads).parameters
    assert p["feat_grads"].default is None and p["accumulate_features"].default is False
    assert inspect.signature(model.SuRSNet.classifier_grads).parameters["features"].default is False
    assert inspect.signature(model.SuRSNet.forward_backward).parameters["features"].default is False
    f = native.FeatGrads([torch.zeros(5, 7, 256)], torch.zeros(9, 6, 64))
    assert len(f.lr) == 1 and tuple(f.hr.shape) == (9, 6, 64)
