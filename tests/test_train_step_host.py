"""The training step without a device: the non-finite guard's host twin (surs_tensors_nonfinite_host) on the tables of
tests/train_step_common.py, the loss head's host gradient against the torch expression, the reshape helpers against a restatement of
lib/train_util.py:14-51, sample_util's PLY files byte for byte against tests/golden/samples_prob.ply, the option wiring of
apps/train_SuRS.py with a stand-in net, the refusals of forward_backward(encoder=True), the new entry points in the header and the
library, and the fixture's own promises (every live pair moves the float64 error by at least 256 resolutions)."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import train_step_common as ts
import sample_ply_common as sp
from surs_amd import _lib, model, native, options, sample_util, train_util

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("surs_forward_losses_grad", "surs_forward_losses_grad_workspace_bytes", "surs_forward_losses_grad_host",
               "surs_tensors_nonfinite", "surs_tensors_nonfinite_workspace_bytes", "surs_tensors_nonfinite_check",
               "surs_tensors_nonfinite_host")


# ------------------------------------------------------------------ the guard's host twin
@pytest.mark.parametrize("name", list(ts.GUARD_POISON))
def test_guard_host_twin(name):
    arrays, want = ts.guard_table(name)
    assert native.tensors_nonfinite_host(arrays) == want
    ref = next((i for i, a in enumerate(arrays) if not np.isfinite(a).all()), -1)     # numpy's own answer
    assert ref == want


def test_guard_host_twin_edges():
    assert native.tensors_nonfinite_host([]) == -1
    assert native.tensors_nonfinite_host([np.zeros(0, np.float32), np.array([np.nan], np.float32)]) == 1
    # every non-finite bit pattern class: quiet and signalling NaNs of both signs, both infinities; the largest finite values are not
    for bits, bad in ((0x7fc00000, True), (0xffc00000, True), (0x7f800001, True), (0xff800001, True), (0x7f800000, True),
                      (0xff800000, True), (0x7f7fffff, False), (0xff7fffff, False), (0x00000001, False), (0x80000000, False)):
        a = np.array([bits], np.uint32).view(np.float32)
        assert native.tensors_nonfinite_host([np.ones(5, np.float32), a]) == (1 if bad else -1), hex(bits)
    with pytest.raises(ValueError, match="contiguous float32"):
        native.tensors_nonfinite_host([np.zeros(4, np.float64)])


def test_guard_table_check_refuses():
    a = np.zeros(5000, np.float32)
    items, total = native.tensor_refs([(a.ctypes.data, a.size), (a.ctypes.data, 1)])
    assert total == 3 and [it.chunk_end for it in items] == [2, 3]
    items[1].chunk_end = 4
    with pytest.raises(_lib.SursError, match="prefix sum"):
        _lib.check(_lib.lib().surs_tensors_nonfinite_check(C.cast(items, C.c_void_p), 2, None))
    with pytest.raises(_lib.SursError, match="null pointer"):
        native.tensor_refs([(None, 3)])
    with pytest.raises(_lib.SursError, match="n = -1"):
        native.tensor_refs([(a.ctypes.data, -1)])


# ------------------------------------------------------------------ the loss head's gradient rule
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 8, 16)])
def test_loss_head_host_gradient_is_the_torch_expression(shape):
    B, Cc, H, W = shape
    rng = np.random.default_rng(5)
    sr = rng.normal(0, 1, (B, Cc, H, W)).astype(np.float32)
    hr = rng.normal(0, 1, (B, Cc, H, W)).astype(np.float32)
    hr.reshape(-1)[::5] = sr.reshape(-1)[::5]                      # exact equality: gradient 0
    sr_nhwc = np.ascontiguousarray(sr.transpose(0, 2, 3, 1))
    for w in (1.0, 0.25, 0.0, 3.0):
        got = native.forward_losses_grad_host(sr_nhwc, hr, w)
        # the fp32 reciprocal of k times the weight (torch's division of a device tensor by a host scalar), times the sign
        want = np.sign(sr - hr) * (np.float32(w) * (np.float32(1.0) / np.float32(sr.size)))
        assert want.dtype == np.float32
        assert np.array_equal(got.transpose(0, 3, 1, 2).view(np.uint32), want.view(np.uint32)), w
        assert (got.transpose(0, 3, 1, 2)[sr == hr] == 0).all()
    sr_nhwc[0, 0, 0, 0] = np.nan
    assert np.isnan(native.forward_losses_grad_host(sr_nhwc, hr, 1.0)[0, 0, 0, 0])      # a NaN stays a NaN: the guard must see it


# ------------------------------------------------------------------ helpers of the application
def test_reshape_helpers():
    """lib/train_util.py:14-51 restated: the view batch and view dimensions merged, batch-major; samples repeated per view."""
    B, V = 2, 3
    hr = torch.arange(B * V * 3 * 4 * 6, dtype=torch.float32).reshape(B, V, 3, 4, 6)
    lr = torch.arange(B * V * 3 * 2 * 3, dtype=torch.float32).reshape(B, V, 3, 2, 3)
    cal = torch.arange(B * V * 16, dtype=torch.float32).reshape(B, V, 4, 4)
    a, b, c = train_util.reshape_multiview_tensors(hr, lr, cal)
    assert a.shape == (B * V, 3, 4, 6) and b.shape == (B * V, 3, 2, 3) and c.shape == (B * V, 4, 4)
    for i in range(B):
        for v in range(V):
            assert torch.equal(a[i * V + v], hr[i, v]) and torch.equal(b[i * V + v], lr[i, v]) and torch.equal(c[i * V + v], cal[i, v])
    assert a.data_ptr() == hr.data_ptr()                           # views
    s = torch.arange(B * 3 * 5, dtype=torch.float32).reshape(B, 3, 5)
    assert train_util.reshape_sample_tensor(s, 1) is s
    r = train_util.reshape_sample_tensor(s, V)
    assert r.shape == (B * V, 3, 5) and all(torch.equal(r[i * V + v], s[i]) for i in range(B) for v in range(V))
    with pytest.raises(ValueError, match="B,V,C,H,W"):
        train_util.reshape_multiview_tensors(hr[0], lr, cal)


def test_samples_ply_bytes(tmp_path, golden_dir):
    pts, prob = sp.samples()
    path = str(tmp_path / "s.ply")
    sample_util.save_samples_truncted_prob(path, pts, prob)
    got = open(path, "rb").read()
    assert got == open(os.path.join(golden_dir, "samples_prob.ply"), "rb").read()
    lines = got.decode().split("\n")
    assert lines[2] == "element vertex %d" % sp.N and lines[9] == "end_header" and lines[-1] == ""
    assert lines[10].endswith(" 0 0 0") and lines[11].endswith(" 0 255 0") and lines[12].endswith(" 255 0 0")   # 0.5, 0, 1
    # the rgb form is the same writer: colours 255 rgb, truncated
    sample_util.save_samples_rgb(path, pts[:2], np.array([[1.0, 0.5, 0.0], [0.999, 0.0, 1.0]]))
    assert open(path).read().split("\n")[10:12] == ["%.6f %.6f %.6f 255 127 0" % tuple(pts[0]), "%.6f %.6f %.6f 254 0 255" % tuple(pts[1])]


class _StubNet:
    """What train() asks of a net, without a device: records the calls."""
    name = "stub"
    SETS = ("mlp",)

    def __init__(self):
        self.loaded, self.calls, self.training = [], 0, True
        self._p = OrderedDict(w=torch.zeros(3))

    def load_state_dict(self, sd):
        self.loaded.append(dict(sd))

    def state_dict(self):
        return OrderedDict(w=self._p["w"].clone() + self.calls)

    def train(self):
        self.training = True

    def eval(self):
        self.training = False


class _StubOptimizer:
    def __init__(self):
        self.param_groups = [dict(lr=None)]
        self.steps = 0

    def zero_grad(self):
        pass

    def step(self, grads, guard=False):
        assert guard is True
        self.steps += 1
        return self.steps != 2          # the second step is refused


def _stub_run(tmp_path, monkeypatch, argv):
    from surs_amd.apps import train_SuRS
    opt = options.BaseOptions().parse(["--checkpoints_path", str(tmp_path / "ck"), "--results_path", str(tmp_path / "res"), "--name", "n",
                                       "--no_gen_mesh", "--batch_size", "2", "--freq_plot", "1", "--gpu_id", "0"] + argv)
    net, o = _StubNet(), _StubOptimizer()

    def fb(*a, **kw):
        assert kw["encoder"] is True and set(kw) >= {"labels_lr", "labels_hr"}
        net.calls += 1
        return torch.full((2, 1, 4), 0.75), torch.tensor(0.5), torch.zeros(2, 1, 4), OrderedDict(w=torch.ones(3))
    net.forward_backward = fb
    monkeypatch.setattr(train_SuRS.optim, "from_options", lambda n, op: o)

    class Data:
        projection_mode = "orthogonal"
        is_train = True

        def __len__(self):
            return 4

        def __getitem__(self, i):
            return {"img_HR": torch.zeros(1, 3, 8, 8), "img_LR": torch.zeros(1, 3, 4, 4), "calib": torch.eye(4)[None],
                    "samples_HR": torch.full((3, 4), float(i)), "samples_LR": torch.zeros(3, 4), "labels_HR": torch.ones(1, 4),
                    "labels_disp": torch.zeros(1, 4)}
    lines = []
    done = train_SuRS.train(opt, datasets=(Data(), Data()), net=net, log=lambda *a: lines.append(" ".join(str(x) for x in a)),
                            device="cpu")
    return opt, net, o, done, lines


def test_app_option_wiring(tmp_path, monkeypatch):
    """Checkpoint names, the schedule, the skipped-step count and the PLY dumps with a stand-in net."""
    opt, net, o, done, lines = _stub_run(tmp_path, monkeypatch, ["--num_epoch", "3", "--schedule", "1", "--gamma", "0.5", "--learning_rate",
                                                                 "0.01", "--freq_save_ply", "2"])
    ck = tmp_path / "ck" / "n"
    assert sorted(os.listdir(ck)) == ["netG_epoch_0", "netG_epoch_1", "netG_epoch_2", "netG_latest"]
    assert done["first_epoch"] == 0 and done["steps"] == 6 and done["skipped"] == 1 and o.steps == 6
    assert done["lr"] == 0.005 and o.param_groups[0]["lr"] == 0.005           # halved once, at epoch 1
    assert torch.equal(torch.load(ck / "netG_latest")["w"], torch.load(ck / "netG_epoch_2")["w"])
    assert float(torch.load(ck / "netG_epoch_0")["w"][0]) == 2.0              # saved after the epoch's two steps
    assert sorted(os.listdir(tmp_path / "res" / "n")) == sorted("%d%s.ply" % (e, s) for e in range(3) for s in ("pred", "pred_gt", "pred_lr"))
    plotted = [l for l in lines if l.startswith("Name: n")]
    assert len(plotted) == 6 and "Err: 0.500000" in plotted[0] and plotted[0].endswith("skipped: 0") and plotted[-1].endswith("skipped: 1")
    assert net.loaded == [] and net.training is False                         # nothing loaded; left in eval mode, as the reference


def test_app_resume(tmp_path, monkeypatch):
    from surs_amd.apps import train_SuRS
    ck = tmp_path / "ck" / "n"
    os.makedirs(ck)
    torch.save(OrderedDict(w=torch.full((3,), 7.0)), ck / "netG_latest")
    torch.save(OrderedDict(w=torch.full((3,), 9.0)), ck / "netG_epoch_1")
    torch.save(OrderedDict(w=torch.full((3,), 5.0)), tmp_path / "init")
    # --continue_train 0 without --resume_epoch: netG_latest, from epoch 0; --load_netG_checkpoint_path is loaded first
    opt, net, _, done, _ = _stub_run(tmp_path, monkeypatch, ["--num_epoch", "1", "--continue_train", "0", "--load_netG_checkpoint_path",
                                                             str(tmp_path / "init")])
    assert [float(sd["w"][0]) for sd in net.loaded] == [5.0, 7.0] and done["first_epoch"] == 0
    # with --resume_epoch 1: that epoch's file, and the loop starts there
    opt, net, _, done, _ = _stub_run(tmp_path, monkeypatch, ["--num_epoch", "3", "--continue_train", "0", "--resume_epoch", "1"])
    assert [float(sd["w"][0]) for sd in net.loaded] == [9.0] and done["first_epoch"] == 1 and done["steps"] == 4
    assert train_SuRS.resume_plan(options.BaseOptions().parse(["--resume_epoch", "4"])) == (None, 0)    # (continue_train -1: a fresh run)


# ------------------------------------------------------------------ refusals, before anything runs
def _net(argv, projection="orthogonal"):
    return model.SuRSNet(options.BaseOptions().parse(ts.CASES["tiny"][0] + argv), projection)


def test_full_gradient_refusals():
    x = {k: torch.from_numpy(v) for k, v in ts.inputs("tiny").items()}
    args = (x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"])
    kw = dict(labels_lr=x["labels_lr"], labels_hr=x["labels_hr"], encoder=True)
    with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal"):
        _net(["--num_views", "2"]).forward_backward(*args, **kw)
    with pytest.raises(NotImplementedError, match="num_views == 1 and orthogonal"):
        _net([], "perspective").forward_backward(*args, **kw)
    with pytest.raises(NotImplementedError, match="--norm group only"):
        _net(["--norm", "batch"]).forward_backward(*args, **kw)
    with pytest.raises(RuntimeError, match="--encoder_precision f16 .* has no backward"):
        _net(["--encoder_precision", "f16"]).forward_backward(*args, **kw)
    with pytest.raises(ValueError, match="features=True goes with encoder=False"):
        _net([]).forward_backward(*args, features=True, **kw)


# ------------------------------------------------------------------ the ABI, and the fixture's promises
def test_new_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "surs.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in _lib.EXPORTS and hasattr(_lib.lib(), s), s
    assert "typedef struct SursTensorRef" in header and C.sizeof(_lib.TensorRef) == 24
    assert _lib.lib().surs_forward_losses_grad_workspace_bytes() == _lib.lib().surs_forward_losses_workspace_bytes()
    assert _lib.lib().surs_tensors_nonfinite_workspace_bytes(3) == 12


@pytest.mark.parametrize("case", list(ts.CASES))
def test_fixture_promises(case, golden_dir):
    rows = ts.load_fixture(golden_dir, case)
    assert list(rows) == [(v, s) for v in ts.VARIANTS for s in ts.SETS]
    for (variant, which), r in rows.items():
        assert r["live"] == ts.live(variant, which) and r["lr"] in ts.LADDER
        if r["live"]:
            assert abs(r["e64"][1] - r["e64"][0]) >= ts.STEP_RATIO * ts.resolution(r), (variant, which)
        else:
            assert r["e64"][0] == r["e64"][1] and r["e32"][0] == r["e32"][1]
    # the sets partition "all"
    keys = {s: ts.set_keys(case, s) for s in ts.SETS}
    assert sorted(keys["mlp"] + keys["sr"] + keys["hg"]) == sorted(keys["all"]) and len(set(keys["all"])) == len(keys["all"])
