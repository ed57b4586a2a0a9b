"""CPU-only checks of the training-sample path: the float64 restatement (tests/mesh_ref.py) against analytic shapes, the
reference's literal `in` loop against the HR-flag form the kernel uses, the OBJ parser, and data.TrainDataset's host side
(calib, colour-jitter refusal, the test phase's fixed seed, the DataLoader-worker refusal)."""
import random

import numpy as np
import pytest

import mesh_ref as mr
import train_data_common as tdc
from surs_amd import data, mesh_util


# ---------------------------------------------------------------- 1. winding number against analytic shapes
def _box_points(n, seed, lo=(-90.0, 10.0, -90.0), hi=(90.0, 190.0, 90.0)):
    """Uniform points in a box around the shapes (which sit at (0, 100, 0))."""
    return np.asarray(lo) + np.random.default_rng(seed).random((n, 3)) * (np.asarray(hi) - np.asarray(lo))


@pytest.mark.parametrize("flip", [False, True])
def test_winding_cube(flip):
    lo, hi = np.array([-40.0, 60.0, -40.0]), np.array([40.0, 140.0, 40.0])
    mesh = mr.cube(lo, hi)
    mesh = mr.flipped(mesh) if flip else mesh
    p = _box_points(400, 1)
    want = np.all((p > lo) & (p < hi), axis=1)
    w = mr.winding(p, *mesh)
    assert 20 < want.sum() < 380
    assert np.abs(w - np.where(want, -1.0 if flip else 1.0, 0.0)).max() < 1e-9
    assert (mr.contains(p, *mesh) == want).all()


@pytest.mark.parametrize("flip", [False, True])
def test_winding_ellipsoid(flip):
    radii, center = np.array([60.0, 80.0, 50.0]), np.array([0.0, 100.0, 0.0])
    mesh = mr.ellipsoid(48, 24, radii, center)
    assert mr.signed_volume(*mesh) > 0.95 * 4 / 3 * np.pi * radii.prod()
    mesh = mr.flipped(mesh) if flip else mesh
    p = _box_points(600, 2)
    t = mesh[0][mesh[1]]
    edge = max(np.linalg.norm(t[:, i] - t[:, (i + 1) % 3], axis=1).max() for i in range(3))
    p = p[mr.surface_distance(p, *mesh) >= edge]
    want = (((p - center) / radii) ** 2).sum(1) < 1
    assert len(p) > 300 and 20 < want.sum() < len(p) - 20
    w = mr.winding(p, *mesh)
    assert np.abs(w - np.where(want, -1.0 if flip else 1.0, 0.0)).max() < 1e-9
    assert (mr.contains(p, *mesh) == want).all()


def test_surface_distance_cube():
    mesh = mr.cube((0, 0, 0), (1, 1, 1))
    p = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 1.25], [2.0, 2.0, 2.0], [0.5, 0.1, 0.5], [1.5, 0.5, 1.5]])
    assert np.allclose(mr.surface_distance(p, *mesh), [0.5, 0.25, np.sqrt(3.0), 0.1, np.sqrt(0.5)], atol=1e-12)


def test_parts_mesh_is_closed_with_one_degenerate_face():
    v, f = mr.parts_mesh()
    area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    assert (area == 0).sum() == 1 and area[2000] == 0
    w = mr.winding(np.array([[60.0, 100.0, 0.0], [0.0, 100.0, 0.0], [200.0, 0.0, 0.0]]), v, f)
    assert np.abs(w - [1, 0, 0]).max() < 1e-9


# ---------------------------------------------------------------- 2. the literal `in` loop == the HR flag of the point
@pytest.mark.parametrize("regime,frac", [("more", 0.5), ("equal", None), ("less", 0.05)])
def test_in_loop_equals_hr_flag(regime, frac):
    N, P = 40, 170
    rng = np.random.default_rng(7)
    pts = rng.random((P, 3)) * 200.0
    if frac is None:
        in_lr = np.zeros(P, bool)
        in_lr[rng.permutation(P)[:N // 2]] = True
    else:
        in_lr = rng.random(P) < frac
    in_hr = in_lr ^ (rng.random(P) < 0.3)
    nin = int(in_lr.sum())
    assert {"more": nin > N // 2, "equal": nin == N // 2, "less": 0 < nin < N // 2}[regime]
    a, b = mr.select(pts, in_hr, in_lr, N, literal=True), mr.select(pts, in_hr, in_lr, N, literal=False)
    for k in ("samples_HR", "samples_LR", "labels_HR", "labels_disp"):
        assert np.array_equal(a[k], b[k]), k
    assert a["labels_disp"].shape == (1, N) and a["samples_LR"].shape == (3, N)
    assert 0 < a["labels_disp"].sum() < N and not np.array_equal(a["labels_disp"][0], np.r_[np.ones(N // 2), np.zeros(N // 2)])


# ---------------------------------------------------------------- 3. OBJ parser
def test_load_obj_mesh_forms(tmp_path):
    path = tmp_path / "m.obj"
    path.write_text("# comment\nvn 0 0 1\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nv 0 1 0\nvt 0 0\n"
                    "f 1/1/1 2/1/1 3/1/1 4/1/1\nf 1//1 2//1 3//1\nf 1/1 3/1 4/1\nv 0 0 1\nf -1 -5 -4\nf 1 2 3 4 5\n")
    v, f = mesh_util.load_obj_mesh(str(path))
    assert v.shape == (5, 3) and v.dtype == np.float64 and f.dtype == np.int32
    assert np.array_equal(v[1], [1, 0, 0]) and np.array_equal(v[4], [0, 0, 1])
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    for bad in ("v 0 0 0\nf 1 2 3\n", "v 0 0 0\nf 1 1\n", "v 0 0 0\nf 0 1 1\n", "v 0 0 0\nf -2 1 1\n"):
        path.write_text(bad)
        with pytest.raises(ValueError):
            mesh_util.load_obj_mesh(str(path))


def test_load_obj_mesh_round_trip(tmp_path):
    """save_obj_mesh writes %.4f coordinates and the faces as (f0, f2, f1): the parser returns exactly that."""
    v, f = mr.torus(8, 6)
    path = str(tmp_path / "t.obj")
    mesh_util.save_obj_mesh(path, v, f)
    v2, f2 = mesh_util.load_obj_mesh(path)
    assert np.array_equal(f2, f[:, [0, 2, 1]])
    assert np.array_equal(v2, np.array([[float("%.4f" % x) for x in p] for p in v]))


# ---------------------------------------------------------------- 4. get_render's calib
def _calib_ref(param, load_size, flip=False, rand_scale=None, dx=0, dy=0):
    """Lines 242-316 of the reference in numpy."""
    R, center, scale, ortho_ratio = param["R"], param["center"], param["scale"], param["ortho_ratio"]
    translate = -np.matmul(R, center).reshape(3, 1)
    extrinsic = np.concatenate([R, translate], axis=1)
    extrinsic = np.concatenate([extrinsic, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
    scale_intrinsic = np.identity(4)
    scale_intrinsic[0, 0] = scale / ortho_ratio
    scale_intrinsic[1, 1] = -scale / ortho_ratio
    scale_intrinsic[2, 2] = scale / ortho_ratio
    uv_intrinsic = np.identity(4)
    uv_intrinsic[0, 0] = 1.0 / float(load_size // 2)
    uv_intrinsic[1, 1] = 1.0 / float(load_size // 2)
    uv_intrinsic[2, 2] = 1.0 / float(load_size // 2)
    trans_intrinsic = np.identity(4)
    if flip:
        scale_intrinsic[0, 0] *= -1
    if rand_scale is not None:
        scale_intrinsic *= rand_scale
        scale_intrinsic[3, 3] = 1
    trans_intrinsic[0, 3] = -dx / float(load_size // 2)
    trans_intrinsic[1, 3] = -dy / float(load_size // 2)
    intrinsic = np.matmul(trans_intrinsic, np.matmul(uv_intrinsic, scale_intrinsic))
    return np.matmul(intrinsic, extrinsic).astype(np.float32), extrinsic.astype(np.float32)


@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    return tdc.make_dataroot(tmp_path_factory.mktemp("train_root"), mr.torus(8, 6), mr.torus(6, 4), size=64)


def _render(ds):
    return ds.get_render("alpha", num_views=1)


def test_get_render_plain(dataroot):
    ds = data.TrainDataset(tdc.opt(dataroot), "train")
    assert ds.subjects == ["alpha"] and len(ds) == 360
    assert data.TrainDataset(tdc.opt(dataroot), "test").subjects == ["beta"]
    r = _render(ds)
    calib, extrinsic = _calib_ref(tdc.PARAM, 64)
    assert np.array_equal(r["calib"][0].numpy(), calib) and np.array_equal(r["extrinsic"][0].numpy(), extrinsic)
    assert tuple(r["img_HR"].shape) == (1, 3, 64, 64) and tuple(r["img_LR"].shape) == (1, 3, 32, 32)
    assert r["img_HR"].dtype == r["img_LR"].dtype == r["calib"].dtype
    # pad by 6, centre crop back: the image itself, masked; Normalize maps 0..255 to -1..1
    from PIL import Image
    import os
    rgb = np.asarray(Image.open(os.path.join(dataroot, "RENDER", "alpha", "0_0_00.png")), np.float32).transpose(2, 0, 1) / np.float32(255)
    mask = np.asarray(Image.open(os.path.join(dataroot, "MASK", "alpha", "0_0_00.png")), np.float32)[None] / np.float32(255)
    assert np.array_equal(r["img_HR"][0].numpy(), mask * ((rgb - np.float32(0.5)) / np.float32(0.5)))
    # the half-size pair: the mask's edges are multiples of 8, so NEAREST gives rows 4 .. 28, columns 8 .. 24 whichever pixel it takes
    lr = r["img_LR"][0].numpy()
    inside = np.zeros((32, 32), bool)
    inside[4:28, 8:24] = True
    assert (lr[:, ~inside] == 0).all() and (np.abs(lr[:, inside]) > 0).mean() > 0.9 and np.abs(lr).max() <= 1


def test_get_render_flip(dataroot, monkeypatch):
    plain = _render(data.TrainDataset(tdc.opt(dataroot), "train"))
    ds = data.TrainDataset(tdc.opt(dataroot, more=["--random_flip"]), "train")
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.9)
    r = _render(ds)
    assert np.array_equal(r["calib"][0].numpy(), _calib_ref(tdc.PARAM, 64, flip=True)[0])
    assert np.array_equal(r["img_HR"].numpy(), plain["img_HR"].numpy()[..., ::-1])
    monkeypatch.setattr(np.random, "rand", lambda *a: 0.1)
    assert np.array_equal(_render(ds)["calib"].numpy(), plain["calib"].numpy())


def test_get_render_scale_and_translation(dataroot, monkeypatch):
    ds = data.TrainDataset(tdc.opt(dataroot, more=["--random_scale", "--random_trans"]), "train")
    monkeypatch.setattr(random, "uniform", lambda a, b: 1.25 if (a, b) == (0.9, 1.1) else None)
    bounds = []
    monkeypatch.setattr(random, "randint", lambda a, b: (bounds.append((a, b)), b)[1])
    r = _render(ds)
    # padded 76 x 76, scaled to int(1.25 * 76) = 95: dx = dy = int(round((95 - 64) / 10)) = 3
    assert bounds == [(-3, 3), (-3, 3)]
    assert np.array_equal(r["calib"][0].numpy(), _calib_ref(tdc.PARAM, 64, rand_scale=1.25, dx=3, dy=3)[0])
    assert tuple(r["img_HR"].shape) == (1, 3, 64, 64)


def test_test_phase_has_no_augmentation(dataroot, monkeypatch):
    ds = data.TrainDataset(tdc.opt(dataroot, more=["--random_flip", "--random_scale", "--random_trans", "--aug_blur", "2"]), "test")
    monkeypatch.setattr(np.random, "rand", lambda *a: pytest.fail("the test phase draws nothing"))
    r = ds.get_render("beta", num_views=1)
    assert np.array_equal(r["calib"][0].numpy(), _calib_ref(tdc.PARAM, 64)[0])


# ---------------------------------------------------------------- 5. colour jitter is refused
@pytest.mark.parametrize("flag", ["aug_bri", "aug_con", "aug_sat", "aug_hue"])
def test_colour_jitter_refused(dataroot, flag):
    with pytest.raises(NotImplementedError, match="--" + flag):
        data.TrainDataset(tdc.opt(dataroot, more=["--" + flag, "0.2"]), "train")
    data.TrainDataset(tdc.opt(dataroot, more=["--" + flag, "0"]), "train")


# ---------------------------------------------------------------- 6. the test phase is deterministic; workers are refused
def test_item_seeds(dataroot):
    test = data.TrainDataset(tdc.opt(dataroot), "test", seed=5)
    assert [test.item_seed(i) for i in (0, 1, 7)] == [1991] * 3
    test.draws += 3
    assert test.item_seed(0) == 1991
    a, b = test.get_render("beta", num_views=1), test.get_render("beta", num_views=1)
    assert all(np.array_equal(a[k].numpy(), b[k].numpy()) for k in a)
    train = data.TrainDataset(tdc.opt(dataroot), "train", seed=5)
    s = [train.item_seed(0), train.item_seed(1)]
    train.draws += 1
    s += [train.item_seed(0), data.TrainDataset(tdc.opt(dataroot), "train", seed=6).item_seed(0)]
    assert len(set(s)) == 4 and all(0 <= x < 2 ** 63 for x in s)
    assert data.TrainDataset(tdc.opt(dataroot), "train", seed=5).item_seed(0) == s[0]


def test_refuses_dataloader_worker(dataroot, monkeypatch):
    import torch.utils.data
    ds = data.TrainDataset(tdc.opt(dataroot), "train")
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="--num_threads 0"):
        ds[0]
    with pytest.raises(RuntimeError, match="--num_threads 0"):
        ds.select_sampling_method(("alpha", ""))
    assert ds._meshes == {}      # nothing was parsed or uploaded


def test_bits64_is_what_uniform01_reads():
    from surs_amd import prng
    b = prng.bits64("some_stream", 3, 1000)
    assert b.dtype == np.uint64 and len(np.unique(b)) == 1000
    assert np.array_equal((b >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24), prng.uniform01("some_stream", 3, 1000))
