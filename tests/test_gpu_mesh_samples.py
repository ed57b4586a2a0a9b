"""GPU checks of the training-sample kernels (csrc/surs_mesh_sample.hip) against the float64 restatement tests/mesh_ref.py:
contains (flags and winding numbers, determinism, batch independence), the area cdf, the pool (faces, points, jitter, box,
shuffle), the selection (bit for bit) and data.TrainDataset end to end, down to one SuRSNet.forward on an item.

Bounds.  A flag is compared where the point's float64 distance to the surface is at least mesh_ref.MARGIN = 2^-24 * 128 * 64
(about 5e-4); at most 1 % of a test's points may fall below it (with seed 11 the restatement alone finds none below 6e-3).
|w32 - w64| <= 1e-3 on the compared points (decision margin 0.5).  Measured on an MI355X: see NOTES.md "Training samples"."""
import numpy as np
import pytest
import torch

import mesh_ref as mr

pytestmark = pytest.mark.gpu

SEED, NPTS = 11, 1000
SHAPES = {"tetrahedron": mr.tetrahedron, "cube": mr.cube, "torus": mr.torus, "parts": mr.parts_mesh}
_ref, _dev_mesh = {}, {}


def _mesh(shape, flip=False):
    if (shape, flip) not in _ref:
        if flip:
            base = _mesh(shape)
            _ref[(shape, True)] = dict(base, mesh=mr.flipped(base["mesh"]), w=mr.winding(base["points"], *mr.flipped(base["mesh"])))
        else:
            mesh = SHAPES[shape]()
            pts = mr.contains_points(mesh, NPTS, SEED)
            _ref[(shape, False)] = dict(mesh=mesh, points=pts, w=mr.winding(pts, *mesh), dist=mr.surface_distance(pts, *mesh))
    return _ref[(shape, flip)]


def _native_mesh(key, mesh):
    from surs_amd import native
    if key not in _dev_mesh:
        _dev_mesh[key] = native.Mesh(mesh[0], mesh[1])
    return _dev_mesh[key]


def _upload(points, ld):
    """[n,3] numpy -> a device tensor view with row pitch ld (the padding holds NaN: reading it would show)."""
    import gpu_common as g
    buf = torch.full((len(points), ld), float("nan"), dtype=torch.float32, device=g.dev())
    buf[:, :3] = torch.from_numpy(np.ascontiguousarray(points, np.float32)).to(g.dev())
    return buf[:, :3] if ld > 3 else buf


# ---------------------------------------------------------------- contains
@pytest.mark.parametrize("ld", [3, 5])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_contains_matches_float64(shape, flip, ld):
    from surs_amd import native
    ref = _mesh(shape, flip)
    if shape == "parts":
        assert len(ref["mesh"][1]) == 2 * mr.FACES_PER_PART + 7 and native.mesh_contains_parts(len(ref["mesh"][1])) == 3
    m = _native_mesh((shape, flip), ref["mesh"])
    compared = ref["dist"] >= mr.MARGIN
    skipped = 1.0 - compared.mean()
    assert skipped <= 0.01, "the margin rule skips %.2f %% of the points" % (100 * skipped)
    want = np.abs(ref["w"]) > 0.5
    assert 0.2 < want.mean() < 0.8
    worst = 0.0
    for n in (1, 63, 64, 65, 1000):
        inside, w = native.mesh_contains(_upload(ref["points"][:n], ld), m, want_winding=True)
        inside, w = inside.cpu().numpy(), w.cpu().numpy()
        assert inside.shape == (n,) and inside.dtype == np.uint8 and np.isfinite(w).all()
        c = compared[:n]
        assert np.array_equal(inside[c] != 0, want[:n][c]), n
        assert np.array_equal(inside != 0, np.abs(w) > 0.5)
        worst = max(worst, float(np.abs(w.astype(np.float64) - ref["w"][:n])[c].max()) if c.any() else 0.0)
    print("contains %s flip=%d ld=%d: worst |w32 - w64| = %.3g, skipped %.2f %%" % (shape, flip, ld, worst, 100 * skipped))
    assert worst <= 1e-3
    if flip:
        assert (ref["w"][want] < -0.5).all()      # the inward-oriented mesh: winding -1 inside, and still 'inside'


@pytest.mark.parametrize("shape", ["torus", "parts"])
def test_contains_same_bits_in_any_batch(shape):
    from surs_amd import native
    ref = _mesh(shape)
    m = _native_mesh((shape, False), ref["mesh"])
    pts = _upload(ref["points"], 3)
    a = native.mesh_contains(pts, m, want_winding=True)
    b = native.mesh_contains(pts, m, want_winding=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    w, f = [], []
    for lo, hi in ((0, 1), (1, 64), (64, 1000)):      # calls of 1, 63 and 936 points
        fi, wi = native.mesh_contains(pts[lo:hi], m, want_winding=True)
        w.append(wi)
        f.append(fi)
    assert torch.equal(torch.cat(w).view(torch.int32), a[1].view(torch.int32)) and torch.equal(torch.cat(f), a[0])


def test_contains_point_on_a_vertex_is_finite():
    from surs_amd import native
    for shape in ("cube", "parts"):
        ref = _mesh(shape)
        m = _native_mesh((shape, False), ref["mesh"])
        v = ref["mesh"][0]
        pts = np.concatenate([v[:40], 0.5 * (v[ref["mesh"][1][:8, 0]] + v[ref["mesh"][1][:8, 1]])]).astype(np.float32)
        inside, w = native.mesh_contains(_upload(pts, 3), m, want_winding=True)
        assert torch.isfinite(w).all() and float(w.abs().max()) < 1.5
    assert native.mesh_contains(_upload(np.zeros((0, 3)), 3), m).shape == (0,)


# ---------------------------------------------------------------- area cdf
@pytest.mark.parametrize("shape", list(SHAPES) + ["two_faces"])
def test_area_cdf(shape):
    mesh = mr.two_faces() if shape == "two_faces" else _mesh(shape)["mesh"]
    cdf = _native_mesh((shape, False), mesh).cdf.cpu().numpy()
    want = mr.area_cdf(*mesh)
    assert cdf.dtype == np.float64 and cdf.shape == want.shape
    assert np.abs(cdf - want).max() <= 1e-12 * want[-1] and np.all(np.abs(cdf - want) <= 1e-12 * want)
    assert (np.diff(cdf) >= 0).all() and cdf[0] > 0


# ---------------------------------------------------------------- pool
def test_pool_matches_restatement():
    from surs_amd import native
    mesh = mr.two_faces()
    m = _native_mesh(("two_faces", False), mesh)
    ns, nb, sigma, seed = 4000, 250, 5.0, 3
    ref = mr.pool(mesh[0], mesh[1], seed, ns, nb, sigma)
    p0, _, face = native.mesh_sample_pool(m, ns, nb, 0.0, mr.B_MIN, mr.B_MAX, seed, want_faces=True, shuffle=False)
    p5, _ = native.mesh_sample_pool(m, ns, nb, sigma, mr.B_MIN, mr.B_MAX, seed, shuffle=False)
    ps, order = native.mesh_sample_pool(m, ns, nb, sigma, mr.B_MIN, mr.B_MAX, seed)
    p0, p5, ps, face, order = (x.cpu().numpy() for x in (p0, p5, ps, face, order))
    # the face: cdf_ref[f - 1] - tol <= u total <= cdf_ref[f] + tol; the 1000 : 1 areas show in the counts
    tol = 1e-9 * ref["total"]
    below = np.where(face > 0, ref["cdf"][np.maximum(face - 1, 0)], 0.0)
    assert face.min() >= 0 and face.max() <= 1
    assert (below - tol <= ref["target"]).all() and (ref["target"] <= ref["cdf"][face] + tol).all()
    assert np.array_equal(face, ref["face"]) and 0 < (face == 1).sum() < 20
    # the un-jittered point on that face
    assert np.abs(p0[:ns].astype(np.float64) - ref["base"]).max() <= 1e-4
    assert np.abs(p0[:ns, 2]).max() == 0 and (p0[:ns, :2] >= 0).all()
    # jitter: what sigma adds, against float64 Box-Muller on the same uniforms
    jitter = p5[:ns].astype(np.float64) - p0[:ns].astype(np.float64)
    err = np.abs(jitter - ref["jitter"]).max()
    print("pool: worst jitter error %.3g (bound %.3g), largest |z| %.3f" % (err, 1e-5 * sigma, np.abs(ref["jitter"]).max() / sigma))
    assert err <= 1e-5 * sigma and np.abs(ref["jitter"]).max() > 3 * sigma
    # box points within 1 ulp, the same with and without sigma
    box = ref["box"].astype(np.float32)
    assert (np.abs(p5[ns:] - box) <= np.spacing(np.abs(box))).all() and np.array_equal(p5[ns:], p0[ns:])
    assert ((p5[ns:] >= mr.B_MIN) & (p5[ns:] < mr.B_MAX)).all()
    # the shuffle: exactly the restatement's order
    assert np.array_equal(order, ref["order"]) and np.array_equal(ps, p5[ref["order"]])
    again, _ = native.mesh_sample_pool(m, ns, nb, sigma, mr.B_MIN, mr.B_MAX, seed)
    other, _ = native.mesh_sample_pool(m, ns, nb, sigma, mr.B_MIN, mr.B_MAX, seed + 1)
    assert np.array_equal(again.cpu().numpy(), ps) and not np.array_equal(other.cpu().numpy(), ps)


# ---------------------------------------------------------------- select
def _crafted(P):
    """P points with pairwise distinct coordinates (so that the literal `in` loop means 'the same point'), exact in fp32."""
    i = np.arange(P, dtype=np.float64)
    return np.stack([i + 0.25, 5000.0 + 2 * i, -7000.0 - 3 * i + 0.5], 1)


def _flags(P, nin, seed):
    f = np.zeros(P, bool)
    f[np.random.default_rng(seed).permutation(P)[:nin]] = True
    return f


def _check_select(pts, in_hr, in_lr, N, ld=3):
    import gpu_common as g
    from surs_amd import native
    ref = mr.select(pts, in_hr, in_lr, N, literal=True)
    up = lambda f: torch.from_numpy(f.astype(np.uint8)).to(g.dev())
    s_hr, l_hr, s_lr, l_disp, counts = native.sample_select(_upload(pts, ld), up(in_hr), up(in_lr), N)
    assert tuple(s_hr.shape) == (3, N) and tuple(s_lr.shape) == (3, N) and tuple(l_hr.shape) == (1, N) and tuple(l_disp.shape) == (1, N)
    s_hr, l_hr, s_lr, l_disp, counts = (x.cpu().numpy() for x in (s_hr, l_hr, s_lr, l_disp, counts))
    assert tuple(counts) == ref["counts"]
    k_hr, k_lr = counts[0] + counts[1], counts[2] + counts[3]
    assert np.array_equal(s_hr[:, :k_hr], ref["samples_HR"].astype(np.float32)) and (s_hr[:, k_hr:] == 0).all()
    assert np.array_equal(s_lr[:, :k_lr], ref["samples_LR"].astype(np.float32)) and (s_lr[:, k_lr:] == 0).all()
    assert np.array_equal(l_hr[:, :k_hr], ref["labels_HR"].astype(np.float32)) and (l_hr[:, k_hr:] == 0).all()
    assert np.array_equal(l_disp, ref["labels_disp"].astype(np.float32))
    return ref


@pytest.mark.parametrize("nin_lr", [0, 20, 32, 150, 272])
def test_select_regimes(nin_lr):
    """N = 64, pool = 4 N + N / 4 = 272: nin = 0, < N / 2, == N / 2, > N / 2, all inside - for the LR flags, the HR flags
    walking through the same regimes one step ahead."""
    N, P = 64, 272
    regimes = [0, 20, 32, 150, 272]
    nin_hr = regimes[(regimes.index(nin_lr) + 1) % len(regimes)]
    pts = _crafted(P)
    in_lr = _flags(P, nin_lr, 1)
    in_hr = _flags(P, nin_hr, 2)
    ref = _check_select(pts, in_hr, in_lr, N)
    assert ref["counts"][2] == min(nin_lr, N // 2)
    # flags that mostly agree (the training case): labels_disp mostly equals its default, not entirely
    if 0 < nin_lr < P:
        near = in_lr ^ (np.random.default_rng(3).random(P) < 0.1)
        _check_select(pts, near, in_lr, N)
        _check_select(pts, in_lr, in_lr, N)


@pytest.mark.parametrize("ld", [3, 4])
def test_select_pool_of_one_chunk_plus_one(ld):
    P, N = mr.SELECT_CHUNK + 1, 240
    pts = _crafted(P)
    rng = np.random.default_rng(5)
    in_lr = rng.random(P) < 0.4
    in_hr = in_lr ^ (rng.random(P) < 0.2)
    in_lr[-1] = in_hr[-1] = True
    _check_select(pts, in_hr, in_lr, N, ld)
    # the entry behind the chunk decides: it is the only inside point
    only = np.zeros(P, bool)
    only[-1] = True
    ref = _check_select(pts, only, only, N, ld)
    assert ref["counts"] == (1, N - 1, 1, N - 1) and np.array_equal(ref["samples_LR"][:, 0], pts[-1])


# ---------------------------------------------------------------- end to end
def test_train_dataset_end_to_end(tmp_path):
    import common
    import gpu_common as g
    import train_data_common as tdc
    from surs_amd import data, model, native, options, weights
    N, size = 256, 128       # a 64 x 64 low-resolution image
    hr, lr = mr.torus(96, 48), mr.torus(24, 12)
    # calib maps the default box onto [-1, 1]^3: scale / ortho_ratio / (loadSize / 2) = 1 / 128 around the box's centre
    param = dict(ortho_ratio=1.0, scale=0.5, center=np.array([0.0, 100.0, 0.0]), R=np.eye(3))
    root = tdc.make_dataroot(tmp_path, hr, lr, size=size, param=param)
    ds = data.TrainDataset(tdc.opt(root, size=size, n=N), "test")
    item = ds[0]
    assert item["name"] == ("beta", "") and item["mesh_path_HR"].endswith("beta_HR.obj")
    for k, shape in (("samples_HR", (3, N)), ("samples_LR", (3, N)), ("labels_HR", (1, N)), ("labels_disp", (1, N))):
        assert item[k].is_cuda and item[k].dtype == torch.float32 and tuple(item[k].shape) == shape, k
    assert tuple(item["img_LR"].shape) == (1, 3, 64, 64) and tuple(item["img_HR"].shape) == (1, 3, 128, 128) and not item["img_LR"].is_cuda
    assert sorted(ds._meshes) == ["beta_HR.obj", "beta_LR.obj"]
    meshes = dict(ds._meshes)
    again = ds[0]      # the test phase: seed 1991 every time, and the meshes are not loaded again
    assert all(torch.equal(item[k], again[k]) for k in ("samples_HR", "samples_LR", "labels_HR", "labels_disp"))
    assert all(ds._meshes[k] is meshes[k] for k in meshes)

    s_hr, s_lr = item["samples_HR"].cpu().numpy().T.astype(np.float64), item["samples_LR"].cpu().numpy().T.astype(np.float64)
    l_hr, l_disp = item["labels_HR"].cpu().numpy()[0], item["labels_disp"].cpu().numpy()[0]
    # labels_HR: the restatement's contains on the returned points (same margin rule); N / 2 of each, inside first
    ok = mr.surface_distance(s_hr, *hr) >= mr.MARGIN
    assert ok.mean() >= 0.99 and np.array_equal(l_hr[ok] != 0, mr.contains(s_hr, *hr)[ok])
    assert np.array_equal(l_hr, np.r_[np.ones(N // 2), np.zeros(N // 2)])
    # labels_disp: the entries the loop overwrites hold the HR flag of samples_LR
    L = int(native.mesh_contains(item["samples_LR"].t().contiguous(), ds._meshes["beta_LR.obj"]).sum())
    assert L == N // 2
    ok = mr.surface_distance(s_lr, *hr) >= mr.MARGIN
    flag = mr.contains(s_lr, *hr)
    assert ok.mean() >= 0.99 and np.array_equal(l_disp[ok] != 0, flag[ok])
    assert 0 < (l_disp != np.r_[np.ones(N // 2), np.zeros(N // 2)]).sum() < N // 4      # the two tori differ a little
    # a train-phase dataset draws other samples each time
    tr = data.TrainDataset(tdc.opt(root, size=size, n=N), "train", seed=3)
    a, b = tr.select_sampling_method(("alpha", ""), 0), tr.select_sampling_method(("alpha", ""), 0)
    assert not torch.equal(a["samples_HR"], b["samples_HR"]) and not torch.equal(a["samples_HR"], item["samples_HR"])

    # one validation forward on the item
    opt = options.BaseOptions().parse(common.FLAGS)
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict(weights.synthetic_state_dict(opt, seed=0))
    net.eval()
    dev = g.dev()
    res_hr, error, res_lr = net.forward(item["img_LR"].to(dev), item["img_HR"].to(dev), item["samples_LR"][None], item["samples_HR"][None],
                                        item["calib"].to(dev), labels_lr=item["labels_disp"][None], labels_hr=item["labels_HR"][None])
    assert error.is_cuda and bool(torch.isfinite(error)) and float(error) > 0
    assert bool(torch.isfinite(res_hr).all()) and bool(torch.isfinite(res_lr).all())
