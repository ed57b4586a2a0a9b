"""GPU checks of the mesh distance kernel (csrc/surs_mesh_distance.hip) and of the scores built on it (metrics.py,
train_util.gen_mesh_metrics).  The kernel is held to surs_mesh_distance_host BIT FOR BIT - the same header looped on the host, which
tests/test_mesh_distance_host.py holds to the float64 yardstick within B = 2^-24 * 16 * S (mesh_dist_ref.bound) - and its results
may not depend on the batch a point arrives in.  The scores are compared with their float64 restatement on the GPU's own samples:
every distance figure within B, normal_consistency within 2^-20 (sr_grad_common.FLOOR)."""
import numpy as np
import pytest
import torch

import mesh_dist_ref as md
import mesh_ref as mr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
_dev_mesh = {}


def _native_mesh(key, mesh):
    from surs_amd import native
    if key not in _dev_mesh:
        _dev_mesh[key] = native.Mesh(mesh[0], mesh[1])
    return _dev_mesh[key]


def _upload(points, ld=3):
    """[n,3] numpy -> a device tensor view with row pitch ld (the padding holds NaN: reading it would show)."""
    import gpu_common as g
    buf = torch.full((len(points), ld), float("nan"), dtype=torch.float32, device=g.dev())
    buf[:, :3] = torch.from_numpy(np.array(points, np.float32)).to(g.dev())
    return buf[:, :3] if ld > 3 else buf


def _device(points, mesh, ld=3):
    from surs_amd import native
    dist, face = native.mesh_distance(_upload(points, ld), mesh, want_face=True)
    assert dist.dtype == torch.float32 and face.dtype == torch.int32 and dist.shape == face.shape == (len(points),)
    return dist.cpu().numpy(), face.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 8. the kernel is the host loop, bit for bit
@pytest.mark.parametrize("name", list(md.MESHES))
def test_kernel_equals_host_bit_for_bit(name):
    from surs_amd import native
    c = md.case(name)
    want = native.mesh_distance_host(c["points"], c["v"], c["f"])
    got = _device(c["points"], _native_mesh(name, (c["v"], c["f"])))
    diff = np.abs(got[0].astype(np.float64) - want[0])
    print("%s: %d points x %d faces, max |device - host| %.3e, faces differing %d" % (name, len(c["points"]), len(c["f"]), diff.max(),
                                                                                    int((got[1] != want[1]).sum())))
    assert _same_bits(got, want)
    assert (got[0][c["vertices"]] == 0).all()
    only_dist = native.mesh_distance(_upload(c["points"]), _native_mesh(name, (c["v"], c["f"])))      # face is nullable
    assert np.array_equal(only_dist.cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def test_kernel_ties_and_duplicate_face():
    from surs_amd import native
    v, f = mr.cube()
    p = (0.5 * (v[0] + v[3]))[None].astype(np.float32)
    dist, face = _device(p, _native_mesh("cube", (v, f)))
    assert dist[0] == 0 and face[0] == 0
    swapped = np.concatenate([f[1:2], f[0:1], f[2:]], 0)
    assert _device(p, native.Mesh(v, swapped))[1][0] == 0
    vd, fd = md.parts_with_duplicate()
    c = md.case("parts")
    got = _device(c["points"], native.Mesh(vd, fd))
    assert got[1].max() < 8199 and (got[1] == 10).sum() > 0
    assert _same_bits(got, native.mesh_distance_host(c["points"], vd, fd))


def test_kernel_non_finite_points_and_no_points():
    import gpu_common as g
    from surs_amd import native
    c = md.case("parts")
    m = _native_mesh("parts", (c["v"], c["f"]))
    p = np.array([[np.nan, 100, 0], [0, np.inf, 0], [0, 100, -np.inf], [1, 2, 3]], np.float32)
    dist, face = _device(p, m)
    assert np.array_equal(dist[:3], [np.inf] * 3) and np.array_equal(face[:3], [-1] * 3) and np.isfinite(dist[3]) and face[3] >= 0
    dist, face = native.mesh_distance(torch.empty((0, 3), dtype=torch.float32, device=g.dev()), m, want_face=True)
    assert dist.shape == (0,) and face.shape == (0,)


# ---------------------------------------------------------------- 9. batch independence
@pytest.mark.parametrize("ld", [3, 4, 7])
def test_batch_independence(ld):
    c = md.case("parts")
    pts = c["points"][:md.N_POINTS]
    m = _native_mesh("parts", (c["v"], c["f"]))
    whole = _device(pts, m)
    start = 0
    for rows in (1, 5, 255, 256, 257):
        part = _device(pts[start:start + rows], m, ld)
        assert _same_bits(part, (whole[0][start:start + rows], whole[1][start:start + rows])), (rows, start)
        start += rows
    assert start + 287 == md.N_POINTS
    for off, rows in ((0, 1024 + 37), (md.N_POINTS - 287, 287), (3, 1024)):
        part = _device(pts[off:off + rows], m, ld)
        assert _same_bits(part, (whole[0][off:off + rows], whole[1][off:off + rows])), (off, rows)


def test_same_bits_from_another_workspace():
    import gpu_common as g
    from surs_amd import _lib, native
    c = md.case("parts")
    pts = _upload(c["points"][:md.N_POINTS])
    m = _native_mesh("parts", (c["v"], c["f"]))
    n = pts.shape[0]
    need = _lib.lib().surs_mesh_distance_workspace_bytes(n, m.nf)
    assert need == 3 * n * 8
    ws = [torch.full((need,), 0xFF, dtype=torch.uint8, device=g.dev()), torch.zeros(need + 4096, dtype=torch.uint8, device=g.dev())]
    outs = []
    for w, offset in ((ws[0], 0), (ws[1], 2048), (ws[0], 0)):
        dist = torch.empty(n, dtype=torch.float32, device=g.dev())
        face = torch.empty(n, dtype=torch.int32, device=g.dev())
        native.check(_lib.lib().surs_mesh_distance(native._ptr(pts), n, 3, native._ptr(m.verts), m.nv, native._ptr(m.faces), m.nf,
                                                   w.data_ptr() + offset, need, native._ptr(dist), native._ptr(face), native._stream()))
        outs.append((dist.cpu().numpy(), face.cpu().numpy()))
    assert ws[0].data_ptr() != ws[1].data_ptr() + 2048
    assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2])
    assert _same_bits(outs[0], _device(c["points"][:md.N_POINTS], m))


# ---------------------------------------------------------------- 10. surface samples
def test_surface_samples():
    from surs_amd import metrics, native
    c = md.case("parts")
    m = _native_mesh("parts", (c["v"], c["f"]))
    pts, face = metrics.surface_samples(m, md.N_POINTS, seed=5)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (md.N_POINTS, 3) and face.dtype == torch.int32
    pool, order, pool_face = native.mesh_sample_pool(m, md.N_POINTS, 0, 0.0, mr.B_MIN, mr.B_MAX, 5, want_faces=True, shuffle=False)
    assert order is None and torch.equal(face, pool_face) and torch.equal(pts, pool)
    p = pts.cpu().numpy()
    d = md.distance_to_face(p, c["v"], c["f"], face.cpu().numpy())
    B = md.bound(c["v"], p)
    print("surface samples: at most %.3e off their face (B %.3e)" % (d.max(), B))
    assert d.max() <= B
    again = metrics.surface_samples(m, md.N_POINTS, seed=5)
    assert torch.equal(again[0], pts) and not torch.equal(metrics.surface_samples(m, md.N_POINTS, seed=6)[0], pts)


def test_face_normals():
    from surs_amd import metrics
    c = md.case("parts")
    n = metrics.face_normals(_native_mesh("parts", (c["v"], c["f"]))).cpu().numpy()
    want = md.unit_normals(c["v"], c["f"])
    assert n.shape == (len(c["f"]), 3) and np.abs(n - want).max() < 1e-12
    assert (n[2000] == 0).all() and np.abs(np.linalg.norm(np.delete(n, 2000, 0), axis=1) - 1).max() < 1e-12


# ---------------------------------------------------------------- 11. the scores
def _shifted(mesh, by):
    return mr._f32(mesh[0] + np.asarray(by, float)), mesh[1]


def _samples(src, dst, n, seed):
    """What mesh_metrics draws and measures for one direction, downloaded: (points, source face, reported face)."""
    from surs_amd import metrics, native
    pts, face = metrics.surface_samples(src, n, seed)
    _, near = native.mesh_distance(pts, dst, want_face=True)
    return pts.cpu().numpy(), face.cpu().numpy(), near.cpu().numpy()


@pytest.mark.parametrize("pair", ["torus_shifted", "ellipsoid_torus"])
def test_mesh_metrics_against_float64(pair):
    from surs_amd import metrics, native
    pred, gt = {"torus_shifted": (mr.torus(), _shifted(mr.torus(), (3, 0, 0))), "ellipsoid_torus": (mr.ellipsoid(), mr.torus())}[pair]
    mp, mg = native.Mesh(*pred), native.Mesh(*gt)
    n, seed = md.N_POINTS, 3
    got = metrics.mesh_metrics(mp, mg, n=n, seed=seed)
    assert got["n"] == n and all(isinstance(got[k], float) for k in got if k != "n")
    want = md.restate_metrics(pred, gt, _samples(mp, mg, n, seed), _samples(mg, mp, n, seed))
    B = md.bound(pred[0], gt[0])
    for k in ("p2s", "gt2pred", "chamfer", "max_p2s", "max_gt2pred"):
        print("%s %s: %.7f against %.7f (%.3e, B %.3e)" % (pair, k, got[k], want[k], abs(got[k] - want[k]), B))
        assert abs(got[k] - want[k]) <= B, k
    print("%s normal_consistency: %.8f against %.8f" % (pair, got["normal_consistency"], want["normal_consistency"]))
    assert abs(got["normal_consistency"] - want["normal_consistency"]) <= FLOOR
    assert got["p2s"] > 1 and got["chamfer"] == 0.5 * (got["p2s"] + got["gt2pred"]) and got["max_p2s"] >= got["p2s"]
    assert metrics.mesh_metrics(pred, gt, n=n, seed=seed) == got                      # (verts, faces) pairs are uploaded; same bits


def test_mesh_metrics_concentric_cubes():
    from surs_amd import metrics
    inner, outer = mr.cube(), mr.cube((-50.0, 50.0, -50.0), (50.0, 150.0, 50.0))
    got = metrics.mesh_metrics(inner, outer, n=md.N_POINTS)
    B = md.bound(inner[0], outer[0])
    print("cubes: p2s %.7f, max %.7f (B %.3e)" % (got["p2s"], got["max_p2s"], B))
    assert abs(got["p2s"] - 10.0) <= B and abs(got["max_p2s"] - 10.0) <= B
    # the outer cube's samples near its edges are nearest to an EDGE of the inner one, whichever of its two faces reports it
    assert got["gt2pred"] > 10.0 and 0.5 < got["normal_consistency"] <= 1.0


def test_mesh_metrics_of_a_mesh_with_itself():
    from surs_amd import metrics
    m = mr.torus()
    got = metrics.mesh_metrics(m, m, n=md.N_POINTS)
    B = md.bound(m[0])
    print("torus against itself: %r (B %.3e)" % (got, B))
    assert 0 <= got["p2s"] <= B and 0 <= got["gt2pred"] <= B and got["chamfer"] <= B
    assert got["normal_consistency"] >= 0.99
    flipped = metrics.mesh_metrics(m, mr.flipped(m), n=md.N_POINTS)
    assert flipped["normal_consistency"] >= 0.99 and flipped["p2s"] <= B                # either orientation


# ---------------------------------------------------------------- 12. a reconstruction, scored
def test_gen_mesh_metrics(tmp_path):
    import common
    import gpu_common as g
    from surs_amd import metrics, model, options, train_util, weights
    opt = options.BaseOptions().parse(common.FLAGS + ["--resolution", "32"])
    net = model.SuRSNet(opt).to(device=g.dev())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in common.state_dict().items()})
    net.eval()
    th = 0.4
    calib = np.identity(4)
    calib[:3, :3] = np.diag([0.011, -0.011, 0.011]) @ np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    calib[:3, 3] = [0.02, 1.1, -0.03]
    data = {"img_LR": torch.from_numpy(weights.synthetic_image(64, seed=1)), "b_min": np.array([-0.5] * 3), "b_max": np.array([0.5] * 3),
            "calib": torch.from_numpy(calib.astype(np.float32)[None])}
    with torch.no_grad():
        vh, fh, vl, fl = train_util.gen_mesh(opt, net, g.dev(), data, str(tmp_path / "a.obj"), use_octree=False)
    assert len(fh) > 0 and len(fl) > 0
    to_gt = metrics.pred_to_gt_transform(data["calib"])
    gt_hr, gt_lr = (metrics.transform_verts(to_gt, vh), fh), (metrics.transform_verts(to_gt, vl), fl)
    with torch.no_grad():
        got = train_util.gen_mesh_metrics(opt, net, g.dev(), data, save_path=str(tmp_path / "b.obj"), use_octree=False, n=2000,
                                          gt_hr=gt_hr, gt_lr=gt_lr)
    assert sorted(got) == ["HR", "LR"]
    for key, gt in (("HR", gt_hr), ("LR", gt_lr)):
        B = md.bound(gt[0])
        print("%s: %r (B %.3e, largest world coordinate %.1f)" % (key, got[key], B, np.abs(gt[0]).max()))
        assert got[key]["n"] == 2000 and 0 <= got[key]["chamfer"] <= B
        assert np.abs(gt[0]).max() > 20                                                 # the scans' frame, not the unit box
    for suffix in ("_HR.obj", "_LR.obj"):
        assert (tmp_path / ("a" + suffix)).read_bytes() == (tmp_path / ("b" + suffix)).read_bytes()
    with torch.no_grad():      # without a save_path nothing is written
        train_util.gen_mesh_metrics(opt, net, g.dev(), data, use_octree=False, n=100, gt_hr=gt_hr, gt_lr=gt_lr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a_HR.obj", "a_LR.obj", "b_HR.obj", "b_LR.obj"]
