"""CPU-only checks of the mesh distance (include/surs.h "mesh distance"): surs_mesh_distance_host - csrc/surs_mesh_distance.h looped
on the host, the bits the kernel gives - against the float64 yardstick tests/mesh_ref.py::surface_distance, the reported face, the
refusals of both entries, and the host side of metrics / train_util.gen_mesh_metrics.

Bound.  B = 2^-24 * 16 * S, S the largest |coordinate| among the call's vertices and points (mesh_dist_ref.bound): 2.2e-4 at the
default box.  EVERY point is within B, and the float64 distance to the reported face is within 2 B of the float64 minimum; no point
is left out.  Measured (the host loop; the kernel equals it bit for bit): at most 0.067 B (1.46e-5) on the four meshes, the reported
face at most 9.6e-7 behind the minimum, every vertex exactly 0."""
import ctypes as C

import numpy as np
import pytest

import mesh_dist_ref as md
import mesh_ref as mr
from surs_amd import _lib, native

E_INVALID = -1


@pytest.fixture(scope="module")
def host():
    """name -> (dist, face) of surs_mesh_distance_host on case(name), computed once."""
    got = {}

    def get(name):
        if name not in got:
            c = md.case(name)
            got[name] = native.mesh_distance_host(c["points"], c["v"], c["f"])
        return got[name]
    return get


# ---------------------------------------------------------------- 1. the distance
@pytest.mark.parametrize("name", list(md.MESHES))
def test_host_distance_within_bound(name, host):
    c, ref = md.case(name), md.reference(name)
    if name == "parts":
        assert len(c["f"]) == 2 * mr.FACES_PER_PART + 7 and _lib.lib().surs_mesh_contains_parts(len(c["f"])) == 3
    dist, face = host(name)
    assert dist.dtype == np.float32 and dist.shape == (len(c["points"]),) and np.isfinite(dist).all()
    err = np.abs(dist.astype(np.float64) - ref)
    print("%s: %d points, B %.3e, max |d32 - d64| %.3e = %.3f B, max distance %.1f" % (name, len(dist), c["B"], err.max(),
                                                                                     err.max() / c["B"], ref.max()))
    assert err.max() <= c["B"]
    assert (dist[c["vertices"]] == 0).all()           # a vertex is at distance 0 exactly
    assert ref.max() > 20 and (ref == 0).sum() >= len(c["v"])


# ---------------------------------------------------------------- 2. the face
@pytest.mark.parametrize("name", list(md.MESHES))
def test_host_face_attains_the_minimum(name, host):
    c, ref = md.case(name), md.reference(name)
    dist, face = host(name)
    assert face.dtype == np.int32 and face.min() >= 0 and face.max() < len(c["f"])
    d_face = md.distance_to_face(c["points"], c["v"], c["f"], face)
    print("%s: the reported face is at most %.3e behind the float64 minimum (2 B = %.3e)" % (name, (d_face - ref).max(), 2 * c["B"]))
    assert (d_face <= ref + 2 * c["B"]).all()
    if name == "torus":    # the lowest index of the float64 tie set, wherever fp32 cannot tell its members apart
        sets = md.argmin_sets(c["points"], c["v"], c["f"], 2 * c["B"])
        assert all(f in s for f, s in zip(face, sets))


def test_tie_reports_the_lower_face():
    """The midpoint of the cube's vertices 0 and 3 lies on the diagonal faces 0 and 1 share, and is exactly representable."""
    v, f = mr.cube()
    assert set(f[0]) & set(f[1]) == {0, 3}
    p = 0.5 * (v[0] + v[3])
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    dist, face = native.mesh_distance_host(p[None], v, f)
    assert dist[0] == 0 and face[0] == 0
    swapped = np.concatenate([f[1:2], f[0:1], f[2:]], 0)
    assert native.mesh_distance_host(p[None], v, swapped)[1][0] == 0            # whichever of the two comes first


def test_duplicate_face_is_never_reported(host):
    v, f = md.parts_with_duplicate()
    assert len(f) == 8200 and np.array_equal(f[8199], f[10]) and 8199 // mr.FACES_PER_PART == 2
    c = md.case("parts")
    dist, face = native.mesh_distance_host(c["points"], v, f)
    assert face.max() < 8199 and (face == 10).sum() > 0
    assert np.array_equal(dist, host("parts")[0]) and np.array_equal(face, host("parts")[1])


# ---------------------------------------------------------------- 3. refusals
def _call(device, n=4, ld=3, nv=8, nf=12, ws_bytes=None, points=True, verts=True, faces=True, dist=True):
    """One call of either entry on host arrays; the device entry must refuse before it touches them (or the device)."""
    lib = _lib.lib()
    v, f = mr.cube()
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    p = np.zeros((max(n, 1), max(ld, 3)), np.float32)
    d, fc = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
    ptr = lambda a, on: a.ctypes.data if on else None
    if device:
        need = lib.surs_mesh_distance_workspace_bytes(n, nf)
        ws = np.zeros(max(need, 8), np.uint8)
        return lib.surs_mesh_distance(ptr(p, points), n, ld, ptr(v, verts), nv, ptr(f, faces), nf, ws.ctypes.data,
                                      need if ws_bytes is None else ws_bytes, ptr(d, dist), fc.ctypes.data, None)
    return lib.surs_mesh_distance_host(ptr(p, points), n, ld, ptr(v, verts), nv, ptr(f, faces), nf, ptr(d, dist), fc.ctypes.data)


def _refused(device, word, **kw):
    assert _call(device, **kw) == E_INVALID
    msg = _lib.lib().surs_last_error().decode()
    assert word in msg, msg


@pytest.mark.parametrize("device", [False, True])
def test_refuses_negative_n(device):
    _refused(device, "n -1", n=-1)


@pytest.mark.parametrize("device", [False, True])
def test_refuses_no_faces(device):
    _refused(device, "nf 0", nf=0)


@pytest.mark.parametrize("device", [False, True])
def test_refuses_no_vertices(device):
    _refused(device, "nv 0", nv=0)


@pytest.mark.parametrize("device", [False, True])
def test_refuses_short_rows(device):
    _refused(device, "ld 2", ld=2)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("missing", ["points", "verts", "faces", "dist"])
def test_refuses_null_arrays(device, missing):
    _refused(device, "NULL", **{missing: False})


def test_refuses_small_workspace():
    lib = _lib.lib()
    need = lib.surs_mesh_distance_workspace_bytes(4, 12)
    assert need == 1 * 4 * 8                                              # [parts][n] of (fp32, int32)
    assert lib.surs_mesh_distance_workspace_bytes(1061, 8199) == 3 * 1061 * 8
    assert lib.surs_mesh_distance_workspace_bytes(1061, 8192) == 2 * 1061 * 8
    _refused(True, "%d needed" % need, ws_bytes=need - 1)


def test_workspace_bytes_of_bad_arguments_is_zero():
    lib = _lib.lib()
    assert [lib.surs_mesh_distance_workspace_bytes(n, nf) for n, nf in ((0, 12), (-1, 12), (4, 0), (4, -3))] == [0] * 4


def test_python_wrapper_checks_its_arrays():
    v, f = mr.cube()
    with pytest.raises(ValueError, match="points"):
        native.mesh_distance_host(np.zeros((3, 2), np.float32), v, f)
    with pytest.raises(_lib.SursError, match="nf 0"):
        native.mesh_distance_host(np.zeros((3, 3), np.float32), v, f[:0])


# ---------------------------------------------------------------- 4. non-finite points
def test_non_finite_point_is_inf_and_minus_one():
    for name in ("cube", "parts"):
        c = md.case(name)
        p = np.array([[np.nan, 100, 0], [0, np.inf, 0], [0, 100, -np.inf], [np.nan, np.inf, -np.inf], [1, 2, 3]], np.float32)
        dist, face = native.mesh_distance_host(p, c["v"], c["f"])
        assert np.array_equal(dist[:4], [np.inf] * 4) and np.array_equal(face[:4], [-1] * 4)
        assert np.isfinite(dist[4]) and face[4] >= 0


def test_rows_wider_than_three():
    c = md.case("torus")
    wide = np.full((64, 7), np.nan, np.float32)
    wide[:, :3] = c["points"][:64]
    a, b = native.mesh_distance_host(wide, c["v"], c["f"]), native.mesh_distance_host(c["points"][:64], c["v"], c["f"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_degenerate_triangles_are_segments_and_points():
    """A zero-area triangle is its three segments, a repeated vertex a point; out-of-range indices are clamped."""
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [5, 5, 5]], np.float32)
    p = np.array([[1, 3, 0], [-1, 0, 0], [5, 5, 9]], np.float32)
    dist, face = native.mesh_distance_host(p, v, np.array([[0, 1, 2]], np.int32))
    assert np.array_equal(dist, np.array([3, 1, np.sqrt(np.float32(9 + 25 + 81))], np.float32)) and (face == 0).all()
    dist, _ = native.mesh_distance_host(p, v, np.array([[3, 3, 3]], np.int32))
    assert np.array_equal(dist, np.array([np.sqrt(np.float32(16 + 4 + 25)), np.sqrt(np.float32(36 + 25 + 25)), 4], np.float32))
    clamped, _ = native.mesh_distance_host(p, v, np.array([[7, 99, 3]], np.int32))
    assert np.array_equal(clamped, dist)


# ---------------------------------------------------------------- 5. n == 0
@pytest.mark.parametrize("device", [False, True])
def test_no_points_is_success(device):
    assert _call(device, n=0) == 0
    assert _call(device, n=0, points=False, dist=False) == 0
    if not device:
        v, f = mr.cube()
        dist, face = native.mesh_distance_host(np.zeros((0, 3), np.float32), v, f)
        assert dist.shape == (0,) and face.shape == (0,)


def test_kernels_use_no_scratch(tmp_path):
    """The gfx950 cross-compile of csrc/surs_mesh_distance.hip with the library's flags: both kernels without scratch or spills
    (a spilled running minimum would show as twice the time of surs_mesh_contains, not as a wrong result)."""
    import os
    import re
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "surs_mesh_distance.hip"), "-o",
                        str(tmp_path / "md.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    field = lambda name: [int(x) for x in re.findall(re.escape(name) + r": (\d+)", r.stderr)]
    print("VGPRs %s, SGPRs %s, LDS %s" % (field("VGPRs"), field("TotalSGPRs"), field("LDS Size [bytes/block]")))
    assert len(re.findall(r"Function Name: \S*mesh_distance_(?:parts|reduce)_kernel", r.stderr)) == 2
    assert field("ScratchSize [bytes/lane]") == [0, 0] and field("VGPRs Spill") == [0, 0] and field("SGPRs Spill") == [0, 0]
    assert field("LDS Size [bytes/block]") == [256 * 7 * 16, 0]


# ---------------------------------------------------------------- 6. the frame rule
def test_pred_to_gt_transform():
    import torch
    from surs_amd import metrics, train_util
    th = 0.7
    rot = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    calib = np.identity(4)
    calib[:3, :3] = np.diag([-1.0, 1.0, 1.0]) @ (np.diag([0.011, -0.011, 0.011]) @ rot)     # a rotation, the scale and a flip
    calib[:3, 3] = [0.05, -1.1, 0.2]                                                        # and a translation
    calib32 = calib.astype(np.float32)
    gen = np.diag([2.0, -2.0, 2.0, 1.0])
    assert np.array_equal(train_util.gen_calib()[0].numpy(), gen.astype(np.float32))
    want = np.linalg.inv(calib32.astype(np.float64)) @ gen
    for given in (calib32, calib32[None], torch.from_numpy(calib32[None]), torch.from_numpy(np.stack([calib32, np.identity(4, np.float32)]))):
        got = metrics.pred_to_gt_transform(given)
        assert got.dtype == np.float64 and got.shape == (4, 4) and np.array_equal(got, want)
    det = np.linalg.det(want[:3, :3])      # gen_calib's own flip against the calib's two: the map reverses orientation
    assert det < 0 and abs(abs(det) ** (1 / 3) - 2 / 0.011) < 1e-3
    # a point of the scan, projected by the item's calib, is where gen_calib projects its image under the inverse map
    x = np.array([12.0, 100.0, -30.0, 1.0])
    assert np.allclose(gen @ np.linalg.solve(want, x), calib32.astype(np.float64) @ x, atol=1e-12)
    assert np.array_equal(metrics.pred_to_gt_transform(None), np.identity(4))
    assert np.array_equal(metrics.pred_to_gt_transform(gen[None]), np.identity(4))
    v = np.array([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0]])
    assert np.array_equal(metrics.transform_verts(want, v), v @ want[:3, :3].T + want[:3, 3])
    with pytest.raises(ValueError, match="calib"):
        metrics.pred_to_gt_transform(np.identity(3))


# ---------------------------------------------------------------- 7. argument checks that need no device
@pytest.mark.parametrize("n", [0, -5, 2.5, True, None])
def test_mesh_metrics_refuses_bad_n(n):
    from surs_amd import metrics
    with pytest.raises(ValueError, match="positive integer"):
        metrics.mesh_metrics(mr.cube(), mr.cube(), n=n)
    with pytest.raises(ValueError, match="positive integer"):
        metrics.surface_samples(None, n)


def test_mesh_metrics_refuses_what_is_no_mesh():
    from surs_amd import metrics
    for bad in (None, np.zeros((4, 3)), (1, 2, 3)):
        with pytest.raises(TypeError, match="verts, faces"):
            metrics.mesh_metrics(bad, bad, n=10)


def test_gen_mesh_metrics_checks_before_it_runs():
    """n and the presence of a ground truth are checked before the net or the device is touched."""
    from surs_amd import train_util
    item = {"mesh_path_HR": "a_HR.obj", "mesh_path_LR": "a_LR.obj"}
    with pytest.raises(ValueError, match="positive integer"):
        train_util.gen_mesh_metrics(None, None, None, item, n=0)
    with pytest.raises(ValueError, match="mesh_path_LR"):
        train_util.gen_mesh_metrics(None, None, None, {"mesh_path_HR": "a_HR.obj"})
    with pytest.raises(ValueError, match="mesh_path_HR"):
        train_util.gen_mesh_metrics(None, None, None, {}, gt_lr=mr.cube())
    with pytest.raises(ValueError, match="calib"):
        train_util.gen_mesh_metrics(None, None, None, dict(item, calib=np.identity(3)))
