"""CPU-only checks of the mesh raster (include/surs.h "mesh raster"): surs_mesh_raster_host and surs_mesh_shade_normals_host -
csrc/surs_mesh_raster.h looped on the host, the bits the kernels give - against the float64 yardstick tests/raster_ref.py, exact cases
on exactly representable inputs, the refusals of all four entries, and the host side of metrics.turntable_views / vertex_normals /
normal_error.

Bounds (raster_ref's docstring): tau_k = 2^-24 x 32 x (1 + G_k W) per barycentric, tau_z = 2^-24 x 16 x Z + (tau_1 + tau_2) Dz.  EVERY
pixel's reported face lies in its float64 candidate set, background is reported only where no face is sure, and on the pixels with a
single candidate depth and both barycentrics are within their bounds.  Measured (the host loop; the kernels equal it bit for bit) over
the thirteen cases: at most 1.02 % of a case's pixels have more than one candidate (32 of 3150, the torus seen edge-on; none in five
cases), and only there does the reported face ever differ from the float64 winner; the barycentrics are at most 0.029 tau off float64,
the depth at most 0.037 tau_z; flat colours at most 5.9e-7 off, smooth ones 8.2e-8 (FLOOR 2^-20 = 9.5e-7)."""
import numpy as np
import pytest

import mesh_ref as mr
import raster_ref as rr
from surs_amd import _lib, metrics, native

E_INVALID = -1
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def host():
    """name -> (face, depth, bary) of surs_mesh_raster_host on case(name), computed once."""
    got = {}

    def get(name):
        if name not in got:
            c = rr.case(name)
            got[name] = native.mesh_raster_host(c["v"], c["f"], c["view"], c["size"])
        return got[name]
    return get


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("name", list(rr.CASES))
def test_host_raster_against_float64(name, host):
    c, ref = rr.case(name), rr.reference(name)
    h, w = c["size"]
    face, depth, bary = host(name)
    assert face.shape == (h, w) and face.dtype == np.int32 and depth.shape == (h, w) and bary.shape == (h, w, 2)
    face, depth, bary = face.reshape(-1), depth.reshape(-1), bary.reshape(-1, 2)
    P = h * w
    assert face.min() >= -1 and face.max() < len(c["f"])
    covered = face >= 0
    # every pixel: the reported face is a candidate; background only where no face is sure
    assert ref["cand"][np.nonzero(covered)[0], face[covered]].all()
    assert not ref["sure_any"][~covered].any()
    assert np.isnan(depth[~covered]).all() and np.isfinite(depth[covered]).all() and (bary[~covered] == 0).all()
    multi = int((ref["n_cand"] > 1).sum())
    single = (ref["n_cand"] == 1) & covered
    assert np.array_equal(face[single], ref["one"][single])
    e1 = np.abs(bary[single, 0] - ref["b1"][single]) / ref["tau1"][single]
    e2 = np.abs(bary[single, 1] - ref["b2"][single]) / ref["tau2"][single]
    ez = np.abs(depth[single] - ref["z"][single]) / ref["tauz"][single]
    worst = lambda e: float(e.max()) if e.size else 0.0
    print("%s: %d pixels, %d covered, %d with several candidates (%.2f %%), differing from the float64 winner %d; max |b - b64| %.4f tau, "
          "max |z - z64| %.4f tau_z; W %.1f" % (name, P, covered.sum(), multi, 100.0 * multi / P,
                                                int((face != ref["winner"]).sum()), max(worst(e1), worst(e2)), worst(ez), ref["W"]))
    assert worst(e1) <= 1 and worst(e2) <= 1 and worst(ez) <= 1
    if "half_off" in name:
        assert 0 < covered.sum() and covered[np.arange(P) % w == w - 1].any()         # the mesh runs off the right edge
    else:
        assert covered.sum() > 20
    assert multi <= 0.05 * P and single.sum() >= 0.5 * covered.sum()          # the comparison with float64 is not vacuous


def test_cases_cover_what_they_should():
    assert len(rr.case("torus_70x45_0")["f"]) == 576
    dets = {n: np.sign(np.linalg.det(rr.case(n)["view"][:, :3])) for n in rr.CASES}
    assert dets["ellipsoid_70x45_flip"] == -dets["ellipsoid_70x45_270"]
    assert {rr.CASES[n][1] for n in rr.CASES} == {(45, 70), (33, 33), (96, 96)}


# ---------------------------------------------------------------- 2. exact cases: an 8 x 8 image, the identity view
EYE = np.identity(4)[:3]


def _at(sx, sy, z=0.0, n=8):
    """The world point that the identity view puts on pixel centre (column sx, row sy) of an n x n image: dyadic, exact in fp32."""
    return [(sx + 0.5) * 2.0 / n - 1.0, (sy + 0.5) * 2.0 / n - 1.0, z]


def _faces(v, f, size=8, view=EYE):
    v = np.array(v, np.float64)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v, equal_nan=True)
    return native.mesh_raster_host(v, np.array(f, np.int32), view, size)


def test_pixel_centre_on_a_shared_edge_reports_the_lower_face():
    v = [_at(1, 1), _at(5, 1), _at(5, 5), _at(1, 5)]
    for f in ([[0, 1, 2], [0, 2, 3]], [[0, 2, 3], [0, 1, 2]], [[2, 1, 0], [0, 2, 3]]):
        face, depth, bary = _faces(v, f)
        assert [face[k, k] for k in range(1, 6)] == [0] * 5            # the diagonal, both end vertices included
        assert face[2, 4] == (0 if f[0] != [0, 2, 3] else 1) and face[4, 2] == (1 if f[0] != [0, 2, 3] else 0)
        assert (face[1:6, 1:6] >= 0).all() and (face[0] == -1).all() and (face[:, 6:] == -1).all()   # edges are inclusive
        assert (depth[1:6, 1:6] == 0).all()
    assert tuple(bary[3, 3]) == (0.0, 0.5)


def test_coplanar_duplicate_reports_the_lower_index():
    v = [_at(0, 0, 0.25), _at(8, 0, 0.25), _at(0, 8, 0.5)]        # edges of 8 pixels: every barycentric is a multiple of 1 / 8
    face, depth, _ = _faces(v, [[0, 1, 2], [0, 1, 2], [1, 2, 0]])
    assert (face == 0).sum() == 43 and (face > 0).sum() == 0 and depth[0, 0] == 0.25 and depth[7, 0] == 0.46875


def test_nearer_face_wins_whatever_its_index():
    v = [_at(0, 0, 0.0), _at(8, 0, 0.0), _at(0, 8, 0.0), _at(0, 0, 0.5), _at(8, 0, 0.5), _at(0, 8, 0.5)]
    for f, want in (([[0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [0, 1, 2]], 0)):
        face, depth, _ = _faces(v, f)
        assert (face == want).sum() == 43 and (face == 1 - want).sum() == 0 and (depth[face >= 0] == 0.5).all()   # the LARGER z'


def test_whole_image_off_image_zero_area_and_edge_on():
    face, depth, bary = _faces([_at(-20, -10), _at(40, -10), _at(-20, 50)], [[0, 1, 2]])
    assert (face == 0).all() and (depth == 0).all()
    assert (_faces([_at(9, 9), _at(12, 9), _at(9, 12)], [[0, 1, 2]])[0] == -1).all()           # wholly off the image
    assert (_faces([_at(1, 1), _at(5, 5), _at(1, 1)], [[0, 1, 2]])[0] == -1).all()             # a repeated vertex
    assert (_faces([_at(1, 1), _at(3, 3), _at(5, 5)], [[0, 1, 2]])[0] == -1).all()             # collinear
    assert (_faces([_at(3, 1, 0.0), _at(3, 5, 0.0), _at(3, 3, 0.5)], [[0, 1, 2]])[0] == -1).all()   # edge-on: through pixel centres
    face, depth, _ = _faces([_at(1, 1), _at(5, 1), _at(1, 5), [np.nan, 0, 0], [np.inf, 0, 0]], [[0, 1, 3], [0, 4, 2], [0, 1, 2]])
    assert set(face.reshape(-1)) == {-1, 2}                                                  # non-finite vertices cover nothing


def test_face_index_out_of_range_is_clamped():
    v = [_at(1, 1), _at(5, 1), _at(1, 5)]
    want = _faces(v, [[0, 1, 2]])
    for f in ([[0, 1, 99]], [[-5, 1, 2]], [[-1, 1, 2 ** 31 - 1]]):
        got = _faces(v, f)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want))
    assert (want[0] == 0).sum() == 15


# ---------------------------------------------------------------- 3. shading
@pytest.mark.parametrize("name", ["cube_33_37", "torus_96_tilt", "ellipsoid_70x45_flip", "torus_33_flip_tilt", "ellipsoid_33_37_tilt"])
def test_flat_normals(name, host):
    c = rr.case(name)
    face = host(name)[0]
    worst = 0.0
    for mesh in ((c["v"], c["f"]), mr.flipped((c["v"], c["f"]))):
        got, mask = native.normal_map_host(mesh[0], mesh[1], c["view"], c["size"])
        assert got.dtype == np.float32 and got.shape == c["size"] + (3,) and np.array_equal(mask, face >= 0)
        want = rr.flat_colours(c["v"], c["f"], c["view"], face).reshape(got.shape)
        n = 2.0 * got[mask].astype(np.float64) - 1.0
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= FLOOR and np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 2 * FLOOR
        assert (got[mask][:, 2] >= 0.5).all() and (got[~mask] == 0).all()                     # n_z' >= 0; background exactly (0, 0, 0)
    print("%s: flat colours at most %.3e off float64 (FLOOR %.3e)" % (name, worst, FLOOR))


@pytest.mark.parametrize("name", ["ellipsoid_33_37_tilt", "ellipsoid_70x45_flip"])
def test_smooth_normals(name, host):
    c = rr.case(name)
    face, _, bary = host(name)
    vn = metrics.vertex_normals((c["v"], c["f"]))
    assert np.abs(vn - rr.vertex_normals(c["v"], c["f"])).max() < 1e-12 and np.abs(np.linalg.norm(vn, axis=1) - 1).max() < 1e-12
    got, mask = native.normal_map_host(c["v"], c["f"], c["view"], c["size"], vertex_normals=vn)
    want = rr.smooth_colours(c["v"], c["f"], c["view"], vn, face, bary).reshape(got.shape)
    print("%s: smooth colours at most %.3e off float64" % (name, np.abs(got - want).max()))
    assert np.abs(got - want).max() <= FLOOR and (got[~mask] == 0).all() and (got[mask][:, 2] >= 0.5).all()
    flat = native.normal_map_host(c["v"], c["f"], c["view"], c["size"])[0]
    assert np.abs(got - flat).max() > 0                                                     # another map, of the same surface
    # an ellipsoid's normal is (x / a^2, ..) normalised: the blend follows it, the flat normals are coarser
    centre, radii = np.array([0.0, 100.0, 0.0]), np.array([50.0, 80.0, 30.0])
    t = c["v"][np.sort(c["f"], axis=1)[face.reshape(-1).clip(0)]]
    b = bary.reshape(-1, 2).astype(np.float64)
    pts = (1 - b.sum(1))[:, None] * t[:, 0] + b[:, :1] * t[:, 1] + b[:, 1:] * t[:, 2]
    true = (pts - centre) / radii ** 2 @ np.linalg.inv(c["view"][:, :3])
    true = true / np.linalg.norm(true, axis=1, keepdims=True)
    true = 0.5 * np.where(true[:, 2:3] < 0, -true, true) + 0.5
    m = mask.reshape(-1)
    err_smooth = np.abs(got.reshape(-1, 3)[m] - true[m]).mean()
    err_flat = np.abs(flat.reshape(-1, 3)[m] - true[m]).mean()
    assert err_smooth < 0.6 * err_flat


# ---------------------------------------------------------------- 4. views and the score
def test_turntable_views():
    calib = rr.base_calib() @ rr.tilt(20)
    views = metrics.turntable_views(calib, (0, 90, 180, 270, 360, 37), rr.CENTRE)
    assert views.dtype == np.float64 and views.shape == (6, 4, 4)
    assert np.array_equal(views[0], calib) and np.array_equal(metrics.turntable_views(calib)[0], calib)
    assert np.abs(views[4] - calib).max() <= 1e-12
    assert np.abs(views - rr.turntable(calib, (0, 90, 180, 270, 360, 37), rr.CENTRE)).max() <= 1e-12
    assert np.array_equal(metrics.turntable_views(calib[None], (90,))[0], metrics.turntable_views(calib, (90,), (0, 0, 0))[0])
    # the torus is symmetric about the vertical axis through CENTRE: the back view's mask is the front view's, mirrored
    v, f = mr.torus(bump=0.0)
    tt = metrics.turntable_views(rr.base_calib(), (0, 180), rr.CENTRE)
    front, back = (native.mesh_raster_host(v, f, m, (45, 70))[0] >= 0 for m in tt)
    assert front.sum() > 100 and np.array_equal(back, front[:, ::-1])


def _host_maps(mesh, views, size, smooth=False):
    vn = metrics.vertex_normals(mesh) if smooth else None
    got = [native.normal_map_host(mesh[0], mesh[1], m, size, vn) for m in views]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def test_normal_error_restated_on_the_host_maps():
    views = metrics.turntable_views(rr.base_calib() @ rr.tilt(30), (0, 90, 180, 270), rr.CENTRE)
    torus = mr.torus()
    a = _host_maps(torus, views, (45, 70))
    same = rr.restate_normal_error(*a, *a)
    assert same["normal_error"] == 0 and same["mask_iou"] == 1 and same["per_view"] == [0.0] * 4
    flipped = rr.restate_normal_error(*a, *_host_maps(mr.flipped(torus), views, (45, 70)))
    assert flipped["normal_error"] == 0 and flipped["mask_iou"] == 1                       # either orientation
    moved = rr.restate_normal_error(*a, *_host_maps((mr._f32(torus[0] + [6.0, 3.0, 0.0]), torus[1]), views, (45, 70)))
    assert moved["normal_error"] > 1e-3 and 0.3 < moved["mask_iou"] < 1 and all(e > 0 for e in moved["per_view"])
    empty = np.zeros((1, 4, 4, 3), np.float32), np.zeros((1, 4, 4), bool)
    assert rr.restate_normal_error(*empty, *empty)["mask_iou"] == 1                         # neither mesh is seen


def test_default_arguments_return_todays_keys():
    import inspect
    from surs_amd import train_util
    sig = inspect.signature(train_util.gen_mesh_metrics)
    assert sig.parameters["normal_views"].default is None and sig.parameters["normal_size"].default == 512
    assert list(inspect.signature(metrics.mesh_metrics).parameters) == ["pred", "gt", "n", "seed"]
    assert list(inspect.signature(metrics.normal_error).parameters) == ["pred", "gt", "views", "size", "smooth", "centre"]
    assert inspect.signature(metrics.turntable_views).parameters["degrees"].default == (0, 90, 180, 270)


# ---------------------------------------------------------------- 5. refusals
def _call(entry, w=8, h=8, nv=8, nf=12, ws_bytes=None, verts=True, faces=True, view=True, face=True, out=True, vn=False, nm=True,
          bary=True):
    """One call of an entry on host arrays filled with a pattern; the device entries must refuse before they touch them (or the
    device).  Returns (code, the arrays an entry could have written)."""
    lib = _lib.lib()
    v, f = mr.cube()
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    m = np.ascontiguousarray(rr.case("cube_33_90")["view"], np.float32)
    n = 64
    fc, dp, by, o = np.full(n, 7, np.int32), np.full(n, 7, np.float32), np.full(2 * n, 7, np.float32), np.full(3 * n, 7, np.float32)
    normals, matrix = np.ones((8, 3), np.float32), np.identity(3, dtype=np.float32)
    ptr = lambda a, on: a.ctypes.data if on else None
    need = lib.surs_mesh_raster_workspace_bytes(w, h, nf)
    ws = np.full(max(min(need, 1 << 20), 8), 7, np.uint8)
    if entry == "raster":
        code = lib.surs_mesh_raster(ptr(v, verts), nv, ptr(f, faces), nf, ptr(m, view), w, h, ws.ctypes.data,
                                    need if ws_bytes is None else ws_bytes, ptr(fc, face), dp.ctypes.data, by.ctypes.data, None)
    elif entry == "raster_host":
        code = lib.surs_mesh_raster_host(ptr(v, verts), nv, ptr(f, faces), nf, ptr(m, view), w, h, ptr(fc, face), dp.ctypes.data,
                                         by.ctypes.data)
    elif entry == "shade":
        code = lib.surs_mesh_shade_normals(ptr(v, verts), nv, ptr(f, faces), nf, ptr(m, view), ptr(normals, vn), ptr(matrix, nm),
                                           ptr(fc, face), ptr(by, bary), w, h, ptr(o, out), None)
    else:
        code = lib.surs_mesh_shade_normals_host(ptr(v, verts), nv, ptr(f, faces), nf, ptr(m, view), ptr(normals, vn), ptr(matrix, nm),
                                                ptr(fc, face), ptr(by, bary), w, h, ptr(o, out))
    return code, (fc, dp, by, o, ws)


def _refused(entry, word, **kw):
    code, arrays = _call(entry, **kw)
    assert code == E_INVALID
    msg = _lib.lib().surs_last_error().decode()
    assert word in msg, msg
    assert all((a == 7).all() for a in arrays)              # nothing touched


ENTRIES = ["raster", "raster_host", "shade", "shade_host"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_refuses_bad_sizes_and_null_mesh(entry):
    _refused(entry, "w 0 x h 8", w=0)
    _refused(entry, "w 8 x h -1", h=-1)
    _refused(entry, "w 8193 x h 8", w=8193)
    _refused(entry, "w 8 x h 8193", h=8193)
    _refused(entry, "nf 0", nf=0)
    _refused(entry, "nv 0", nv=0)
    _refused(entry, "NULL", verts=False)
    _refused(entry, "NULL", faces=False)
    _refused(entry, "NULL", view=False)
    _refused(entry, "face", face=False)


@pytest.mark.parametrize("entry", ["shade", "shade_host"])
def test_shading_refuses_missing_arrays(entry):
    _refused(entry, "out", out=False)
    _refused(entry, "normal matrix", vn=True, nm=False)
    _refused(entry, "bary", vn=True, bary=False)
    if entry == "shade_host":      # flat shading needs neither
        code, (fc, dp, by, o, ws) = _call(entry, nm=False, bary=False, w=2, h=2)
        assert code == 0 and (o[:12].reshape(4, 3)[:, 2] >= 0.5).all() and (o[12:] == 7).all()


def test_raster_refuses_short_workspace_and_too_many_parts():
    lib = _lib.lib()
    need = lib.surs_mesh_raster_workspace_bytes(8, 8, 12)
    assert need == 256 + 8 * 8 * 16 and lib.surs_mesh_raster_parts(12) == 1
    _refused("raster", "workspace of %d bytes, %d needed" % (need - 1, need), ws_bytes=need - 1)
    assert lib.surs_mesh_raster_workspace_bytes(0, 8, 12) == 0 and lib.surs_mesh_raster_workspace_bytes(8, 8, 0) == 0
    old = native.get_option("raster_part")
    try:
        native.set_option("raster_part", 256)
        assert lib.surs_mesh_raster_parts(576) == 3 and lib.surs_mesh_raster_parts(512) == 2 and lib.surs_mesh_raster_parts(513) == 3
        assert lib.surs_mesh_raster_workspace_bytes(70, 45, 576) == 576 * 16 + 3 * 70 * 45 * 16
        nf = 256 * 65535 + 1
        _refused("raster", "%d faces make 65536 face parts of 256" % nf, nf=nf, w=1, h=1)
        for bad in (0, 100, 257, -256):
            native.set_option("raster_part", bad)
            _refused("raster", "raster_part %d" % bad)
            assert lib.surs_mesh_raster_parts(576) == 0
    finally:
        native.set_option("raster_part", old)
    assert old % 256 == 0 and "raster_part" in native.options()


# ---------------------------------------------------------------- 6. the shipped kernels
def test_kernels_use_no_scratch_and_no_atomics(tmp_path):
    """The four kernels in the shipped gfx950 code object (llvm-readelf / llvm-objdump, CPU only): no scratch, at most 128 registers
    (512 per SIMD lane: four waves per SIMD, so four workgroups of the parts kernel per CU hide each other's barriers), and no atomic
    instruction to global memory or to LDS - the winner is a comparison, never an atomic maximum."""
    import isa
    if not isa.available():
        pytest.skip("llvm-objdump / llvm-readelf or the built library missing")
    found = {}
    for co in isa.code_objects(isa.SO, str(tmp_path)):
        md, dis = isa.kernel_metadata(co), isa.disassembly(co)
        names = isa.demangle(list(md))
        for k, m in md.items():
            if "mesh_raster_" in names[k] or "mesh_shade_normals_" in names[k]:
                found[names[k]] = (m, dis[k])
    assert len(found) == 4, sorted(found)
    for name, (m, ins) in found.items():
        print("%s: %s registers, %s bytes of scratch, %s bytes of LDS, %d instructions" % (
            name[:60], m[".vgpr_count"], m[".private_segment_fixed_size"], m[".group_segment_fixed_size"], len(ins)))
        assert int(m[".private_segment_fixed_size"]) == 0 and int(m[".vgpr_count"]) <= 128
        assert not [i for i in ins if i.startswith(("global_atomic", "flat_atomic", "ds_add", "ds_max", "ds_min", "ds_cmpst"))]
        assert not [i for i in ins if i.startswith("scratch_")]
    parts = [m for n, (m, _) in found.items() if "parts_kernel" in n][0]
    assert int(parts[".group_segment_fixed_size"]) == 256 * 5 * 16 + 256 * 4 + 4 * 4
