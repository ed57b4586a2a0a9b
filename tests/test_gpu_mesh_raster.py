"""GPU checks of the mesh raster kernels (csrc/surs_mesh_raster.hip) and of the score built on them (metrics.normal_error,
train_util.gen_mesh_metrics(normal_views=...)).  The kernels are held to surs_mesh_raster_host / surs_mesh_shade_normals_host BIT FOR
BIT - the same header looped on the host, which tests/test_mesh_raster_host.py holds to the float64 yardstick tests/raster_ref.py - at
the option raster_part = 256 (several face parts on meshes of a few hundred faces) and at its default; a pixel's results may depend
neither on the workspace and the output buffers nor on the image it sits in.  The score is compared with its float64 restatement on
the GPU's own maps within 2^-20."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import raster_ref as rr

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
_dev_mesh = {}


def _native_mesh(key, mesh):
    from surs_amd import native
    if key not in _dev_mesh:
        _dev_mesh[key] = native.Mesh(mesh[0], mesh[1])
    return _dev_mesh[key]


class _part:
    """The option raster_part set for a block (None: the default)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from surs_amd import native
        self.old = native.get_option("raster_part")
        if self.value is not None:
            native.set_option("raster_part", self.value)

    def __exit__(self, *exc):
        from surs_amd import native
        native.set_option("raster_part", self.old)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def host():
    """name -> (face, depth, bary, flat map, smooth map) of the host entries on case(name), computed once."""
    from surs_amd import metrics, native
    got = {}

    def get(name):
        if name not in got:
            c = rr.case(name)
            vn = metrics.vertex_normals((c["v"], c["f"]))
            got[name] = native.mesh_raster_host(c["v"], c["f"], c["view"], c["size"]) + (
                native.normal_map_host(c["v"], c["f"], c["view"], c["size"])[0],
                native.normal_map_host(c["v"], c["f"], c["view"], c["size"], vn)[0], vn)
        return got[name]
    return get


# ---------------------------------------------------------------- 1. the kernels are the host loops, bit for bit
@pytest.mark.parametrize("part", [256, None])
@pytest.mark.parametrize("name", list(rr.CASES))
def test_kernels_equal_host_bit_for_bit(name, part, host):
    from surs_amd import _lib, native
    c = rr.case(name)
    m = _native_mesh(c["mesh"], (c["v"], c["f"]))
    face_h, depth_h, bary_h, flat_h, smooth_h, vn = host(name)
    with _part(part):
        if part == 256 and c["mesh"] == "torus":
            assert _lib.lib().surs_mesh_raster_parts(m.nf) == 3
        face, depth, bary = native.mesh_raster(m, c["view"], c["size"], want_depth=True, want_bary=True)
        assert face.dtype == torch.int32 and tuple(face.shape) == c["size"] and tuple(bary.shape) == c["size"] + (2,)
        got = face.cpu().numpy(), depth.cpu().numpy(), bary.cpu().numpy()
        print("%s, part %s: %d covered, faces differing from the host %d" % (name, part, (got[0] >= 0).sum(), (got[0] != face_h).sum()))
        assert _same(got, (face_h, depth_h, bary_h))                                   # (the NaN pattern of depth included)
        assert _same([native.mesh_raster(m, c["view"], c["size"]).cpu().numpy()], [face_h])       # depth and bary are nullable
        only_depth = native.mesh_raster(m, c["view"], c["size"], want_depth=True)
        assert _same([only_depth[0].cpu().numpy(), only_depth[1].cpu().numpy()], [face_h, depth_h])
        flat, mask = native.normal_map(m, c["view"], c["size"])
        smooth, mask_s = native.normal_map(m, c["view"], c["size"], vertex_normals=vn)
    assert flat.dtype == torch.float32 and tuple(flat.shape) == c["size"] + (3,) and mask.dtype == torch.bool
    assert _same([flat.cpu().numpy(), smooth.cpu().numpy()], [flat_h, smooth_h])
    assert np.array_equal(mask.cpu().numpy(), face_h >= 0) and torch.equal(mask, mask_s)


def test_kernel_clamps_indices_and_skips_what_covers_nothing():
    """Out-of-range vertex indices are clamped (straight through the C entry: native.Mesh would refuse them), and faces that cover
    nothing - zero area, edge-on, off the image, non-finite - sit among the others."""
    import gpu_common as g
    from surs_amd import _lib, native
    c = rr.case("torus_70x45_0")
    v = np.concatenate([c["v"], [[np.nan, 0, 0], [np.inf, -np.inf, 0]]], 0).astype(np.float32)
    nv = len(v) - 2                                   # the kernel is told of the finite vertices only ...
    f = np.concatenate([c["f"][:300], [[5, 5, 9], [3, 3, 3], [0, 1, nv + 5], [-7, 2, 4]], c["f"][300:]], 0).astype(np.int32)
    h, w = c["size"]
    view = np.ascontiguousarray(c["view"], np.float32)
    want = native.mesh_raster_host(v[:nv], f, view, (h, w))
    vd, fd = torch.from_numpy(v).to(g.dev()), torch.from_numpy(f).to(g.dev())
    with _part(256):
        need = _lib.lib().surs_mesh_raster_workspace_bytes(w, h, len(f))
        ws = torch.empty(need, dtype=torch.uint8, device=g.dev())
        face = torch.empty((h, w), dtype=torch.int32, device=g.dev())
        depth = torch.empty((h, w), dtype=torch.float32, device=g.dev())
        bary = torch.empty((h, w, 2), dtype=torch.float32, device=g.dev())
        native.check(_lib.lib().surs_mesh_raster(native._ptr(vd), nv, native._ptr(fd), len(f), view.ctypes.data, w, h, native._ptr(ws),
                                                 need, native._ptr(face), native._ptr(depth), native._ptr(bary), native._stream()))
    assert _same((face.cpu().numpy(), depth.cpu().numpy(), bary.cpu().numpy()), want)
    assert (want[0] >= 0).sum() > 100
    # ... and faces on vertices that ARE non-finite cover nothing: the rest is drawn as before
    far = np.concatenate([f[:300], f[304:], [[0, 1, nv], [0, 1, nv + 1]]], 0).astype(np.int32)
    m = native.Mesh.__new__(native.Mesh)
    m.verts, m.faces, m.nv, m.nf = vd, torch.from_numpy(far).to(g.dev()), len(v), len(far)
    with _part(256):
        got = native.mesh_raster(m, view, (h, w), want_depth=True, want_bary=True)
    assert _same([a.cpu().numpy() for a in got], native.mesh_raster_host(c["v"], c["f"], view, (h, w)))


# ---------------------------------------------------------------- 2. buffers and the image
def test_same_bits_from_other_buffers_and_padding_stays():
    import gpu_common as g
    from surs_amd import _lib, native
    c = rr.case("torus_70x45_0")
    m = _native_mesh("torus", (c["v"], c["f"]))
    h, w = c["size"]
    view = np.ascontiguousarray(c["view"], np.float32)
    pad = 37
    outs = []
    with _part(256):
        need = _lib.lib().surs_mesh_raster_workspace_bytes(w, h, m.nf)
        assert need == 576 * 16 + 3 * h * w * 16
        ws = [torch.full((need,), 0xFF, dtype=torch.uint8, device=g.dev()), torch.zeros(need + 4096, dtype=torch.uint8, device=g.dev())]
        for k, (wsp, offset) in enumerate(((ws[0], 0), (ws[1], 2048), (ws[0], 0))):
            face = torch.full((h * w + pad,), -99, dtype=torch.int32, device=g.dev())
            depth = torch.full((h * w + pad,), float("nan"), dtype=torch.float32, device=g.dev())
            bary = torch.full((2 * h * w + pad,), float("nan"), dtype=torch.float32, device=g.dev())
            out = torch.full((3 * h * w + pad,), float("nan"), dtype=torch.float32, device=g.dev())
            native.check(_lib.lib().surs_mesh_raster(native._ptr(m.verts), m.nv, native._ptr(m.faces), m.nf, view.ctypes.data, w, h,
                                                     wsp.data_ptr() + offset, need, native._ptr(face), native._ptr(depth),
                                                     native._ptr(bary), native._stream()))
            native.check(_lib.lib().surs_mesh_shade_normals(native._ptr(m.verts), m.nv, native._ptr(m.faces), m.nf, view.ctypes.data, None,
                                                            None, native._ptr(face), None, w, h, native._ptr(out), native._stream()))
            face, depth, bary, out = face.cpu().numpy(), depth.cpu().numpy(), bary.cpu().numpy(), out.cpu().numpy()
            assert (face[h * w:] == -99).all() and np.isnan(depth[h * w:]).all() and np.isnan(bary[2 * h * w:]).all()
            assert np.isnan(out[3 * h * w:]).all() and not np.isnan(out[:3 * h * w]).any() and not np.isnan(bary[:2 * h * w]).any()
            outs.append((face[:h * w], depth[:h * w], bary[:2 * h * w], out[:3 * h * w]))
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
    want = native.mesh_raster_host(c["v"], c["f"], view, (h, w))
    assert _same(outs[0][:3], [a.reshape(-1) for a in want])


@pytest.mark.parametrize("kind", ["inside", "flip", "half_off"])
def test_a_pixel_does_not_depend_on_its_image(kind):
    """The 70 x 45 image is the top half of a 70 x 90 image whose view has y' halved and moved up, y'' = (y' - 1) / 2: (y'' + 1) 90 / 2
    = (y' + 1) 45 / 2.  For fp32 to sample the SAME points the projection itself must be free of rounding in both views: the torus'
    vertices are rounded to multiples of 1 / 64 and the view looks down the y axis with a scale of 2^-8 (2^-7 for half_off), so every
    product and sum of the matrix rows is exact; the rest of the arithmetic then sees the same numbers."""
    from surs_amd import native
    v, f = mr.torus()
    v = np.round(v * 64.0) / 64.0
    s = 2.0 ** -7 if kind == "half_off" else 2.0 ** -8
    small = np.array([[-s if kind == "flip" else s, 0, 0, 0.75 if kind == "half_off" else 0.0], [0, 0, -s, 0.125], [0, s, 0, -100 * s]])
    tall = small.copy()
    tall[1] = 0.5 * small[1]
    tall[1, 3] -= 0.5
    assert np.array_equal(rr._f32(tall), tall) and np.array_equal(rr._f32(v), v)
    m = native.Mesh(v, f)
    with _part(256):
        a = [t.cpu().numpy() for t in native.mesh_raster(m, small, (45, 70), want_depth=True, want_bary=True)]
        b = [t.cpu().numpy() for t in native.mesh_raster(m, tall, (90, 70), want_depth=True, want_bary=True)]
        na, nb = native.normal_map(m, small, (45, 70))[0].cpu().numpy(), native.normal_map(m, tall, (90, 70))[0].cpu().numpy()
    assert _same(a, [t[:45] for t in b])
    covered = a[0] >= 0
    assert covered.sum() > 200 and (covered[:, -1].any() if kind == "half_off" else not covered[:, -1].any())
    assert len(np.unique(a[0])) > 100 and (b[0][45:] >= 0).sum() < covered.sum()
    # the normals are those of another camera (y' is halved): only their masks agree
    assert np.array_equal(na.any(-1), nb[:45].any(-1))
    assert _same(b, native.mesh_raster_host(v, f, tall, (90, 70)))


# ---------------------------------------------------------------- 3. the scores
def _views():
    from surs_amd import metrics
    return metrics.turntable_views(rr.base_calib() @ rr.tilt(30), (0, 90, 180, 270), rr.CENTRE)


def _device_maps(mesh, views, size):
    from surs_amd import native
    got = [native.normal_map(mesh, m, size) for m in views]
    return [g[0].cpu().numpy() for g in got], [g[1].cpu().numpy() for g in got]


def test_normal_error_against_float64():
    from surs_amd import metrics, native
    pred, gt = mr.torus(), (mr._f32(mr.torus()[0] + [6.0, 3.0, 0.0]), mr.torus()[1])
    mp, mg = native.Mesh(*pred), native.Mesh(*gt)
    views, size = _views(), (45, 70)
    got = metrics.normal_error(mp, mg, views, size=size)
    assert sorted(got) == ["mask_iou", "normal_error", "per_view", "size"] and got["size"] == size
    assert isinstance(got["normal_error"], float) and isinstance(got["mask_iou"], float) and len(got["per_view"]) == 4
    want = rr.restate_normal_error(*_device_maps(mp, views, size), *_device_maps(mg, views, size))
    print("normal_error %.9f against %.9f, mask_iou %.9f against %.9f" % (got["normal_error"], want["normal_error"], got["mask_iou"],
                                                                        want["mask_iou"]))
    assert abs(got["normal_error"] - want["normal_error"]) <= FLOOR and abs(got["mask_iou"] - want["mask_iou"]) <= FLOOR
    assert np.abs(np.array(got["per_view"]) - want["per_view"]).max() <= FLOOR
    assert got["normal_error"] > 1e-3 and 0.3 < got["mask_iou"] < 1
    assert metrics.normal_error(pred, gt, views, size=size) == got                       # (verts, faces) pairs are uploaded; same bits
    assert metrics.normal_error(mp, mg, views[:, :3], size=size) == got                  # [V,3,4]
    smooth = metrics.normal_error(mp, mg, views, size=size, smooth=True)
    assert smooth["mask_iou"] == got["mask_iou"] and smooth["normal_error"] != got["normal_error"]


def test_normal_error_of_a_mesh_with_itself_and_its_flipped_copy():
    from surs_amd import metrics, native
    m = mr.torus()
    views = _views()
    for other in (m, mr.flipped(m)):
        for smooth in (False, True):
            got = metrics.normal_error(m, other, views, size=(45, 70), smooth=smooth)
            assert got["normal_error"] == 0 and got["per_view"] == [0.0] * 4 and got["mask_iou"] == 1
    # views given as turntable degrees: about the centre of gt's box; a mesh that no view sees scores an IoU of 1
    ndc = (mr._f32((m[0] - rr.CENTRE) * rr.SCALE), m[1])
    by_degrees = metrics.normal_error(ndc, ndc, (0, 90), size=33)
    assert by_degrees["size"] == (33, 33) and by_degrees["normal_error"] == 0 and by_degrees["mask_iou"] == 1
    far = (mr._f32(ndc[0] + [5.0, 0.0, 0.0]), m[1])
    assert metrics.normal_error(far, far, np.identity(4)[None], size=33)["mask_iou"] == 1


def test_gen_mesh_metrics_with_normal_views(tmp_path):
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
    to_gt = metrics.pred_to_gt_transform(data["calib"])
    gt_hr, gt_lr = (metrics.transform_verts(to_gt, vh), fh), (metrics.transform_verts(to_gt, vl), fl)
    with torch.no_grad():
        plain = train_util.gen_mesh_metrics(opt, net, g.dev(), data, use_octree=False, n=500, gt_hr=gt_hr, gt_lr=gt_lr)
        got = train_util.gen_mesh_metrics(opt, net, g.dev(), data, use_octree=False, n=500, gt_hr=gt_hr, gt_lr=gt_lr,
                                          normal_views=(0, 90, 180, 270), normal_size=64)
    today = ["chamfer", "gt2pred", "max_gt2pred", "max_p2s", "n", "normal_consistency", "p2s"]
    for key in ("HR", "LR"):
        assert sorted(plain[key]) == today
        assert sorted(got[key]) == sorted(today + ["normal_error", "normal_per_view", "mask_iou"])
        assert {k: got[key][k] for k in today} == plain[key]                               # the same bits
        print("%s: normal_error %.3e, per view %r, mask_iou %.6f" % (key, got[key]["normal_error"], got[key]["normal_per_view"],
                                                                     got[key]["mask_iou"]))
        assert got[key]["normal_error"] == 0 and got[key]["mask_iou"] == 1 and len(got[key]["normal_per_view"]) == 4   # scored against itself
    # the reconstruction is seen in the item's own image: the first view's mask is not empty
    from surs_amd import native
    mask = native.normal_map(native.Mesh(*gt_hr), data["calib"][0], 64)[1]
    assert 50 < int(mask.sum()) < 64 * 64
    with pytest.raises(ValueError, match="calib"):
        train_util.gen_mesh_metrics(opt, net, g.dev(), {k: v for k, v in data.items() if k != "calib"}, use_octree=False, n=100,
                                    gt_hr=gt_hr, gt_lr=gt_lr, normal_views=(0,))


# ---------------------------------------------------------------- 4. volume
def test_volume_two_parts_at_the_default_part_size():
    """A fine torus of 2 x 182 x 182 = 66 248 faces at 96 x 96: the one test with more than one part at the DEFAULT raster_part
    (65 536)."""
    from surs_amd import _lib, native
    mesh = mr.torus(182, 182)
    assert len(mesh[1]) == 66248 and native.get_option("raster_part") == 65536 and _lib.lib().surs_mesh_raster_parts(66248) == 2
    view = rr._f32((rr.base_calib() @ rr.tilt(50))[:3])
    want = native.mesh_raster_host(mesh[0], mesh[1], view, 96)
    m = native.Mesh(*mesh)
    got = native.mesh_raster(m, view, 96, want_depth=True, want_bary=True)
    assert _same([a.cpu().numpy() for a in got], want)
    assert (want[0] >= 65536).sum() >= 5 and ((want[0] >= 0) & (want[0] < 65536)).sum() > 1000           # both parts win pixels
    flat, mask = native.normal_map(m, view, 96)
    assert _same([flat.cpu().numpy()], [native.normal_map_host(mesh[0], mesh[1], view, 96)[0]])
