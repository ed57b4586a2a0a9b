"""Host checks of surs_amd/render.py and apps/render_data.py: the light-side rotation, the seeded draws, the OBJ reader, and the one
contract that matters to training - data.TrainDataset must read back a calib that projects the mesh onto the pixels where the
renderer put it.  Everything runs the library's host twins (device='cpu').  No GPU."""
import os

import numpy as np
import pytest

import prt_ref as pr
import render_ref as rr
import train_data_common as tdc
from surs_amd import data, native, render
from surs_amd.apps import render_data


def _rotations(n, seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rs.randn(3, 3))
        q = q * np.sign(np.diag(r))
        out.append(q * np.sign(np.linalg.det(q)))
    return out


def test_sh_rotate_is_the_rotation_of_the_lighting():
    rs = np.random.RandomState(1)
    d = rs.randn(64, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for R in _rotations(16, 2):
        c = rs.randn(9, 3)
        got = pr.sh9(d) @ render.sh_rotate(c, R)
        want = pr.sh9(d @ R) @ c                              # rows (R^T d)^T
        assert np.abs(got - want).max() <= 1e-12
    c = rs.randn(9, 3)
    assert np.abs(render.sh_rotate(c, np.identity(3)) - c).max() <= 1e-14
    M = render.sh_rotation_matrix(_rotations(1, 3)[0])
    # orthogonal band by band - as far as the basis' six-digit constants are orthonormal (band 2's three differ in the 7th digit)
    assert np.abs(M @ M.T - np.identity(9)).max() <= 1e-5
    assert np.all(M[0, 1:] == 0) and np.all(M[1:4, 4:] == 0) and np.all(M[4:, :4] == 0)


def test_light_side_rotation_equals_vertex_side():
    """Rotating the light into the mesh's frame, sh_rotate(light, R^T), gives the shading of rotating the transfer vector into the
    camera's: for the analytic transfer p(n) = A_l Y(n) that is p(n) . L' = p(R n) . L."""
    rs = np.random.RandomState(4)
    n = rs.randn(32, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    for R in _rotations(4, 5):
        light = rs.rand(9, 3)
        assert np.abs(pr.closed_form(n) @ render.sh_rotate(light, R.T) - pr.closed_form(n @ R.T) @ light).max() <= 1e-12


def test_seeded_draws_are_pure_functions():
    a, b = render.sample_light(7), render.sample_light(7)
    assert a.shape == (9, 3) and np.array_equal(a, b) and not np.array_equal(a, render.sample_light(8))
    assert np.all(a[0] == 0.8) and np.all((a[1:] >= 0) & (a[1:] < 1))
    env = np.random.RandomState(0).rand(5, 9, 3)
    a = render.sample_light(11, env)
    assert np.array_equal(a, render.sample_light(11, env))
    # one of the entries, turned about the up axis by at most 0.1 pi: band 0 and the up-axis (m = 0) rows do not move
    k = [i for i in range(5) if np.allclose(a[0], env[i, 0], atol=1e-12)]
    assert len(k) == 1 and np.allclose(a[1], env[k[0], 1], atol=1e-12) and not np.allclose(a[3], env[k[0], 3], atol=1e-9)
    assert np.allclose(np.linalg.norm(a[1:4], axis=0), np.linalg.norm(env[k[0], 1:4], axis=0), atol=1e-12)
    assert np.array_equal(render.prt_directions(6, 3), render.prt_directions(6, 3))
    assert not np.array_equal(render.prt_directions(6, 3), render.prt_directions(6, 4))


OBJ = """# a quad, a triangle with negative indices, a/b/c corners
mtllib scan.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 2 0 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 0.25
vn 0 0 1
usemtl skin
f 1/1 2/2 3/3 4/4
f -1/-1/1 -4/2/1 3/-3/1
"""


def test_load_textured_obj(tmp_path):
    p = tmp_path / "scan.obj"
    p.write_text(OBJ)
    v, f, uv, fuv = render.load_textured_obj(str(p))
    assert v.shape == (5, 3) and uv.shape == (5, 2) and f.dtype == np.int32 and fuv.dtype == np.int32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 1, 2]]
    assert fuv.tolist() == [[0, 1, 2], [0, 2, 3], [4, 1, 2]]
    assert uv[4].tolist() == [0.5, 0.25]
    from surs_amd import mesh_util
    v0, f0 = mesh_util.load_obj_mesh(str(p))                  # the plain reader is untouched and agrees
    assert np.array_equal(v0, v) and np.array_equal(f0, f)
    (tmp_path / "two.obj").write_text(OBJ + "usemtl cloth\nf 1/1 2/2 3/3\n")
    with pytest.raises(ValueError, match="multi-material"):
        render.load_textured_obj(str(tmp_path / "two.obj"))
    (tmp_path / "bare.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="texture index"):
        render.load_textured_obj(str(tmp_path / "bare.obj"))
    (tmp_path / "range.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/2\n")
    with pytest.raises(ValueError, match="out of range"):
        render.load_textured_obj(str(tmp_path / "range.obj"))


def test_subject_frame_and_view_param():
    v = np.array([[0.0, 10, 0], [2, 30, 4], [1, 20, 9], [7, 12, 1], [3, 28, 2]])
    center, scale = render.subject_frame(v)
    assert center.tolist() == [2.0, 20.0, 2.0] and scale == 180.0 / 20.0
    param, calib = render.view_param(90, 0, 64, center, scale)
    assert param["ortho_ratio"] == 0.4 * 512 / 64 and sorted(param) == ["R", "center", "ortho_ratio", "scale"]
    assert np.allclose(param["R"], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-15)
    assert calib.dtype == np.float32 and calib.shape == (4, 4)
    # the subject's height fills 180 / (0.4 * 512) of the image's: its top lands on y' = -0.8789 (y' grows downwards)
    top = calib @ np.array([center[0], 30.0, center[2], 1.0])
    assert abs(top[1] + 90.0 / 102.4) < 1e-6 and abs(top[0]) < 1e-6
    param, _ = render.view_param(0, 30, 64, center, scale)
    assert np.allclose(param["R"], render._rot_axis(0, np.pi / 6))


# ---------------------------------------------------------------- the round trip
SIZE, MS, YAWS = 64, 2, (0, 90, 180, 270)


def _write_textured_obj(path, v, f, uvs, fuv):
    with open(path, "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in v))
        fh.write("".join("vt %r %r\n" % tuple(float(x) for x in p) for p in uvs))
        fh.write("".join("f %d/%d %d/%d %d/%d\n" % (a + 1, ta + 1, b + 1, tb + 1, c + 1, tc + 1) for (a, b, c), (ta, tb, tc) in zip(f, fuv)))


@pytest.fixture(scope="module")
def rendered():
    """The textured torus rendered on the host at size 64, ms 2, four yaws: computed once, never changed."""
    v, f, n, uvs, fuv = rr.torus_uv()
    tex = rr.texture(64, 32, 5)
    sub = render.Subject((v, f, uvs, fuv), tex, "cpu")
    prt = sub.prt(render.prt_directions(6, 0))
    center, scale = render.subject_frame(v)
    views = [render.view_param(y, 0, SIZE, center, scale) for y in YAWS]
    lights = np.stack([render.sample_light(100 + y) for y in YAWS])
    images, masks = render.render_views(sub, None, prt, [p for p, _ in views], lights, SIZE, ms=MS)
    return dict(v=v, f=f, uvs=uvs, fuv=fuv, tex=tex, prt=prt, views=views, lights=lights, images=images, masks=masks)


def test_round_trip_through_the_dataset(rendered, tmp_path):
    """render_views -> the app's writer -> data.TrainDataset(phase='test').  For every view: the item's calib equals view_param's bit
    for bit; every surface point the renderer's raster (size * ms) put on a sub-pixel - the winner's corners blended by its
    barycentrics, a vertex itself where its weight is 1 - projects with the ITEM's calib onto that sub-pixel (within a thousandth of
    a pixel: the contract is 'within one pixel', the arithmetic gives this); and the dataset's mask is non-zero there."""
    from PIL import Image
    r = rendered
    root = str(tmp_path / "dataroot")
    name = tdc.SUBJECTS[1]
    for (param, _), y, image, mask, light in zip(r["views"], YAWS, r["images"], r["masks"], r["lights"]):
        render.write_view(root, name, y, 0, image, mask, param, light)
    os.makedirs(os.path.join(root, "GEO", "OBJ"))
    for tag in ("_HR", "_LR"):
        tdc.write_obj(os.path.join(root, "GEO", "OBJ", name + tag + ".obj"), r["v"], r["f"])
    with open(os.path.join(root, "val.txt"), "w") as fh:
        fh.write(name + "\n")
    ds = data.TrainDataset(tdc.opt(root, size=SIZE), phase="test")
    assert ds.subjects == [name]
    assert r["masks"].max() == 255 and (r["masks"] > 0).mean() > 0.1 and r["images"][r["masks"] == 0].max() == 0
    for (param, calib), y, mask in zip(r["views"], YAWS, r["masks"]):
        item = ds.get_render(name, 1, yid=y)
        got = item["calib"][0].numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), calib.view(np.uint32))
        assert item["img_HR"].shape[-2:] == (SIZE, SIZE)
        stored = np.load(os.path.join(root, "PARAM", name, "%d_0_00.npy" % y), allow_pickle=True).item()
        assert sorted(stored) == ["R", "center", "ortho_ratio", "scale", "sh"] and stored["sh"].shape == (9, 3)
        ds_mask = np.asarray(Image.open(os.path.join(root, "MASK", name, "%d_0_00.png" % y)).convert("L"))
        assert np.array_equal(ds_mask, mask)
        big = SIZE * MS
        face, _, bary = native.mesh_raster_host(r["v"], r["f"], calib, big)
        sy, sx = np.nonzero(face >= 0)
        assert len(sy) > 2000
        idx = np.sort(r["f"][face[sy, sx]], axis=1)
        b1, b2 = bary[sy, sx].astype(np.float64).T
        wgt = np.stack([1 - b1 - b2, b1, b2], 1)
        point = (wgt[:, :, None] * r["v"][idx]).sum(1)
        project = lambda p: (np.c_[p, np.ones(len(p))] @ got.astype(np.float64).T)[:, :2]
        px = (project(point) + 1) * (SIZE / 2.0) - 0.5                      # the dataset's pixels: x' = (2 j + 1) / size - 1
        want = np.stack([(sx + 0.5) / MS - 0.5, (sy + 0.5) / MS - 0.5], 1)
        assert np.abs(px - want).max() <= 1e-3
        assert np.all(ds_mask[sy // MS, sx // MS] > 0)
        # and the picture is where the mask is: lit, textured pixels inside, black outside
        img = np.asarray(Image.open(os.path.join(root, "RENDER", name, "%d_0_00.jpg" % y)).convert("RGB"))
        assert img[ds_mask == 255].mean() > 20 and img[ds_mask == 0].mean() < 3


def test_render_views_variants(rendered):
    """Untextured and analytic renders share the mask; a single light broadcasts.  On a convex mesh (nothing occluded) the PRT render
    - light turned into the mesh's frame - and the analytic render - normals turned into the camera's - are the same picture up
    to the PRT's sampling error (n = 40: a few per cent of a coefficient, so a few bytes), in a view whose R is no identity."""
    r = rendered
    params = [p for p, _ in r["views"][:1]]
    plain, m1 = render.render_views((r["v"], r["f"]), None, r["prt"], params, r["lights"][0], SIZE, ms=MS, device="cpu")
    analytic, m2 = render.render_views((r["v"], r["f"]), None, None, params, r["lights"][0], SIZE, ms=MS, device="cpu")
    assert np.array_equal(m1, r["masks"][:1]) and np.array_equal(m2, m1)
    assert plain.shape == (1, SIZE, SIZE, 3)
    v, f, _ = pr.icosphere(2)
    sub = render.Subject((v, f), None, "cpu")
    param = render.view_param(70, 20, SIZE, *render.subject_frame(v))[0]
    light = 0.4 * render.sample_light(5)
    a, ma = render.render_views(sub, None, sub.prt(), [param], light, SIZE, ms=1)
    b, mb = render.render_views(sub, None, None, [param], light, SIZE, ms=1)
    assert np.array_equal(ma, mb) and (ma == 255).mean() > 0.3
    gap = np.abs(a.astype(int) - b.astype(int))[ma == 255]
    print("PRT against analytic on the icosphere: mean %.2f, max %d bytes" % (gap.mean(), gap.max()))
    # (the gamma is steep at 0: a dark pixel turns a small gap in the shading into many bytes - hence a mean and a percentile)
    assert 100 < np.ptp(b[mb == 255].astype(int)) and gap.mean() <= 3.0 and np.percentile(gap, 99) <= 8
    with pytest.raises(ValueError):
        render.render_views((r["v"], r["f"]), r["tex"], None, params, r["lights"][0], SIZE, device="cpu")      # texture without uvs


# ---------------------------------------------------------------- the app
def test_app_writes_resumes_and_reports(rendered, tmp_path, capsys):
    from PIL import Image
    r = rendered
    scans, root = tmp_path / "scans", str(tmp_path / "out")
    os.makedirs(scans / "ring")
    _write_textured_obj(str(scans / "ring" / "ring.obj"), r["v"], r["f"], r["uvs"], r["fuv"])
    Image.fromarray(r["tex"]).save(str(scans / "ring" / "ring.png"))
    _write_textured_obj(str(scans / "solo.obj"), r["v"], r["f"], r["uvs"], r["fuv"])
    Image.fromarray(r["tex"]).save(str(scans / "solo.png"))
    tdc.write_obj(str(scans / "solo_LR.obj"), r["v"], r["f"])
    args = ["-i", str(scans), "-o", root, "--size", "32", "--yaws", "0:360:90", "--n_prt", "4", "--device", "cpu", "--prt_cache",
            str(tmp_path / "cache"), "--seed", "3"]
    assert render_data.main(args) == 8
    out = capsys.readouterr().out
    miss = [l for l in out.splitlines() if "training will miss" in l]
    assert len(miss) == 1 and miss[0].startswith("ring:") and os.path.join(root, "GEO", "OBJ", "ring_LR.obj") in miss[0]
    want = sorted("%d_0_00" % y for y in (0, 90, 180, 270))
    for name in ("ring", "solo"):
        for folder, ext in (("RENDER", ".jpg"), ("MASK", ".png"), ("PARAM", ".npy")):
            assert sorted(os.listdir(os.path.join(root, folder, name))) == [s + ext for s in want]
        assert os.path.isfile(os.path.join(root, "GEO", "OBJ", name + "_HR.obj"))
    assert os.path.isfile(os.path.join(root, "GEO", "OBJ", "solo_LR.obj")) and not os.path.exists(os.path.join(root, "GEO", "OBJ", "ring_LR.obj"))
    assert sorted(os.listdir(tmp_path / "cache")) == ["ring_n4_s3.npy", "solo_n4_s3.npy"]
    assert Image.open(os.path.join(root, "RENDER", "ring", "90_0_00.jpg")).size == (32, 32)
    # resume: nothing to do; then one view removed is the one view written again, with the same bytes
    stamp = {p: os.path.getmtime(p) for p in (os.path.join(root, "MASK", "ring", s + ".png") for s in want)}
    assert render_data.main(args) == 0
    victim = os.path.join(root, "MASK", "ring", "180_0_00.png")
    before = open(victim, "rb").read()
    os.remove(victim)
    assert render_data.main(args) == 1
    assert open(victim, "rb").read() == before
    assert all(os.path.getmtime(p) == t for p, t in stamp.items() if p != victim)
    capsys.readouterr()
    assert render_data.parse_yaws("0:360:120") == [0, 120, 240] and render_data.parse_yaws("5,7") == [5, 7]
