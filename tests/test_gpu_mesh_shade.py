"""GPU checks of the shading kernels (csrc/surs_mesh_shade.hip): the pyramid, surs_mesh_shade_prt (textured, untextured, analytic)
and the resolve against their host twins BIT FOR BIT - the same header looped on the host, which tests/test_mesh_shade_host.py holds
to the float64 model tests/render_ref.py - and render.render_views on the device against device='cpu', byte for byte."""
import numpy as np
import pytest
import torch

import render_ref as rr

pytestmark = pytest.mark.gpu

LIGHT = np.array([[0.8, 0.7, 0.9], [0.3, 0.1, 0.2], [0.5, 0.4, 0.1], [0.2, 0.6, 0.3], [0.1, 0.2, 0.5], [0.4, 0.1, 0.1],
                  [0.3, 0.3, 0.2], [0.2, 0.5, 0.4], [0.1, 0.1, 0.6]])
SIZES = {"33x47": (33, 47), "64x64": (64, 64)}           # (h, w)
TEXTURES = {"8x16": (8, 16, 1), "64x32": (64, 32, 2)}    # (w, h, seed)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def scene():
    """The torus with uvs, its host PRT at n = 6 and its device mesh: shared, never changed."""
    from surs_amd import native, render
    v, f, n, uvs, fuv = rr.torus_uv()
    prt = native.mesh_prt_host(v, f, n, render.prt_directions(6, 0), 0.5)
    return dict(v=v, f=f, n=n.astype(np.float32), uvs=uvs.astype(np.float32), fuv=fuv, prt=prt, mesh=native.Mesh(v, f))


@pytest.mark.parametrize("tex", sorted(TEXTURES))
def test_pyramid_is_the_host_loop(tex):
    from surs_amd import native
    w, h, seed = TEXTURES[tex]
    img = rr.texture(w, h, seed)
    want = native.texture_pyramid(img, host=True)
    got = native.texture_pyramid(img)
    assert (got.w, got.h) == (w, h) and got.levels.numel() == want.levels.size
    assert np.array_equal(_bits(got.levels.cpu().numpy()), _bits(want.levels))


@pytest.mark.parametrize("tex", sorted(TEXTURES))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_shade_is_the_host_loop(scene, size, tex):
    """Textured, untextured and analytic, on the host raster's face / bary (the raster's own parity is tests/test_gpu_mesh_raster.py)."""
    from surs_amd import native
    c = scene
    h, w = SIZES[size]
    tw, th, seed = TEXTURES[tex]
    view = rr.torus_view(w, h)
    face, _, bary = native.mesh_raster_host(c["v"], c["f"], view, (h, w))
    assert (face >= 0).sum() > 200
    img = rr.texture(tw, th, seed)
    t_host, t_dev = native.texture_pyramid(img, host=True), native.texture_pyramid(img)
    dev = c["mesh"].verts.device
    face_d, bary_d = torch.from_numpy(face).to(dev), torch.from_numpy(bary).to(dev)
    nm = np.asarray(view, np.float64)[:3, :3]
    nm = nm / np.linalg.norm(nm[0])
    variants = {
        "textured": (dict(prt=c["prt"]), True),
        "untextured": (dict(prt=c["prt"]), False),
        "analytic": (dict(normals=c["n"], normal_matrix=nm), tex == "8x16"),
    }
    for name, (how, textured) in variants.items():
        th_kw = dict(texture=t_host, faces_uv=c["fuv"], uvs=c["uvs"]) if textured else {}
        td_kw = dict(texture=t_dev, faces_uv=c["fuv"], uvs=c["uvs"]) if textured else {}
        want = native.mesh_shade_prt_host(c["v"], c["f"], view, face, bary, LIGHT, **how, **th_kw)
        got = native.mesh_shade_prt(c["mesh"], view, face_d, bary_d, LIGHT, **how, **td_kw)
        assert got.shape == (h, w, 4)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), name
        assert want[face >= 0][:, :3].max() > 0.2 and np.all(want[face < 0] == 0)


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_resolve_is_the_host_loop(scene, size, m):
    from surs_amd import native
    c = scene
    h, w = SIZES[size]
    view = rr.torus_view(w * m, h * m)
    face, _, bary = native.mesh_raster_host(c["v"], c["f"], view, (h * m, w * m))
    rgba = native.mesh_shade_prt_host(c["v"], c["f"], view, face, bary, LIGHT, prt=c["prt"])
    want_rgb, want_mask = native.image_resolve(rgba, m, host=True)
    rgb, mask = native.image_resolve(torch.from_numpy(rgba).to(c["mesh"].verts.device), m)
    assert rgb.shape == (h, w, 3) and mask.shape == (h, w) and rgb.dtype == torch.uint8
    assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(mask.cpu().numpy(), want_mask)
    assert 0 < (want_mask == 255).mean() < 1


def test_render_views_device_equals_cpu(scene):
    """The round trip's render - textured torus, size 64, ms 2, yaws 0 / 90 / 180 / 270, PRT lighting - byte for byte; and the
    analytic, untextured variant."""
    from surs_amd import render
    c = scene
    tex = rr.texture(64, 32, 5)
    mesh = (c["v"], c["f"], c["uvs"], c["fuv"])
    center, scale = render.subject_frame(c["v"])
    params = [render.view_param(y, 0, 64, center, scale)[0] for y in (0, 90, 180, 270)]
    lights = np.stack([render.sample_light(100 + y) for y in (0, 90, 180, 270)])
    dirs = render.prt_directions(6, 0)
    host, dev = render.Subject(mesh, tex, "cpu"), render.Subject(mesh, tex)
    prt_h, prt_d = host.prt(dirs), dev.prt(dirs)
    assert np.array_equal(_bits(prt_d.cpu().numpy()), _bits(prt_h))
    want = render.render_views(host, None, prt_h, params, lights, 64, ms=2)
    got = render.render_views(dev, None, prt_d, params, lights, 64, ms=2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1].max() == 255 and want[0].max() > 100
    want = render.render_views((c["v"], c["f"]), None, None, params[:2], lights[0], 64, ms=2, device="cpu")
    got = render.render_views((c["v"], c["f"]), None, None, params[:2], lights[0], 64, ms=2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
