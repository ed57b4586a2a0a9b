"""Host checks of the colour shading (csrc/surs_mesh_shade.h through the _host entries, the kernels' twins) against the float64 model
tests/render_ref.py and closed forms: the pyramid, the texture lookup's conventions, shading / gamma / colour on the raster's own
output, the analytic branch, the 8-bit resolve.  No GPU."""
import numpy as np
import pytest

import prt_ref as pr
import render_ref as rr
from surs_amd import _lib, native, render

EPS = rr.EPS
LIGHT = np.array([[0.8, 0.7, 0.9], [0.3, 0.1, 0.2], [0.5, 0.4, 0.1], [0.2, 0.6, 0.3], [0.1, 0.2, 0.5], [0.4, 0.1, 0.1],
                  [0.3, 0.3, 0.2], [0.2, 0.5, 0.4], [0.1, 0.1, 0.6]]).astype(np.float32).astype(np.float64)
# what sh_gamma's own arithmetic may cost a value, relative: the exponent 0.4545 log2 s is off by at most 0.4545 (|log2 s| 3 eps +
# 4e-10 + 5 eps) <= 1e-6 for s in [1e-3, 1e3] (|log2 s| <= 10), which is 7e-7 of the value; the exp2 series' tail is 1.3e-7 and its
# seven steps round to 5e-7 more
GAMMA_REL = 2e-6


def test_pyramid_levels_are_numpy_means():
    for w, h, seed in ((8, 16, 1), (64, 32, 2)):
        tex = rr.texture(w, h, seed)
        t = native.texture_pyramid(tex, host=True)
        want = rr.pyramid(tex)
        assert t.levels.size == _lib.lib().surs_texture_pyramid_floats(w, h) == sum(x.size for x in want)
        for l in range(4):
            assert t.level(l).shape == want[l].shape
            assert np.abs(t.level(l) - want[l]).max() <= 4 * EPS
        assert np.array_equal(t.level(0), (tex.astype(np.float32) / np.float32(255.0)))
    for w, h in ((12, 16), (16, 4), (0, 8), (16392, 8)):
        with pytest.raises(_lib.SursError):
            native.texture_pyramid(np.zeros((max(h, 1), max(w, 1), 3), np.uint8)[:h, :w], host=True)
        assert _lib.lib().surs_texture_pyramid_floats(w, h) == 0


def _quad_render(tex, w, h):
    """(textured rgba, untextured rgba, the twin's pyramid) of the quad scene under an ambient light, analytic branch."""
    v, f, uv, fuv, n = rr.quad()
    face, _, bary = native.mesh_raster_host(v, f, rr.QUAD_VIEW, (h, w))
    assert (face >= 0).all()
    light = np.zeros((9, 3))
    light[0] = 1.0
    t = native.texture_pyramid(tex, host=True)
    kw = dict(normals=n, normal_matrix=np.identity(3))
    plain = native.mesh_shade_prt_host(v, f, rr.QUAD_VIEW, face, bary, light, **kw)
    tx = native.mesh_shade_prt_host(v, f, rr.QUAD_VIEW, face, bary, light, texture=t, faces_uv=fuv, uvs=uv, **kw)
    return tx, plain, t


@pytest.mark.parametrize("kind", ["hramp", "vramp", "checker"])
def test_texture_lookup_conventions(kind):
    """A texture of 8 x 16 texels on the quad at 32 x 32 pixels (more pixels than texels: level 0).  The horizontal ramp pins the
    texel centres and the clamp (value = clip(8 u - 0.5, 0, 7) * 32 / 255), the vertical ramp the v flip (row 0 is v = 1), the
    checker the bilinear weights against the model.  The albedo is read as rgba over the untextured render's (the same gamma bits)."""
    w = h = 32
    tex = rr.texture(8, 16, kind=kind)
    tx, plain, _ = _quad_render(tex, w, h)
    assert np.all(plain[..., :3] > 0.5) and np.all(plain[..., 3] == 1)
    u, v = rr.quad_uv(w, h)
    if kind == "hramp":
        want = np.clip(8 * u - 0.5, 0, 7) * 32 / 255
    elif kind == "vramp":
        want = np.clip(16 * (1 - v) - 0.5, 0, 15) * 16 / 255
    else:
        want = rr.bilinear(rr.pyramid(tex)[0], u.ravel(), v.ravel())[:, 0].reshape(h, w)
    got = tx[..., :3].astype(np.float64) / plain[..., :3]
    # uv is a blend of three fp32 products (4 eps), scaled by up to 16 texels, on a texture whose steps are at most 1
    assert np.abs(got - want[..., None]).max() <= 16 * 8 * EPS + 4 * EPS
    assert np.all(tx[..., 3] == 1)


def test_mip_level_blends_levels():
    """64 x 32 texels on 8 x 8 pixels: A_tex / A_pix = 32, lambda = 2.5, an even blend of levels 2 and 3; on 16 x 16 pixels
    lambda = 1.5; on 4 x 4 pixels the ratio is 128 and lambda clamps to 3."""
    tex = rr.texture(64, 32, 7)
    lv = rr.pyramid(tex)
    for size, lam in ((8, 2.5), (16, 1.5), (4, 3.0)):
        tx, plain, _ = _quad_render(tex, size, size)
        u, v = rr.quad_uv(size, size)
        want = rr.trilinear(lv, u.ravel(), v.ravel(), np.full(u.size, lam)).reshape(size, size, 3)
        got = tx[..., :3].astype(np.float64) / plain[..., :3]
        assert np.abs(got - want).max() <= 1e-5


@pytest.fixture(scope="module")
def torus_case():
    """The raster's own face / bary of a 48 x 40 view of the torus, its PRT at n = 8, a 64 x 32 texture: shared, never changed."""
    w, h = 48, 40
    v, f, n, uvs, fuv = rr.torus_uv()
    view = rr.torus_view(w, h)
    face, _, bary = native.mesh_raster_host(v, f, view, (h, w))
    prt = native.mesh_prt_host(v, f, n, render.prt_directions(8, 0), 0.5)
    tex = rr.texture(64, 32, 11)
    return dict(w=w, h=h, v=v, f=f, n=n, uvs=uvs.astype(np.float32), fuv=fuv, view=view, face=face, bary=bary, prt=prt, tex=tex,
                pyr=native.texture_pyramid(tex, host=True))


def _shading_bound(p_max, l_max):
    """s = nine fma of p_i light_i: each p_i a blend of three products (5 roundings of at most p_max), nine sums of partials of at
    most 9 p_max l_max at one rounding each."""
    return EPS * p_max * l_max * (9 * 5 + 81)


def _check_colour(c, got, shading, model, textured):
    cov = c["face"] >= 0
    assert cov.sum() > 300 and (~cov).sum() > 100
    assert np.all(got[~cov] == 0)                                            # background: exactly (0, 0, 0, 0)
    assert np.all(got[cov][:, 3] == 1)
    p_max = np.abs(c["prt"]).max() if model.get("p_max") is None else model["p_max"]
    sb = _shading_bound(p_max, LIGHT.max())
    gap = np.abs(shading - model["shading"])[cov].max()
    print("shading gap %.3e (bound %.3e)" % (gap, sb))
    assert gap <= sb
    s = model["shading"]
    lit = cov[..., None] & (s >= 1e-3)
    assert lit.sum() > 0.8 * 3 * cov.sum()
    g = np.maximum(s, 0) ** (1 / 2.2)
    rel = sb / (2.2 * np.maximum(s, 1e-3)) + GAMMA_REL
    tol = model["albedo"] * g * rel + 2 * EPS
    if textured:
        # the albedo: uv off by 4 eps scaled by 64 texels on steps of at most 1, and the level lambda off by 0.75 (the areas'
        # relative errors: the pixel area from coordinates of size S = max(w, h) off by 16 eps each over edges of length E, so
        # 64 eps S E / A_pix) + 2e-6 (the polynomial log2), times a level difference of at most 1
        with np.errstate(divide="ignore", invalid="ignore"):
            dlam = np.where(cov, 0.75 * (64 * EPS * max(c["w"], c["h"]) * model["edge"] / model["a_pix"] + 16 * EPS) + 2e-6, 0.0)
        tol = tol + g * (64 * 8 * EPS + dlam[..., None])
    gap = np.abs(got[..., :3] - model["rgba"][..., :3])
    print("colour gap %.3e where lit" % gap[lit].max())
    assert np.all(gap[lit] <= tol[lit])


@pytest.mark.parametrize("textured", [False, True])
def test_shade_prt_matches_model(torus_case, textured):
    c = torus_case
    tex = dict(texture=c["pyr"], faces_uv=c["fuv"], uvs=c["uvs"]) if textured else {}
    got, shading = native.mesh_shade_prt_host(c["v"], c["f"], c["view"], c["face"], c["bary"], LIGHT, prt=c["prt"], want_shading=True,
                                              **tex)
    ref = dict(levels=[c["pyr"].level(l).astype(np.float64) for l in range(4)], faces_uv=c["fuv"], uvs=c["uvs"]) if textured else {}
    model = rr.shade(c["face"], c["bary"], c["v"], c["f"], c["view"], LIGHT, prt=c["prt"], **ref)
    if textured:
        assert np.ptp(model["lam"][c["face"] >= 0]) > 0.2                    # faces of several levels
    _check_colour(c, got, shading, model, textured)


def test_analytic_branch_matches_closed_form(torus_case):
    """prt = NULL: p = A_l Y_i(n) of the blended, turned, normalised vertex normal - against the closed form in float64."""
    c = torus_case
    nm = np.asarray(c["view"], np.float64)[:3, :3]
    nm = (nm / np.linalg.norm(nm[0])).astype(np.float32).astype(np.float64)      # a rotation with y turned down: still orthonormal
    got, shading = native.mesh_shade_prt_host(c["v"], c["f"], c["view"], c["face"], c["bary"], LIGHT, normals=c["n"], normal_matrix=nm,
                                              want_shading=True)
    model = rr.shade(c["face"], c["bary"], c["v"], c["f"], c["view"], LIGHT, normals=c["n"], normal_matrix=nm)
    # p: the normal's components are off by about 12 roundings (blend, turn, normalise), the band-2 polynomials double that
    model["p_max"] = 4.0 * np.pi * 0.55
    _check_colour(c, got, shading, model, False)
    # and it is the unshadowed limit of the PRT: an ambient-only light gives pi 0.282095 light_0 everywhere
    amb = np.zeros((9, 3))
    amb[0] = 0.5
    _, s = native.mesh_shade_prt_host(c["v"], c["f"], c["view"], c["face"], c["bary"], amb, normals=c["n"], normal_matrix=nm,
                                      want_shading=True)
    assert np.abs(s[c["face"] >= 0] - np.pi * 0.282095 * 0.5).max() <= 4 * EPS


@pytest.mark.parametrize("m", [1, 2, 3])
def test_resolve_rounds_the_box_mean(torus_case, m):
    """The colour bytes equal the float64 model's, except - by one step - where 255 x mean lies within 1e-3 of a rounding tie; at
    most 1 % of the covered pixels may lie there (checked on the model alone).  The mask's bytes are equal everywhere."""
    c = torus_case
    w, h = 128 * m, 96 * m       # (some 4500 covered pixels: the cap is a rate, 0.6 % is what three channels 2e-3 wide expect)
    view = rr.torus_view(w, h)
    face, _, bary = native.mesh_raster_host(c["v"], c["f"], view, (h, w))
    rgba = native.mesh_shade_prt_host(c["v"], c["f"], view, face, bary, LIGHT, prt=c["prt"], texture=c["pyr"], faces_uv=c["fuv"],
                                      uvs=c["uvs"])
    rgb, mask = native.image_resolve(rgba, m, host=True)
    want, val = rr.resolve(rgba, m)
    covered = want[..., 3] > 0
    # the colour channels; the mask is a count of sub-samples over m m - exact on both sides, exact ties (half coverage at m = 2:
    # 127.5 -> 128) included - and must be EQUAL everywhere
    tie = rr.near_tie(val)
    tie[..., 3] = False
    print("m %d: %d covered, %d near a tie" % (m, covered.sum(), tie[covered].any(1).sum()))
    assert covered.sum() > 1000 and tie[covered].any(1).mean() <= 0.01
    got = np.concatenate([rgb, mask[..., None]], 2).astype(int)
    diff = np.abs(got - want.astype(int))
    assert np.all(diff[~tie] == 0) and diff.max() <= 1
    assert np.all(got[~covered] == 0)
    if m == 1:
        assert set(np.unique(mask)) <= {0, 255}
    # ties go to even: 0.5 / 255 x 255 = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    flat = np.zeros((1, 3, 4), np.float32)
    flat[0, :, 0] = np.array([0.5, 1.5, 2.5], np.float32) / np.float32(255.0)
    exact = (flat[0, :, 0].astype(np.float64) * 255.0)
    rgb, _ = native.image_resolve(flat, 1, host=True)
    assert [int(x) for x in rgb[0, :, 0]] == [int(np.rint(np.float32(x) * np.float32(255.0))) for x in flat[0, :, 0]], exact
    for bad in (0, 9):
        with pytest.raises((_lib.SursError, ValueError)):
            native.image_resolve(np.zeros((bad * 2 or 2, bad * 2 or 2, 4), np.float32), bad, host=True)


def test_gamma_polynomials_track_pow():
    """sh_gamma through a one-pixel shade: max(s, 0)^(1 / 2.2) within GAMMA_REL over [1e-3, 1e3], 0 for s <= 0."""
    v, f, uv, fuv, n = rr.quad()
    face, _, bary = native.mesh_raster_host(v, f, rr.QUAD_VIEW, (1, 1))
    k = np.pi * 0.282095
    for s in list(np.geomspace(1e-3, 1e3, 61)) + [0.0, -0.3]:
        light = np.zeros((9, 3))
        light[0] = s / k
        rgba, sh = native.mesh_shade_prt_host(v, f, rr.QUAD_VIEW, face, bary, light, normals=n, normal_matrix=np.identity(3),
                                              want_shading=True)
        s32 = float(sh[0, 0, 0])
        want = min(max(s32, 0.0) ** (1 / 2.2), 1.0)
        assert abs(float(rgba[0, 0, 0]) - want) <= GAMMA_REL * want + (EPS if want == 1.0 else 0.0), (s, rgba[0, 0], want)
