"""Float64 model of the colour shading (include/surs.h "mesh shading"), written from its statement in plain numpy: the texture pyramid,
the trilinear lookup with its per-face level, spherical-harmonic shading, gamma and the box resolve; plus the scenes the shading
tests share.  Real log2 and power functions here: the product's polynomial ones are held to these."""
import numpy as np

import prt_ref as pr

EPS = 2.0 ** -24
QUAD_VIEW = np.array([[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, 1.0, 0]])


def pyramid(tex):
    """[level 0 .. 3] float64 arrays [h >> l, w >> l, 3]: u8 / 255 and the 2 x 2 means."""
    lv = [np.asarray(tex, np.float64) / 255.0]
    for _ in range(3):
        a = lv[-1]
        lv.append(a.reshape(a.shape[0] // 2, 2, a.shape[1] // 2, 2, 3).mean((1, 3)))
    return lv


def bilinear(level, u, v):
    """level [H, W, 3] at uv (arrays): texel centres at (i + 0.5) / size, v = 0 the LAST row, clamp to edge."""
    H, W = level.shape[:2]
    x, y = u * W - 0.5, (1.0 - v) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    xa, xb = np.clip(x0, 0, W - 1).astype(int), np.clip(x0 + 1, 0, W - 1).astype(int)
    ya, yb = np.clip(y0, 0, H - 1).astype(int), np.clip(y0 + 1, 0, H - 1).astype(int)
    top = level[ya, xa] * (1 - fx) + level[ya, xb] * fx
    bot = level[yb, xa] * (1 - fx) + level[yb, xb] * fx
    return top * (1 - fy) + bot * fy


def trilinear(levels, u, v, lam):
    lam = np.clip(lam, 0.0, 3.0)
    lo = np.minimum(np.floor(lam), 2).astype(int)
    frac = (lam - lo)[:, None]
    out = np.zeros((len(u), 3))
    for l in range(3):
        m = lo == l
        if m.any():
            out[m] = bilinear(levels[l], u[m], v[m]) * (1 - frac[m]) + bilinear(levels[l + 1], u[m], v[m]) * frac[m]
    return out


def pixel_coords(verts, view, w, h):
    p = np.asarray(verts, np.float64) @ np.asarray(view, np.float64)[:3, :3].T + np.asarray(view, np.float64)[:3, 3]
    return np.stack([(p[:, 0] + 1) * (w / 2.0) - 0.5, (p[:, 1] + 1) * (h / 2.0) - 0.5], -1)


def shade(face, bary, verts, faces, view, light, prt=None, normals=None, normal_matrix=None, levels=None, faces_uv=None, uvs=None):
    """dict of float64 arrays over the image: shading [h,w,3] (before the gamma), rgba [h,w,4], albedo [h,w,3], lam [h,w] (the
    face's level), a_pix [h,w] and edge [h,w] (its projected area and longest projected edge in pixels)."""
    face = np.asarray(face)
    h, w = face.shape
    cov = face >= 0
    fi = face[cov]
    b1, b2 = np.asarray(bary, np.float64)[cov].T
    b0 = 1.0 - b1 - b2
    corners = np.asarray(faces)[fi]
    order = np.argsort(corners, axis=1, kind="stable")
    idx = np.take_along_axis(corners, order, 1)
    blend = lambda a: b0[:, None] * a[idx[:, 0]] + b1[:, None] * a[idx[:, 1]] + b2[:, None] * a[idx[:, 2]]
    out = {k: np.zeros((h, w, 3)) for k in ("shading", "albedo")}
    out.update(rgba=np.zeros((h, w, 4)), lam=np.zeros((h, w)), a_pix=np.zeros((h, w)), edge=np.zeros((h, w)))
    albedo = np.ones((len(fi), 3))
    if levels is not None:
        th, tw = levels[0].shape[:2]
        uvi = np.take_along_axis(np.asarray(faces_uv)[fi], order, 1)
        t = np.asarray(uvs, np.float64)[uvi]
        uv = b0[:, None] * t[:, 0] + b1[:, None] * t[:, 1] + b2[:, None] * t[:, 2]
        e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        a_tex = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) * tw * th
        q = pixel_coords(verts, view, w, h)[idx]
        d1, d2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        a_pix = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = np.where(a_tex > a_pix, np.clip(0.5 * np.log2(a_tex / a_pix), 0.0, 3.0), 0.0)
        albedo = trilinear(levels, uv[:, 0], uv[:, 1], lam)
        out["lam"][cov], out["a_pix"][cov] = lam, a_pix
        out["edge"][cov] = np.maximum(np.maximum(np.linalg.norm(d1, axis=1), np.linalg.norm(d2, axis=1)), np.linalg.norm(d2 - d1, axis=1))
    if prt is not None:
        p = blend(np.asarray(prt, np.float64))
    else:
        n = blend(np.asarray(normals, np.float64)) @ np.asarray(normal_matrix, np.float64).T
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        p = pr.closed_form(n)
    s = p @ np.asarray(light, np.float64)
    g = np.maximum(s, 0.0) ** (1.0 / 2.2)
    out["shading"][cov], out["albedo"][cov] = s, albedo
    out["rgba"][cov] = np.concatenate([np.clip(albedo * g, 0.0, 1.0), np.ones((len(fi), 1))], 1)
    return out


def resolve(rgba, m):
    """(bytes uint8 [h,w,4], value float64 [h,w,4] = 255 x the mean of the m x m sub-samples): round to nearest, ties to even."""
    a = np.asarray(rgba, np.float64)
    h, w = a.shape[0] // m, a.shape[1] // m
    val = 255.0 * a.reshape(h, m, w, m, 4).mean((1, 3))
    return np.clip(np.rint(val), 0, 255).astype(np.uint8), val


def near_tie(val, width=1e-3):
    """Where 255 x mean lies within `width` of a rounding tie (k + 1/2)."""
    return np.abs(val - np.floor(val) - 0.5) < width


# ---------------------------------------------------------------- scenes
def quad():
    """The square [-1, 1]^2 at z = 0 through QUAD_VIEW fills the image; uv (0, 0) at its lower left (x = -1, y = -1: the image's
    LAST row).  Returns (verts, faces, uvs, faces_uv, normals); the faces list their corners in other orders than ascending."""
    v = np.array([[-1.0, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]])
    uv = np.array([[1.0, 1], [0, 1], [0, 0], [1, 0]])          # uv index k is NOT vertex k: 2 <-> 0, 3 <-> 1
    f = np.array([[2, 0, 1], [3, 0, 2]], np.int32)
    fuv = np.array([[0, 2, 3], [1, 2, 0]], np.int32)
    return v, f, uv, fuv, np.tile([0.0, 0.0, 1.0], (4, 1))


def quad_uv(w, h):
    """The uv of every pixel centre of the quad scene: u = (j + 0.5) / w, v = 1 - (i + 0.5) / h."""
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    return (j + 0.5) / w, 1.0 - (i + 0.5) / h


def torus_uv(nu=24, nv=12):
    """The torus with one uv per vertex and a seam-free (wrapping ignored) unwrap: (verts, faces, normals, uvs, faces_uv)."""
    v, f, n = pr.torus_scene(nu, nv)
    k = np.arange(len(v))
    uvs = np.stack([(k // nv + 0.5) / nu, (k % nv + 0.5) / nv], -1)
    return v, f, n, uvs, f.copy()


def torus_view(w, h, yaw=0.4):
    """An orthographic calib-like view of the torus (centre (0, 100, 0), radius about 90): y' down, larger z' nearer."""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]])
    k = 1.0 / 100.0
    M = np.diag([k, -k, k]) @ R
    t = -M @ np.array([0.0, 100.0, 0.0])
    return np.concatenate([M, t[:, None]], 1).astype(np.float32).astype(np.float64)


def texture(w, h, seed=0, kind="noise"):
    rs = np.random.RandomState(seed)
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "hramp":
        t = x * (256 // w)
    elif kind == "vramp":
        t = y * (256 // h)
    else:                                   # checker of single texels
        t = ((x + y) % 2) * 255
    return np.repeat(t[..., None], 3, 2).astype(np.uint8)
