"""Float64 yardstick of the mesh-raster tests (plain numpy, nothing of the product): a brute-force rasteriser over pixel x face,
chunked over the faces, on the meshes of tests/mesh_ref.py, with the fp32 rounding bounds of csrc/surs_mesh_raster.h's arithmetic.

Per pixel it gives the float64 winner (largest z', lowest index among equals, over the faces whose three barycentrics are >= 0) and the
CANDIDATE SET: what an fp32 evaluation of the same formulas may report.

Bounds (counted on the header's operations, in the way mesh_dist_ref.bound counts: roundings x 2^-24 x the largest magnitude).
  W     the largest |pixel-unit coordinate| of the call: over the projected vertices and the image's sides.
  G_k   |a_k| + |c_k|, the L1 norm of barycentric k's gradient per pixel (float64): 1 / (the triangle's height in pixels), so a
        sliver - every triangle near a silhouette - has a large G and a proportionally wide bound.
  tau_k(f) = 2^-24 x 32 x (1 + G_k W).  A barycentric is q . (a, c) with q = pixel - vertex: the vertex's pixel position carries 9
        roundings at magnitude W (6 of the matrix row, 3 of the pixel transform), q one more at 2 W, the edge differences 2, the area
        (two products and a difference, which CANCEL in a sliver: relative error 2^-24 x 2 W G) 4, the reciprocal and the scaled
        coefficient 2, the two products and their sum 3 at magnitude 2 W G: 25 roundings, taken as 32, at magnitude 1 + G W.
  tau_z(f) = 2^-24 x 16 x Z + (tau_1 + tau_2) Dz.  z' = z0 + b1 dz1 + b2 dz2: Z the largest sum of |terms| of a vertex's z' row (6
        roundings for z0, 1 for each difference, 4 for the two products and sums: 12, taken as 16), Dz = max(|dz1|, |dz2|) times the two
        barycentrics' own bounds.
A face is SURE at a pixel where its three barycentrics are >= +tau_k: fp32 covers the pixel with it, so fp32's winner has a z' no
lower than max over the sure faces of (z' - tau_z).  A face is a CANDIDATE where its barycentrics are >= -tau_k and its z' + tau_z is
not below that maximum.  (Where the frontmost face that fp32 MIGHT cover - barycentrics >= -tau - is itself sure, this is the set
"within tau_z of the largest such z'"; where it is not - a silhouette pixel - whatever lies behind it is a candidate too, as it must
be.)  Background is allowed where no face is sure.  A float64 zero-area face is never a candidate."""
import functools

import numpy as np

import mesh_ref as mr

EPS = 2.0 ** -24
R_BARY, R_Z = 32, 16

MESHES = {"cube": mr.cube, "tetrahedron": mr.tetrahedron, "torus": mr.torus, "ellipsoid": mr.ellipsoid}
CENTRE = 0.5 * (mr.B_MIN + mr.B_MAX)
SCALE = float(np.float32(1.0 / 190.0))        # the test box's half diagonal in x / z is 181: inside the image at every turn


def _f32(m):
    return np.asarray(m, np.float32).astype(np.float64)


def base_calib(scale=SCALE, shift=(0.0, 0.0), flip_x=False):
    """diag(+-s, -s, s) about CENTRE, then a shift in x', y': a calib as TrainDataset.get_render builds them (y' downwards)."""
    c = np.identity(4)
    c[0, 0], c[1, 1], c[2, 2] = (-scale if flip_x else scale), -scale, scale
    c[:3, 3] = -c[:3, :3] @ CENTRE
    c[0, 3] += shift[0]
    c[1, 3] += shift[1]
    return c


def tilt(deg):
    """T(CENTRE) R_x(deg) T(-CENTRE): shows the torus' hole."""
    t = np.deg2rad(deg)
    r = np.identity(4)
    r[1, 1], r[1, 2], r[2, 1], r[2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    a, b = np.identity(4), np.identity(4)
    a[:3, 3], b[:3, 3] = CENTRE, -CENTRE
    return a @ r @ b


# name -> (mesh, (h, w), calib kwargs, tilt degrees, turntable degrees)
CASES = {
    "cube_70x45_0": ("cube", (45, 70), {}, 0, 0),
    "cube_33_37": ("cube", (33, 33), {}, 0, 37),
    "cube_33_90": ("cube", (33, 33), {}, 0, 90),
    "tetrahedron_33_90": ("tetrahedron", (33, 33), {}, 0, 90),
    "tetrahedron_70x45_37": ("tetrahedron", (45, 70), {}, 20, 37),
    "torus_70x45_0": ("torus", (45, 70), {}, 0, 0),
    "torus_96_tilt": ("torus", (96, 96), {}, 50, 0),
    "torus_33_180_tilt": ("torus", (33, 33), {}, 50, 180),
    "ellipsoid_70x45_270": ("ellipsoid", (45, 70), {}, 0, 270),
    "ellipsoid_33_37_tilt": ("ellipsoid", (33, 33), {}, 30, 37),
    "torus_70x45_half_off": ("torus", (45, 70), {"scale": float(np.float32(1.0 / 90.0)), "shift": (0.9, 0.3)}, 50, 0),
    "ellipsoid_70x45_flip": ("ellipsoid", (45, 70), {"flip_x": True}, 0, 37),
    "torus_33_flip_tilt": ("torus", (33, 33), {"flip_x": True}, 50, 90),
}


def turntable(calib, degrees, centre):
    """metrics.turntable_views restated: calib . T(c) . R_y . T(-c)."""
    out = []
    for d in degrees:
        t = np.deg2rad(d)
        r = np.identity(4)
        r[0, 0], r[0, 2], r[2, 0], r[2, 2] = np.cos(t), np.sin(t), -np.sin(t), np.cos(t)
        a, b = np.identity(4), np.identity(4)
        a[:3, 3], b[:3, 3] = centre, -np.asarray(centre)
        out.append(calib @ a @ r @ b)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def case(name):
    """One case's inputs, made once and shared (read-only): v (float64 of fp32), f, size (h, w), view (float64 of the fp32 3 x 4 the
    product is handed)."""
    from surs_amd import metrics
    mesh, size, kw, tilt_deg, turn = CASES[name]
    v, f = MESHES[mesh]()
    calib = base_calib(**kw) @ tilt(tilt_deg)
    view = _f32(metrics.turntable_views(calib, (turn,), CENTRE)[0][:3])
    for a in (v, f, view):
        a.setflags(write=False)
    return dict(v=v, f=f, size=size, view=view, mesh=mesh)


def project(v, view, size):
    """Vertices in pixel units and z': ([nv, 2] (sx, sy), [nv] z', Z the largest sum of |terms| of a z')."""
    h, w = size
    v = np.asarray(v, np.float64)
    p = v @ view[:, :3].T + view[:, 3]
    s = np.stack([(p[:, 0] + 1) * (0.5 * w) - 0.5, (p[:, 1] + 1) * (0.5 * h) - 0.5], 1)
    zmag = float((np.abs(v) @ np.abs(view[2, :3]) + abs(view[2, 3])).max())
    return s, p[:, 2], zmag


def raster(v, f, view, size, chunk=256):
    """The float64 raster of one view.  Returns a dict over the P = h w pixels (row-major) and F faces:
    winner [P] (-1: background), cand bool [P, F], sure_any bool [P] (a sure face exists: background is NOT allowed), n_cand [P],
    and for the pixels with exactly one candidate that face's values one [P], b1, b2, z, tau1, tau2, tauz [P] (NaN elsewhere)."""
    h, w = size
    f = np.sort(np.asarray(f), axis=1)                 # the product's vertex order: ascending index
    s, zv, zmag = project(v, view, size)
    W = max(float(np.abs(s[np.unique(f)]).max()), float(w), float(h))
    t = s[f]                                           # [F, 3, 2]
    d1, d2, e = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], t[:, 2] - t[:, 1]
    area = d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]
    live = area != 0
    inv = np.where(live, 1.0 / np.where(live, area, 1.0), 0.0)
    a1, c1, a2, c2, a0, c0 = d2[:, 1] * inv, -d2[:, 0] * inv, -d1[:, 1] * inv, d1[:, 0] * inv, -e[:, 1] * inv, e[:, 0] * inv
    tau = [EPS * R_BARY * (1 + (np.abs(a) + np.abs(c)) * W) for a, c in ((a0, c0), (a1, c1), (a2, c2))]
    z0, dz1, dz2 = zv[f[:, 0]], zv[f[:, 1]] - zv[f[:, 0]], zv[f[:, 2]] - zv[f[:, 0]]
    tauz = EPS * R_Z * zmag + (tau[1] + tau[2]) * np.maximum(np.abs(dz1), np.abs(dz2))
    py, px = [g.reshape(-1).astype(np.float64) for g in np.meshgrid(np.arange(h), np.arange(w), indexing="ij")]
    P, F = h * w, len(f)

    def chunk_values(k):
        sl = slice(k, min(F, k + chunk))
        qx, qy = px[:, None] - t[None, sl, 0, 0], py[:, None] - t[None, sl, 0, 1]
        rx, ry = px[:, None] - t[None, sl, 1, 0], py[:, None] - t[None, sl, 1, 1]
        b1, b2, b0 = qx * a1[sl] + qy * c1[sl], qx * a2[sl] + qy * c2[sl], rx * a0[sl] + ry * c0[sl]
        z = z0[sl] + b1 * dz1[sl] + b2 * dz2[sl]
        return sl, b0, b1, b2, z

    best, winner, floor = np.full(P, -np.inf), np.full(P, -1, np.int64), np.full(P, -np.inf)
    for k in range(0, F, chunk):
        sl, b0, b1, b2, z = chunk_values(k)
        inside = live[sl] & (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
        zi = np.where(inside, z, -np.inf)
        j = zi.argmax(1)                                # the first (lowest) index of the chunk's maximum
        m = zi[np.arange(P), j]
        better = m > best
        best, winner = np.where(better, m, best), np.where(better, k + j, winner)
        sure = live[sl] & (b0 >= tau[0][sl]) & (b1 >= tau[1][sl]) & (b2 >= tau[2][sl])
        floor = np.maximum(floor, np.where(sure, z - tauz[sl], -np.inf).max(1))
    cand = np.zeros((P, F), bool)
    for k in range(0, F, chunk):
        sl, b0, b1, b2, z = chunk_values(k)
        loose = live[sl] & (b0 >= -tau[0][sl]) & (b1 >= -tau[1][sl]) & (b2 >= -tau[2][sl])
        cand[:, sl] = loose & (z + tauz[sl] >= floor[:, None])
    n_cand = cand.sum(1)
    single = n_cand == 1
    one = np.where(single, cand.argmax(1), -1)
    vals = {k: np.full(P, np.nan) for k in ("b1", "b2", "z", "tau1", "tau2", "tauz")}
    if single.any():
        i, g = np.nonzero(single)[0], one[single]
        qx, qy = px[i] - t[g, 0, 0], py[i] - t[g, 0, 1]
        vals["b1"][i], vals["b2"][i] = qx * a1[g] + qy * c1[g], qx * a2[g] + qy * c2[g]
        vals["z"][i] = z0[g] + vals["b1"][i] * dz1[g] + vals["b2"][i] * dz2[g]
        vals["tau1"][i], vals["tau2"][i], vals["tauz"][i] = tau[1][g], tau[2][g], tauz[g]
    return dict(winner=winner, cand=cand, sure_any=floor > -np.inf, n_cand=n_cand, one=one, W=W, **vals)


@functools.lru_cache(maxsize=None)
def reference(name):
    """raster() of case(name), once (read-only)."""
    c = case(name)
    ref = raster(c["v"], c["f"], c["view"], c["size"])
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


# ---------------------------------------------------------------- normals and the score, restated
def flat_colours(v, f, view, face):
    """float64 [P, 3]: 0.5 n + 0.5 of face[p]'s unit normal in the view frame, turned to n_z' >= 0; (0, 0, 0) where face[p] < 0."""
    p = np.asarray(v, np.float64) @ view[:, :3].T + view[:, 3]
    t = p[np.asarray(f)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n = n / np.linalg.norm(n, axis=1, keepdims=True).clip(1e-300)
    n = np.where(n[:, 2:3] < 0, -n, n)
    face = np.asarray(face).reshape(-1)
    return np.where(face[:, None] >= 0, 0.5 * n[face.clip(0)] + 0.5, 0.0)


def vertex_normals(v, f):
    """Area-weighted unit vertex normals, float64 (a plain loop over the faces)."""
    v, f = np.asarray(v, np.float64), np.asarray(f)
    out = np.zeros_like(v)
    for a, b, c in f:
        n = np.cross(v[b] - v[a], v[c] - v[a])
        out[a] += n
        out[b] += n
        out[c] += n
    l = np.linalg.norm(out, axis=1, keepdims=True)
    return np.where(l == 0, 0.0, out / np.where(l == 0, 1.0, l))


def smooth_colours(v, f, view, vn, face, bary):
    """float64 [P, 3] of the smooth mode from given winners and barycentrics: inverse-transpose of the view's linear part times the
    blend of the vertex normals, normalised, turned to n_z' >= 0."""
    face, bary = np.asarray(face).reshape(-1), np.asarray(bary, np.float64).reshape(-1, 2)
    idx = np.sort(np.asarray(f), axis=1)[face.clip(0)]     # bary refers to the vertices in ascending index order
    b0 = 1.0 - bary[:, 0] - bary[:, 1]
    m = b0[:, None] * vn[idx[:, 0]] + bary[:, :1] * vn[idx[:, 1]] + bary[:, 1:] * vn[idx[:, 2]]
    n = m @ np.linalg.inv(view[:, :3])                  # (A^-T m)^T = m^T A^-1
    n = n / np.linalg.norm(n, axis=1, keepdims=True).clip(1e-300)
    n = np.where(n[:, 2:3] < 0, -n, n)
    return np.where(face[:, None] >= 0, 0.5 * n + 0.5, 0.0)


def restate_normal_error(maps_pred, masks_pred, maps_gt, masks_gt):
    """metrics.normal_error from the maps of each view ([V, h, w, 3] and [V, h, w]), in float64."""
    per_view, iou = [], []
    for mp, kp, mg, kg in zip(maps_pred, masks_pred, maps_gt, masks_gt):
        d = np.asarray(mp, np.float64) - np.asarray(mg, np.float64)
        per_view.append(float((d * d).sum(-1).mean()))
        either = int((kp | kg).sum())
        iou.append(float((kp & kg).sum()) / either if either else 1.0)
    return dict(normal_error=float(np.mean(per_view)), per_view=per_view, mask_iou=float(np.mean(iou)))
