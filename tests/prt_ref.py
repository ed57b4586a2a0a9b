"""Float64 model of the per-vertex PRT (include/surs.h "mesh PRT"), written from its statement in plain numpy - nothing of the product
except the directions' generator: the basis, the ray - triangle test, the visibility and the sum, plus the meshes and scenes the PRT
and shading tests share and the closed form the unshadowed sum converges to."""
import functools

import numpy as np

import mesh_ref as mr

EPS = 2.0 ** -24
A_BAND = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sh9(d):
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([0.282095 + 0 * x, 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3 * z * z - 1), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def closed_form(n):
    """The unshadowed transfer vector of a unit normal: A_l Y_i(n)."""
    return A_BAND * sh9(n)


# ---------------------------------------------------------------- meshes and scenes (vertices rounded to fp32)
@functools.lru_cache(None)
def icosphere(level=1, radius=50.0, center=(0.0, 100.0, 0.0)):
    """20 * 4^level faces (level 1: 80, level 2: 320), outward oriented; returns (verts, faces, unit normals)."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    unit = np.array(v)
    verts = mr._f32(unit * radius + np.asarray(center))
    faces = np.array(f, np.int32)
    assert mr.signed_volume(verts, faces) > 0
    return verts, faces, np.asarray(unit, np.float32).astype(np.float64)


@functools.lru_cache(None)
def floor_roof():
    """Scene 1: a 2 x 2 floor at y = 0 (3 x 3 vertices, 8 triangles) under a 1 x 1 roof at y = 0.5 (2 triangles); every normal +y."""
    v = [(x, 0.0, z) for z in (-1.0, 0.0, 1.0) for x in (-1.0, 0.0, 1.0)]
    f = []
    for j in range(2):
        for i in range(2):
            a, b, c, d = j * 3 + i, j * 3 + i + 1, (j + 1) * 3 + i + 1, (j + 1) * 3 + i
            f += [(a, d, c), (a, c, b)]
    v += [(-0.5, 0.5, -0.5), (0.5, 0.5, -0.5), (0.5, 0.5, 0.5), (-0.5, 0.5, 0.5)]
    f += [(9, 12, 11), (9, 11, 10)]
    verts = mr._f32(np.array(v))
    return verts, np.array(f, np.int32), np.tile(np.array([0.0, 1.0, 0.0]), (len(v), 1))


def unit_normals(v, f):
    """Area-weighted unit vertex normals, float64 rounded to fp32 (what the kernels are given)."""
    t = np.asarray(v, np.float64)[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    out = np.zeros((len(v), 3))
    for k in range(3):
        np.add.at(out, f[:, k], n)
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return out.astype(np.float32).astype(np.float64)


@functools.lru_cache(None)
def torus_scene(nu=24, nv=12):
    """Scene 2: the bumpy torus, whose inner ring shadows itself."""
    v, f = mr.torus(nu, nv)
    return v, f, unit_normals(v, f)


def diagonal(v):
    v = np.asarray(v, np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ---------------------------------------------------------------- the model
def _ray_segment_distance(o, d, length, a, b):
    """Distance between the ray pieces o + t d, t in [0, length] ([P,1,3]) and the segments a b ([1,E,3]): [P,E]."""
    d1, d2, r = d * length, b - a, o - a
    aa, ee = np.einsum("pei,pei->pe", d1, d1), np.einsum("pei,pei->pe", d2, d2)
    ff, cc, bb = np.einsum("pei,pei->pe", d2, r), np.einsum("pei,pei->pe", d1, r), np.einsum("pei,pei->pe", d1, d2)
    den = aa * ee - bb * bb
    safe_e = np.where(ee == 0, 1.0, ee)
    s = np.where(den > 0, np.clip((bb * ff - cc * ee) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
    t = np.where(ee == 0, 0.0, np.clip((bb * s + ff) / safe_e, 0.0, 1.0))
    s = np.clip((bb * t - cc) / aa, 0.0, 1.0)
    gap = (o + d1 * s[..., None]) - (a + d2 * t[..., None])
    return np.sqrt(np.einsum("pei,pei->pe", gap, gap))


def visibility(v, f, normals, dirs, offset, margin=None, chunk=256):
    """lit bool [nv, D]: n . d > 0 and no triangle hit (Moeller - Trumbore, edges inclusive, t > 0, own faces skipped by index, a
    zero-area or non-finite triangle hits nothing; a non-finite vertex is never lit).  With margin (a length) also uncertain bool
    [nv, D]: pairs whose ray passes within margin of a triangle edge (own faces included: they bound the neighbours) or whose
    |n . d| is below 1e-4."""
    v, normals, dirs = np.asarray(v, np.float64), np.asarray(normals, np.float64), np.asarray(dirs, np.float64)
    f = np.asarray(f)
    nv, D = len(v), len(dirs)
    tri = v[f]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(invalid="ignore"):
        good = np.isfinite(tri).all((1, 2)) & np.any(np.cross(e1, e2) != 0, axis=1)
    cosine = normals @ dirs.T
    usable = np.isfinite(v).all(1) & np.isfinite(normals).all(1)
    with np.errstate(invalid="ignore"):
        cast = usable[:, None] & (cosine > 0)
    origin = v + offset * normals
    lit = np.zeros((nv, D), bool)
    uncertain = np.zeros((nv, D), bool)
    reach = 4.0 * diagonal(v[usable]) if margin is not None else 0.0
    edges_a = np.concatenate([tri[good][:, k] for k in range(3)])[None]
    edges_b = np.concatenate([tri[good][:, (k + 1) % 3] for k in range(3)])[None]
    pv, pk = np.nonzero(cast)
    for c0 in range(0, len(pv), chunk):
        iv, ik = pv[c0:c0 + chunk], pk[c0:c0 + chunk]
        o, d = origin[iv][:, None], dirs[ik][:, None]                   # [P,1,3]
        p = np.cross(d, e2[None])                                       # [P,F,3]
        det = np.einsum("fi,pfi->pf", e1, p)
        s = o - a[None]
        u = np.einsum("pfi,pfi->pf", s, p)
        q = np.cross(s, e1[None])
        w = np.einsum("pfi,pfi->pf", np.broadcast_to(d, q.shape), q)
        t = np.einsum("fi,pfi->pf", e2, q)
        sign = np.where(det < 0, -1.0, 1.0)
        ad, u, w, t = np.abs(det), u * sign, w * sign, t * sign
        own = (f[None, :, :] == iv[:, None, None]).any(2)
        hit = good[None] & ~own & (ad > 0) & (u >= 0) & (w >= 0) & (u + w <= ad) & (t > 0)
        lit[iv, ik] = ~hit.any(1)
        if margin is not None:
            uncertain[iv, ik] = (_ray_segment_distance(o, d, reach, edges_a, edges_b) < margin).any(1)
    if margin is not None:
        with np.errstate(invalid="ignore"):
            uncertain |= usable[:, None] & (np.abs(cosine) < 1e-4)
        return lit, uncertain
    return lit


def coefficients(normals, dirs, lit):
    """prt float64 [nv, 9] = (4 pi / D) sum_k lit max(0, n . d_k) Y(d_k)."""
    normals, dirs = np.asarray(normals, np.float64), np.asarray(dirs, np.float64)
    with np.errstate(invalid="ignore"):
        wgt = np.where(lit, np.maximum(np.nan_to_num(normals) @ dirs.T, 0.0), 0.0)
    return (4.0 * np.pi / len(dirs)) * (wgt @ sh9(dirs))


def bound(D):
    """What fp32 may cost a coefficient: D terms of at most 1.1 (max(0, n.d) |Y_i| <= 1.093), each off by at most 8 roundings of its
    own size (the dot product, the basis polynomial, the product), added into a partial sum of at most 1.1 k at one rounding each,
    then scaled by 4 pi / D (the constant's and the product's roundings, and the division's, on a result of at most 4 pi 1.1)."""
    return (4.0 * np.pi / D) * 1.1 * EPS * (D * D / 2.0 + 8.0 * D) + 3.0 * EPS * 4.0 * np.pi * 1.1
