"""Float64 yardstick of the mesh-distance tests (plain numpy, nothing of the product): the per-pair distance matrix of
mesh_ref.surface_distance's formula (chunked over the faces), the set of faces that attain a point's minimum, the distance to one
given face per point, the tests' points and bound, and the restatement of metrics.mesh_metrics on given samples."""
import functools

import numpy as np

import mesh_ref as mr

ROUNDINGS = 16


def bound(*arrays):
    """B = 2^-24 * 16 * S, S the largest |coordinate| among the call's vertices and points: mesh_ref.MARGIN's rule (fp32 roundings at
    the coordinate's size) narrowed from 64 roundings to 16."""
    s = max(float(np.abs(np.asarray(a, np.float64)).max()) for a in arrays if np.size(a))
    return 2.0 ** -24 * ROUNDINGS * s


def _pair_d2(p, a, b, c):
    """mesh_ref.surface_distance's body for broadcastable [P, F, 3] operands: squared distances [P, F]."""
    d2 = np.minimum(np.minimum(mr._segment_d2(p, a, b), mr._segment_d2(p, b, c)), mr._segment_d2(p, c, a))
    n = np.cross(b - a, c - a)
    nn = np.einsum("pfi,pfi->pf", n, n)
    safe = np.where(nn == 0, 1.0, nn)
    ap = p - a
    wb = np.einsum("pfi,pfi->pf", np.cross(ap, c - a), n) / safe
    wc = np.einsum("pfi,pfi->pf", np.cross(b - a, ap), n) / safe
    inside = (nn != 0) & (wb >= 0) & (wc >= 0) & (wb + wc <= 1)
    plane = np.einsum("pfi,pfi->pf", ap, n) ** 2 / safe
    return np.where(inside, plane, d2)


def distance_matrix(points, v, f, chunk=512):
    """Yields (first face, distances [n, faces of the chunk]) in float64."""
    p = np.asarray(points, np.float64).reshape(-1, 3)[:, None]
    t = np.asarray(v, np.float64)[np.asarray(f)]
    for k in range(0, len(t), chunk):
        yield k, np.sqrt(_pair_d2(p, t[None, k:k + chunk, 0], t[None, k:k + chunk, 1], t[None, k:k + chunk, 2]))


def nearest(points, v, f, chunk=512):
    """(float64 distance to the nearest face, the lowest face index attaining it in float64)."""
    n = len(np.asarray(points).reshape(-1, 3))
    best, arg = np.full(n, np.inf), np.full(n, -1, np.int64)
    for k, d in distance_matrix(points, v, f, chunk):
        j = d.argmin(1)
        m = d[np.arange(n), j]
        less = m < best
        best, arg = np.where(less, m, best), np.where(less, k + j, arg)
    return best, arg


def argmin_sets(points, v, f, tol, chunk=512):
    """Per point the sorted face indices whose float64 distance is within tol of the point's minimum."""
    best, _ = nearest(points, v, f, chunk)
    sets = [[] for _ in best]
    for k, d in distance_matrix(points, v, f, chunk):
        for i, j in zip(*np.nonzero(d <= best[:, None] + tol)):
            sets[i].append(k + int(j))
    return sets


def distance_to_face(points, v, f, face):
    """Float64 distance of point i to triangle face[i]."""
    p = np.asarray(points, np.float64).reshape(-1, 1, 3)
    t = np.asarray(v, np.float64)[np.asarray(f)[np.asarray(face, np.int64)]][:, None]
    return np.sqrt(_pair_d2(p, t[:, :, 0], t[:, :, 1], t[:, :, 2]))[:, 0]


MESHES = {"tetrahedron": mr.tetrahedron, "cube": mr.cube, "torus": mr.torus, "parts": mr.parts_mesh}
N_POINTS = 1061


def special_points(v, f, faces=64):
    """Every vertex (the distance is exactly 0), and the edge midpoints and centroids of the first `faces` faces, fp32."""
    t = np.asarray(v, np.float64)[np.asarray(f)[:faces]]
    mid = [0.5 * (t[:, i] + t[:, (i + 1) % 3]) for i in range(3)]
    return np.concatenate([np.asarray(v, np.float64)] + mid + [t.mean(1)], 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """One mesh's inputs, made once and shared (read-only): v (float64 of fp32), f, points fp32 [n, 3] = contains_points sigma 5 |
    sigma 0 | special_points, vertices (their slice of the points), B."""
    v, f = MESHES[name]()
    seed = sorted(MESHES).index(name) + 11
    pts = np.concatenate([mr.contains_points((v, f), N_POINTS, seed, 5.0), mr.contains_points((v, f), N_POINTS, seed + 100, 0.0),
                          special_points(v, f)], 0)
    for a in (v, f, pts):
        a.setflags(write=False)
    return dict(v=v, f=f, points=pts, vertices=slice(2 * N_POINTS, 2 * N_POINTS + len(v)), B=bound(v, pts))


@functools.lru_cache(maxsize=None)
def reference(name):
    """mesh_ref.surface_distance of case(name)'s points, once (read-only)."""
    c = case(name)
    ref = mr.surface_distance(c["points"], c["v"], c["f"])
    ref.setflags(write=False)
    return ref


def parts_with_duplicate():
    """parts_mesh with face 10 appended once more at the end: index 8199, in the last part."""
    v, f = mr.parts_mesh()
    return v, np.concatenate([f, f[10:11]], 0)


# ---------------------------------------------------------------- the metrics, restated
def unit_normals(v, f):
    t = np.asarray(v, np.float64)[np.asarray(f)]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(l == 0, 0.0, n / np.where(l == 0, 1.0, l))


def direction(points, src_face, src, dst, reported_face):
    """One direction of the metrics on given samples of `src` (their points and faces): (mean float64 distance to dst, the maximum,
    the mean |n_src[sample's face] . n_dst[reported_face]|)."""
    d = mr.surface_distance(points, *dst)
    dots = np.abs(np.einsum("ij,ij->i", unit_normals(*src)[np.asarray(src_face)], unit_normals(*dst)[np.asarray(reported_face)]))
    return float(d.mean()), float(d.max()), float(dots.mean())


def restate_metrics(pred, gt, samples_pred, samples_gt):
    """mesh_metrics from downloaded samples: samples_* = (points, source face, the face the product reported on the other mesh)."""
    p2s, max_p2s, nc_p = direction(samples_pred[0], samples_pred[1], pred, gt, samples_pred[2])
    g2p, max_g2p, nc_g = direction(samples_gt[0], samples_gt[1], gt, pred, samples_gt[2])
    return dict(p2s=p2s, gt2pred=g2p, chamfer=0.5 * (p2s + g2p), max_p2s=max_p2s, max_gt2pred=max_g2p,
                normal_consistency=0.5 * (nc_p + nc_g))
