"""How good a reconstruction is: point-to-surface distance (P2S), Chamfer distance and normal consistency against a ground-truth
mesh, the scores this family of papers reports.  Samples come from the package's counter PRNG (native.mesh_sample_pool, area
weighted, no jitter), distances from the brute-force kernel behind native.mesh_distance; one host synchronisation per score."""
import numpy as np
import torch

from . import native


def as_mesh(m):
    """A native.Mesh as it is; a (verts, faces) pair uploaded as one."""
    if isinstance(m, native.Mesh):
        return m
    if isinstance(m, (tuple, list)) and len(m) == 2:
        return native.Mesh(m[0], m[1])
    raise TypeError("a native.Mesh or a (verts, faces) pair is expected, not %s" % type(m).__name__)


def check_samples(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("n %r: the number of surface samples must be a positive integer" % (n,))
    return int(n)


def surface_samples(mesh, n, seed=0):
    """n points on the mesh's surface, area weighted and un-jittered, from the streams of `seed` in generation order: (points [n,3]
    float32, face [n] int32, the face each point was drawn on).  Device tensors."""
    n = check_samples(n)
    zero = (0.0, 0.0, 0.0)
    points, _, face = native.mesh_sample_pool(mesh, n, 0, 0.0, zero, zero, seed, want_faces=True, shuffle=False)
    return points, face


def face_normals(mesh):
    """[nf,3] unit normals (v1 - v0) x (v2 - v0) / |.|, float64 from the fp32 vertices; zero for a zero-area face."""
    t = mesh.verts.double()[mesh.faces.long()]
    n = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    l = torch.linalg.norm(n, dim=1, keepdim=True)
    return torch.where(l == 0, torch.zeros_like(n), n / torch.where(l == 0, torch.ones_like(l), l))


def _direction(src, dst, n, seed, normals_src, normals_dst):
    """[sum of distances, largest distance, sum of |n_src . n_dst|] of n samples of src against dst: float64 [3] on the device."""
    points, face = surface_samples(src, n, seed)
    dist, near = native.mesh_distance(points, dst, want_face=True)
    dots = (normals_src[face.long()] * normals_dst[near.long()]).sum(1).abs()
    return torch.stack([dist.double().sum(), dist.max().double(), dots.sum()])


def mesh_metrics(pred, gt, n=10000, seed=0):
    """Scores of the mesh `pred` against the mesh `gt` (native.Mesh objects or (verts, faces) pairs in ONE frame and unit), from n
    surface samples of each:
        p2s                 mean distance of pred's samples to gt        max_p2s       the largest of them
        gt2pred             mean distance of gt's samples to pred        max_gt2pred
        chamfer             (p2s + gt2pred) / 2
        normal_consistency  mean over both directions of |n_src[sample's face] . n_dst[nearest face]| (either orientation)
        n
    Python floats.  The means are float64 sums of the fp32 distances; everything is enqueued first and read back once."""
    n = check_samples(n)
    pred, gt = as_mesh(pred), as_mesh(gt)
    normals_pred, normals_gt = face_normals(pred), face_normals(gt)
    both = torch.cat([_direction(pred, gt, n, seed, normals_pred, normals_gt),
                      _direction(gt, pred, n, seed, normals_gt, normals_pred)]).cpu().tolist()     # the one synchronisation
    p2s, gt2pred = both[0] / n, both[3] / n
    return dict(p2s=p2s, gt2pred=gt2pred, chamfer=0.5 * (p2s + gt2pred), max_p2s=both[1], max_gt2pred=both[4],
                normal_consistency=0.5 * (both[2] / n + both[5] / n), n=n)


def pred_to_gt_transform(calib=None):
    """The 4x4 float64 matrix that takes a reconstruction's vertices into the frame of the item's ground-truth scan.  The
    reconstruction lives where train_util.gen_calib() projects, the scan where the item's calib projects - both onto the same image -,
    so X_world = inv(calib[0]) . gen_calib . x.  calib: [V,4,4] or [4,4] (tensor or array; view 0 counts); None: the identity."""
    if calib is None:
        return np.identity(4)
    from .train_util import gen_calib
    c = calib.detach().cpu().numpy() if isinstance(calib, torch.Tensor) else np.asarray(calib)
    c = np.asarray(c, np.float64)
    if c.ndim == 3:
        c = c[0]
    if c.shape != (4, 4):
        raise ValueError("calib: [V,4,4] or [4,4] expected, not %s" % (c.shape,))
    return np.linalg.inv(c) @ gen_calib()[0].numpy().astype(np.float64)


def transform_verts(mat, verts):
    """mat[:3,:3] . v + mat[:3,3] per vertex, float64 on the host."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    return v @ mat[:3, :3].T + mat[:3, 3]
