"""How good a reconstruction is: point-to-surface distance (P2S), Chamfer distance and normal consistency against a ground-truth
mesh, the scores this family of papers reports.  Samples come from the package's counter PRNG (native.mesh_sample_pool, area
weighted, no jitter), distances from the brute-force kernel behind native.mesh_distance; one host synchronisation per score.
The papers' third number, the normal reprojection error (normal_error), renders both meshes as normal maps through turntable views
(turntable_views) with the rasteriser behind native.normal_map and compares them per pixel."""
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


def _matrix44(calib, what):
    """[4,4] float64 from a [4,4] or [V,4,4] tensor or array (view 0 counts)."""
    c = calib.detach().cpu().numpy() if isinstance(calib, torch.Tensor) else np.asarray(calib)
    c = np.asarray(c, np.float64)
    if c.ndim == 3:
        c = c[0]
    if c.shape != (4, 4):
        raise ValueError("%s: [V,4,4] or [4,4] expected, not %s" % (what, c.shape))
    return c


def turntable_views(calib, degrees=(0, 90, 180, 270), centre=None):
    """float64 [V,4,4]: view k is calib . T(c) . R_y(degrees[k]) . T(-c), the camera of `calib` looking at the scene turned about the
    vertical axis through c (the origin without a centre).  View 0 of the default is the calib itself."""
    c44 = _matrix44(calib, "calib")
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float64).reshape(3)
    to, back = np.identity(4), np.identity(4)
    to[:3, 3], back[:3, 3] = c, -c
    views = []
    for d in degrees:
        quarter, rest = divmod(float(d), 90.0)
        if rest == 0:      # whole quarter turns are exact
            cs, sn = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(quarter) % 4]
        else:
            cs, sn = np.cos(np.deg2rad(d)), np.sin(np.deg2rad(d))
        r = np.identity(4)
        r[0, 0], r[0, 2], r[2, 0], r[2, 2] = cs, sn, -sn, cs
        views.append(c44 @ to @ r @ back)
    return np.stack(views) if views else np.zeros((0, 4, 4))


def vertex_normals(mesh):
    """[nv,3] float64 unit vertex normals on the host: the sum of (v1 - v0) x (v2 - v0) over the faces at a vertex (area weighted),
    normalised; zero where a vertex has no face with an area.  mesh: a native.Mesh or a (verts, faces) pair.  Once per mesh."""
    if isinstance(mesh, native.Mesh):
        v, f = mesh.verts.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy().astype(np.int64)
    else:
        v, f = np.asarray(mesh[0], np.float32).astype(np.float64).reshape(-1, 3), np.asarray(mesh[1], np.int64).reshape(-1, 3)
    t = v[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    out = np.zeros_like(v)
    for k in range(3):
        np.add.at(out, f[:, k], n)
    l = np.linalg.norm(out, axis=1, keepdims=True)
    return np.where(l == 0, 0.0, out / np.where(l == 0, 1.0, l))


def box_centre(mesh):
    """The centre of the mesh's bounding box: float64 [3] on the host (one read of the device)."""
    v = as_mesh(mesh).verts
    return (0.5 * (v.min(0)[0].double() + v.max(0)[0].double())).cpu().numpy()


def normal_error_of_maps(maps_pred, masks_pred, maps_gt, masks_gt):
    """The sums of normal_error for one view from the two meshes' maps [h,w,3] and masks [h,w] (device tensors): float64 [3] on the
    device - the sum over pixels and channels of (c_pred - c_gt)^2, |both covered|, |either covered|."""
    d = maps_pred.double() - maps_gt.double()
    return torch.stack([(d * d).sum(), (masks_pred & masks_gt).sum().double(), (masks_pred | masks_gt).sum().double()])


def normal_error(pred, gt, views, size=512, smooth=False, centre=None):
    """The normal reprojection error of the mesh `pred` against the mesh `gt` (native.Mesh objects or (verts, faces) pairs in ONE
    frame): both are rendered as normal maps (native.normal_map: 0.5 n + 0.5 in the view frame, background (0, 0, 0)) through each
    of `views` and the maps are compared per pixel.
        normal_error  the mean over the views of [mean over the h w pixels of sum over the channels of (c_pred - c_gt)^2]
        per_view      the list of those values
        mask_iou      the mean over the views of |both covered| / |either covered| (1 where neither mesh is seen)
        size          (h, w)
    views: [V,4,4] or [V,3,4] matrices, or a tuple of turntable degrees - then the views are turntable_views(identity, degrees,
    centre), centre=None being the centre of gt's bounding box (any other `views` ignores centre).  smooth blends vertex_normals.
    Python floats.  The sums are float64 on the device; everything is enqueued first and read back once."""
    pred, gt = as_mesh(pred), as_mesh(gt)
    h, w = native._image_size(size)
    v = np.asarray(views, np.float64) if not isinstance(views, torch.Tensor) else views.detach().cpu().numpy().astype(np.float64)
    if v.ndim == 1:
        if centre is None:
            centre = box_centre(gt)
        v = turntable_views(np.identity(4), tuple(v.tolist()), centre)
    if v.ndim != 3 or v.shape[1:] not in ((3, 4), (4, 4)) or len(v) == 0:
        raise ValueError("views: [V,4,4], [V,3,4] or a tuple of degrees expected, not %s" % (v.shape,))
    upload = lambda m: torch.from_numpy(vertex_normals(m).astype(np.float32)).to(m.verts.device)      # once per mesh, not per view
    vn_pred = upload(pred) if smooth else None
    vn_gt = upload(gt) if smooth else None
    sums = []
    for m in v:
        map_p, mask_p = native.normal_map(pred, m, (h, w), vn_pred)
        map_g, mask_g = native.normal_map(gt, m, (h, w), vn_gt)
        sums.append(normal_error_of_maps(map_p, mask_p, map_g, mask_g))
    sums = torch.stack(sums).cpu().tolist()                                         # the one synchronisation
    per_view = [s[0] / (h * w) for s in sums]
    iou = [s[1] / s[2] if s[2] else 1.0 for s in sums]
    return dict(normal_error=sum(per_view) / len(per_view), per_view=per_view, mask_iou=sum(iou) / len(iou), size=(h, w))


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
