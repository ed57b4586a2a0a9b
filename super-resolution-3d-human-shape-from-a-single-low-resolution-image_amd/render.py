"""Render a textured scan's training views without OpenGL: per-vertex PRT (native.mesh_prt), the raster (native.mesh_raster), colour
shading and the box resolve (native.mesh_shade_prt, native.image_resolve), and the PARAM dict / calib of each view in exactly the
form data.TrainDataset reads.  apps/render_data.py writes a dataroot with it.  Orthographic camera only; INTEGRATION.md "Rendering
the training set" states the conventions and what differs from a GL render.

Frames.  A view's R = Rx(pitch) Ry(yaw) takes the mesh's frame into the camera's (y up, the camera on the +z side).  A light is nine
RGB coefficients in the CAMERA frame.  The transfer vectors live in the mesh's frame, so render_views rotates the LIGHT into the
mesh's frame once per view - sh_rotate(light, R^T) - instead of every vertex's transfer vector into the camera's, as a GL vertex
shader does: the shading is the inner product of the two either way, and nine vectors are cheaper than a mesh."""
import os

import numpy as np

from . import data, prng

SH_A = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)     # the clamped-cosine kernel per band
PRT_OFFSET = 1e-3            # the ray origin's offset along the normal, as a fraction of the subject's height
_BANDS = ((0, 1), (1, 4), (4, 9))


# ---------------------------------------------------------------- spherical harmonics (float64, host)
def sh9(d):
    """Y_0..8 of unit directions d [..., 3] in the order l (l + 1) + m: float64 [..., 9] (the constants of include/surs.h)."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z,
                     0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z, 0.546274 * (x * x - y * y)], -1)


def _fixed_directions():
    """Nine unit directions at which each band's basis is of full rank (a fixed, well-spread set)."""
    k = np.arange(9) + 0.5
    z = 1.0 - 2.0 * k / 9.0
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def sh_rotation_matrix(R):
    """M [9,9] float64, block diagonal by band, with sum_i c'_i Y_i(d) = sum_i c_i Y_i(R^T d) for c' = M c.  Each band is a
    rotation-invariant space, so its block is fixed by the basis at enough directions: Y_l(R^T d_k) = M_l^T Y_l(d_k), solved by least
    squares over nine fixed directions (exact up to rounding)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    d = _fixed_directions()
    A, B = sh9(d), sh9(d @ R)                      # rows k: Y(d_k) and Y(R^T d_k)   (d @ R = (R^T d)^T)
    M = np.zeros((9, 9))
    for lo, hi in _BANDS:
        # B_l = A_l X, c'. Y(d) = c . Y(R^T d) = c . (X^T Y(d))  =>  c' = X c
        X = np.linalg.lstsq(A[:, lo:hi], B[:, lo:hi], rcond=None)[0]
        M[lo:hi, lo:hi] = X
    return M


def sh_rotate(light, R):
    """The coefficients [9, 3] (or [9]) of the lighting seen from a frame rotated by R: L'(d) = L(R^T d), band by band; float64."""
    return sh_rotation_matrix(R) @ np.asarray(light, np.float64)


# ---------------------------------------------------------------- directions, lights (pure functions of the seed)
def prt_directions(n=40, seed=0):
    """n x n stratified unit directions, float32 [n n, 3]: cos theta = 1 - 2 (i + xi_1) / n, phi = 2 pi (j + xi_2) / n at index
    i n + j, (xi_1, xi_2) the entries [i n + j] and [n n + i n + j] of the counter PRNG stream 'prt_dirs'."""
    n = int(n)
    if n < 1:
        raise ValueError("prt_directions: n >= 1 is needed")
    xi = prng.uniform01("prt_dirs", int(seed), 2 * n * n).astype(np.float64)
    i, j = np.divmod(np.arange(n * n), n)
    c = 1.0 - 2.0 * (i + xi[:n * n]) / n
    phi = 2.0 * np.pi * (j + xi[n * n:]) / n
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    return np.ascontiguousarray(np.stack([s * np.cos(phi), s * np.sin(phi), c], -1).astype(np.float32))


def _rot_axis(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.identity(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def sample_light(rng, env_sh=None, up=1):
    """One light [9, 3] float64 in the camera frame, a pure function of the integer seed `rng` (stream 'render_light').  env_sh
    [K, 9, 3]: entry floor(xi_0 K), rotated about the up axis by 0.2 pi (xi_1 - 0.5).  None: band 0 = 0.8, the other eight rows
    uniform in [0, 1) per channel."""
    u = prng.uniform01("render_light", int(rng), 26).astype(np.float64)
    if env_sh is None:
        light = np.empty((9, 3))
        light[0] = 0.8
        light[1:] = u[2:].reshape(8, 3)
        return light
    env = np.asarray(env_sh, np.float64)
    if env.ndim != 3 or env.shape[1:] != (9, 3) or len(env) < 1:
        raise ValueError("env_sh: [K, 9, 3] expected, not %s" % (env.shape,))
    k = min(int(u[0] * len(env)), len(env) - 1)
    return sh_rotate(env[k], _rot_axis(up, 0.2 * np.pi * (u[1] - 0.5)))


# ---------------------------------------------------------------- OBJ with texture coordinates
def load_textured_obj(path):
    """(verts float64 [nv,3], faces int32 [nf,3], uvs float64 [nuv,2], faces_uv int32 [nf,3]) of a Wavefront OBJ with one texture:
    `v`, `vt` and `f a/b[/c]` records, negative indices counting back, polygons as the fan (0, i, i + 1).  Every face corner needs
    a texture index.  A file that switches materials (more than one distinct `usemtl`) is refused: multi-material scans are not built."""
    verts, uvs, faces, faces_uv, materials = [], [], [], [], []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            rec = line.split()
            if not rec:
                continue
            if rec[0] == "v":
                if len(rec) < 4:
                    raise ValueError("%s:%d: a vertex needs three coordinates" % (path, no))
                verts.append((float(rec[1]), float(rec[2]), float(rec[3])))
            elif rec[0] == "vt":
                if len(rec) < 3:
                    raise ValueError("%s:%d: a texture coordinate needs two values" % (path, no))
                uvs.append((float(rec[1]), float(rec[2])))
            elif rec[0] == "usemtl":
                name = " ".join(rec[1:])
                if name not in materials:
                    materials.append(name)
                if len(materials) > 1:
                    raise ValueError("%s:%d: a second material (%s after %s): multi-material OBJ/MTL is not built; bake the scan "
                                     "into one texture" % (path, no, materials[1], materials[0]))
            elif rec[0] == "f":
                vi, ti = [], []
                for entry in rec[1:]:
                    part = entry.split("/")
                    if len(part) < 2 or not part[1]:
                        raise ValueError("%s:%d: corner %s has no texture index" % (path, no, entry))
                    for field, pool, dst, what in ((part[0], verts, vi, "vertex"), (part[1], uvs, ti, "texture")):
                        i = int(field)
                        i = i - 1 if i > 0 else len(pool) + i
                        if field.lstrip("-") == "0" or i < 0 or i >= len(pool):
                            raise ValueError("%s:%d: %s index %s out of range" % (path, no, what, entry))
                        dst.append(i)
                if len(vi) < 3:
                    raise ValueError("%s:%d: a face needs three corners" % (path, no))
                for k in range(1, len(vi) - 1):
                    faces.append((vi[0], vi[k], vi[k + 1]))
                    faces_uv.append((ti[0], ti[k], ti[k + 1]))
    return (np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3),
            np.asarray(uvs, np.float64).reshape(-1, 2), np.asarray(faces_uv, np.int32).reshape(-1, 3))


# ---------------------------------------------------------------- the subject's frame, a view's parameters
def subject_frame(verts, up=1):
    """(center float64 [3], scale): the per-axis median of the vertices with the up axis replaced by the middle of its range;
    scale = 180 / (range along up)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    lo, hi = v[:, up].min(), v[:, up].max()
    if not hi > lo:
        raise ValueError("subject_frame: the mesh has no extent along axis %d" % up)
    center = np.median(v, 0)
    center[up] = 0.5 * (lo + hi)
    return center, 180.0 / (hi - lo)


def view_param(yaw, pitch, size, center, scale):
    """(param, calib): the PARAM dict {ortho_ratio: 0.4 * 512 / size, scale, center, R = Rx(pitch) Ry(yaw)} (degrees) and the
    float32 [4,4] calib data.TrainDataset makes of it at loadSize = size (data.param_calib: the dataset's own expressions)."""
    R = _rot_axis(0, np.radians(float(pitch))) @ _rot_axis(1, np.radians(float(yaw)))
    param = {"ortho_ratio": 0.4 * 512 / int(size), "scale": float(scale), "center": np.asarray(center, np.float64).reshape(3), "R": R}
    return param, data.param_calib(param, int(size))[0]


# ---------------------------------------------------------------- rendering
class Subject:
    """A scan prepared for render_views: the mesh (host arrays, or a native.Mesh and device tensors), its float32 vertex normals,
    and - textured - uvs, faces_uv and the texture pyramid.  device='cpu' keeps everything on the host for the host twins."""

    def __init__(self, mesh, texture=None, device=None):
        from . import metrics, native
        self.host = device == "cpu"
        verts, faces = np.asarray(mesh[0], np.float32), np.asarray(mesh[1], np.int32)
        self.normals = np.ascontiguousarray(metrics.vertex_normals((verts, faces)).astype(np.float32))
        self.textured = texture is not None
        if self.textured and len(mesh) < 4:
            raise ValueError("a texture needs the mesh's uvs and faces_uv: (verts, faces, uvs, faces_uv)")
        self.uvs = np.ascontiguousarray(np.asarray(mesh[2], np.float32)) if self.textured else None
        self.faces_uv = np.ascontiguousarray(np.asarray(mesh[3], np.int32)) if self.textured else None
        if self.host:
            self.verts, self.faces = np.ascontiguousarray(verts), np.ascontiguousarray(faces)
            self.texture = native.texture_pyramid(texture, host=True) if self.textured else None
        else:
            import torch
            self.mesh = native.Mesh(verts, faces, device)
            dev = self.mesh.verts.device
            self.verts, self.faces = self.mesh.verts, self.mesh.faces
            self.texture = native.texture_pyramid(texture, device=dev) if self.textured else None
            self.normals_dev = torch.from_numpy(self.normals).to(dev)
            if self.textured:
                self.uvs, self.faces_uv = torch.from_numpy(self.uvs).to(dev), torch.from_numpy(self.faces_uv).to(dev)

    def prt(self, dirs=None, offset=None):
        """The subject's transfer vectors [nv, 9] (a device tensor, or an array on the host) for `dirs` (default: prt_directions())
        with the ray offset PRT_OFFSET times the mesh's largest extent unless given.  Compute once and keep."""
        from . import native
        dirs = prt_directions() if dirs is None else dirs
        if self.host:
            if offset is None:
                offset = PRT_OFFSET * float((self.verts.max(0) - self.verts.min(0)).max())
            return native.mesh_prt_host(self.verts, self.faces, self.normals, dirs, offset)
        if offset is None:
            offset = PRT_OFFSET * float((self.verts.max(0)[0] - self.verts.min(0)[0]).max())
        return native.mesh_prt(self.mesh, self.normals_dev, dirs, offset)


def render_views(mesh, texture, prt, params, lights, size, ms=2, device=None):
    """Render one subject's views: uint8 images [V, size, size, 3] and masks [V, size, size] (numpy).  mesh: (verts, faces[, uvs,
    faces_uv]) or a prepared Subject; texture: uint8 [h, w, 3] with sides that are multiples of 8, or None (albedo 1; ignored with a
    Subject); prt: the subject's transfer vectors [nv, 9] (Subject.prt(), computed once by the caller), or None for the analytic,
    unshadowed transfer of the vertex normals; params: the views' PARAM dicts (view_param); lights: [V, 9, 3] or one [9, 3], camera
    frame.  Each view is rastered at size * ms, shaded and box-resolved.  device='cpu' runs the host twins and gives the same bytes."""
    from . import native
    size, ms = int(size), int(ms)
    sub = mesh if isinstance(mesh, Subject) else Subject(mesh, texture, device)
    lights = np.asarray(lights, np.float64)
    lights = np.broadcast_to(lights, (len(params), 9, 3)) if lights.ndim == 2 else lights
    if lights.shape != (len(params), 9, 3):
        raise ValueError("lights: [%d, 9, 3] or [9, 3] expected, not %s" % (len(params), lights.shape))
    images, masks = np.empty((len(params), size, size, 3), np.uint8), np.empty((len(params), size, size), np.uint8)
    big = size * ms
    tex = dict(texture=sub.texture, faces_uv=sub.faces_uv, uvs=sub.uvs) if sub.textured else {}
    for k, param in enumerate(params):
        calib = data.param_calib(param, size)[0]
        R = np.asarray(param["R"], np.float64)
        if prt is not None:
            how = dict(prt=prt, light=sh_rotate(lights[k], R.T))
        else:
            how = dict(normals=sub.normals if sub.host else sub.normals_dev, normal_matrix=R, light=lights[k])
        if sub.host:
            face, _, bary = native.mesh_raster_host(sub.verts, sub.faces, calib, big)
            rgba = native.mesh_shade_prt_host(sub.verts, sub.faces, calib, face, bary, **how, **tex)
            images[k], masks[k] = native.image_resolve(rgba, ms, host=True)
        else:
            face, bary = native.mesh_raster(sub.mesh, calib, big, want_bary=True)
            rgba = native.mesh_shade_prt(sub.mesh, calib, face, bary, **how, **tex)
            rgb, mask = native.image_resolve(rgba, ms)
            images[k], masks[k] = rgb.cpu().numpy(), mask.cpu().numpy()
    return images, masks


# ---------------------------------------------------------------- the dataroot's files
def view_stem(yaw, pitch):
    return "%d_%d_%02d" % (int(yaw), int(pitch), 0)


def view_paths(root, name, yaw, pitch):
    """The three files of a view, in the names data.TrainDataset opens."""
    stem = view_stem(yaw, pitch)
    return (os.path.join(root, "RENDER", name, stem + ".jpg"), os.path.join(root, "MASK", name, stem + ".png"),
            os.path.join(root, "PARAM", name, stem + ".npy"))


def write_view(root, name, yaw, pitch, image, mask, param, light):
    """Write one view's RENDER jpg, MASK png and PARAM npy (the PARAM dict plus 'sh', the light).  The PARAM file goes last and by
    rename: a view whose three files exist is complete."""
    from PIL import Image
    render_path, mask_path, param_path = view_paths(root, name, yaw, pitch)
    for p in (render_path, mask_path, param_path):
        os.makedirs(os.path.dirname(p), exist_ok=True)
    Image.fromarray(np.asarray(image, np.uint8)).save(render_path, quality=95)
    Image.fromarray(np.asarray(mask, np.uint8)).save(mask_path)
    tmp = param_path + ".tmp.npy"
    np.save(tmp, dict(param, sh=np.asarray(light, np.float64)), allow_pickle=True)
    os.replace(tmp, param_path)
