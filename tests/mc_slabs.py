"""What marching cubes' ranged and slab extraction must return, DERIVED from the oracle's mesh of the whole volume.

Lewiner's sweep has axis 0 outermost and hands out vertex / face numbers in order of first use, so the oracle's mesh of
vol[:L + 1] (the cell layers [0, L)) is a PREFIX - vertices and faces - of its mesh of the whole volume.  prefix_counts asserts
that as it goes; everything else follows from it:

  * a range extraction that has seen the cell layers [0, L) holds the first prefix_counts[L] vertices / faces;
  * a slab of cell layers [b0, b1) - the voxel planes b0 .. b1 - owns the vertices / faces those layers create, numbers them
    from 0 and refers to the vertices of the slab below (they sit on x- or y-edges of plane b0) as -(2 + slot),
    slot = axis * n1 * n2 + y * n2 + x  (axis 0: the x-edge starting at voxel (y, x), 1: the y-edge), as include/surs.h states
    for surs_mc_lewiner_range_slab;
  * the ids it hands to the slab above are the local numbers of its vertices on the x- / y-edges of plane b1;
  * fixup() - v >= 0 -> v + own_offset, v < 0 -> below_ids[-v - 2] + below_offset - and concatenation give the whole mesh back
    (tests/test_mc_slabs_host.py checks exactly that, without a GPU, for every volume and split the GPU tests use).

Used by tests/test_dist_cpu.py (the host protocol), tests/test_mc_slabs_host.py and tests/test_gpu_mc_ranges.py."""
import hashlib

import numpy as np

import mc_volumes
import oracle

UNDEFINED = -7   # top-plane ids of edges the surface does not cross: the kernels leave them undefined

_cache = {}


def _key(vol, level):
    return (hashlib.sha1(np.ascontiguousarray(vol, np.float32).tobytes()).hexdigest(), vol.shape, float(level))


def mesh(vol, level):
    """The oracle's (verts, faces, normals, values) of `vol`, cached (read-only arrays)."""
    k = _key(vol, level)
    if k not in _cache:
        out = oracle.marching_cubes_lewiner(np.ascontiguousarray(vol, np.float32), level)
        for a in out:
            a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def prefix_counts(vol, level):
    """int array [n0, 2]: (n_verts, n_faces) after the cell layers [0, L), L = 0 .. n0 - 1; asserts the prefix property."""
    k = ("prefix",) + _key(vol, level)
    if k in _cache:
        return _cache[k]
    V, F, _, _ = mesh(vol, level)
    n0 = vol.shape[0]
    out = np.zeros((n0, 2), np.int64)
    for L in range(1, n0):
        if L == n0 - 1:
            v, f = V, F
        else:
            try:
                v, f, _, _ = oracle.marching_cubes_lewiner(np.ascontiguousarray(vol[:L + 1], np.float32), level)
            except (ValueError, RuntimeError):   # level outside these planes' range / no surface yet
                v, f = V[:0], F[:0]
            assert np.array_equal(v, V[:len(v)]) and np.array_equal(f, F[:len(f)]), "not a prefix of the whole mesh at L = %d" % L
        out[L] = len(v), len(f)
    assert np.all(np.diff(out, axis=0) >= 0)
    out.setflags(write=False)
    _cache[k] = out
    return out


def slabs(vol, level, bounds):
    """bounds = [0 = b_0 < b_1 < ... < b_k = n0 - 1]: slab i holds the cell layers [b_i, b_i+1) = the voxel planes b_i .. b_i+1 (the
    last one is the next slab's first: the halo).  For every slab a dict:
        verts   float32 [v, 3]  its own vertices, whole-grid coordinates
        faces   int32 [f, 3]    local numbering, -(2 + slot) for vertices of the slab below
        ids     int32 [2, n1, n2]  local ids of its vertices on the x- (0) / y-edges (1) of its top plane, UNDEFINED elsewhere
        counts  (n_verts, n_faces, min, max of its planes)"""
    V, F, _, _ = mesh(vol, level)
    n0, n1, n2 = vol.shape
    bounds = [int(b) for b in bounds]
    assert bounds[0] == 0 and bounds[-1] == n0 - 1 and all(a < b for a, b in zip(bounds, bounds[1:])), bounds
    pc = prefix_counts(vol, level)
    out = []
    for b0, b1 in zip(bounds, bounds[1:]):
        (v0, f0), (v1, f1) = pc[b0], pc[b1]
        faces = F[f0:f1].astype(np.int64)
        assert faces.size == 0 or faces.max() < v1
        ref = faces < v0
        pos = V[faces[ref]]                       # vertices of the slab below: on plane b0, on an x- or a y-edge
        assert np.all(pos[:, 0] == b0)
        on_x, on_y = pos[:, 2] != np.floor(pos[:, 2]), pos[:, 1] != np.floor(pos[:, 1])
        assert np.all(on_x ^ on_y)
        slot = np.where(on_x, 0, n1 * n2) + np.floor(pos[:, 1]).astype(np.int64) * n2 + np.floor(pos[:, 2]).astype(np.int64)
        faces[ref] = -(2 + slot)
        faces[~ref] -= v0
        own = V[v0:v1]
        ids = np.full((2, n1, n2), UNDEFINED, np.int32)
        for k in np.nonzero(own[:, 0] == b1)[0]:
            p = own[k]
            on_x, on_y = p[2] != np.floor(p[2]), p[1] != np.floor(p[1])
            assert on_x ^ on_y, "a vertex exactly on a voxel: choose another volume / level"
            y, x = int(np.floor(p[1])), int(np.floor(p[2]))
            assert ids[0 if on_x else 1, y, x] == UNDEFINED
            ids[0 if on_x else 1, y, x] = k
        mm = vol[b0:b1 + 1]
        out.append(dict(verts=own.copy(), faces=faces.astype(np.int32), ids=ids,
                        counts=(int(v1 - v0), int(f1 - f0), float(mm.min()), float(mm.max()))))
    return out


def fixup(faces, own_offset, below_ids, below_offset):
    """surs_mc_slab_fixup in numpy: a slab's faces in the whole mesh's numbering (a new array)."""
    a = np.asarray(faces).astype(np.int64).reshape(-1)
    neg = a < 0
    out = a + own_offset
    if neg.any():
        looked_up = np.asarray(below_ids).reshape(-1)[-a[neg] - 2]
        assert np.all(looked_up != UNDEFINED), "a face refers to an edge the slab below has no vertex on"
        out[neg] = looked_up.astype(np.int64) + below_offset
    return out.astype(np.int32).reshape(-1, 3)


def chain(slab_list):
    """Renumber the slabs bottom-up with fixup() and concatenate: (verts, faces) of the whole mesh."""
    offs = np.concatenate([[0], np.cumsum([s["counts"][0] for s in slab_list])]).astype(np.int64)
    faces = []
    for i, s in enumerate(slab_list):
        assert s["verts"].shape == (s["counts"][0], 3) and s["faces"].shape == (s["counts"][1], 3)
        below = slab_list[i - 1]["ids"] if i else np.zeros(0, np.int32)
        assert i or not (s["faces"] < 0).any()
        faces.append(fixup(s["faces"], int(offs[i]), below, int(offs[i - 1]) if i else 0))
    return np.concatenate([s["verts"] for s in slab_list]), np.concatenate(faces)


# ------------------------------------------------------------------ the volumes and splits of the slab tests (CPU and GPU)

def slab_volume(name):
    return mc_volumes.CASES[name]()


SLAB_VOLUMES = ("noise24", "aniso")      # aniso: 20 x 31 x 17, n1 != n2


def splits(n0):
    """Ragged splits of the n0 - 1 cell layers into 2, 3 and 5 slabs; the 3- and 5-slab ones have a slab of ONE cell layer in
    the middle, the 5-slab one also at the top (a two-plane slab: its ring is two planes whatever mc_ring says)."""
    c = n0 - 1
    assert c >= 12
    return [[0, 2 * c // 5, c], [0, c // 3, c // 3 + 1, c], [0, 3, 4, c // 2, c - 1, c]]


# ------------------------------------------------------------------ levels a float cannot hold (test_gpu_mc_ranges)

def tenths_volume(shape=(12, 10, 14)):
    """Multiples of float32(0.1): a tenth of the voxels EQUAL each of the levels below once it is rounded to float, so a kernel that
    compares in float on the wrong side of the double level classifies them wrongly."""
    return np.round(mc_volumes.noise(shape, 8) * 10).astype(np.float32) * np.float32(0.1)


TENTHS_LEVELS = (0.1, 0.3, 0.7, float(np.float32(0.3)))
# shape -> the range the number of voxels equal to (float)level lies in, for every level above (a tenth of the voxels, give or take)
TENTHS_EQUAL = {(12, 10, 14): (160, 180), (12, 10, 16): (160, 230)}
