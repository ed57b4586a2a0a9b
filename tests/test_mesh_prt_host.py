"""Host checks of the per-vertex PRT (csrc/surs_mesh_prt.h through surs_mesh_prt_host, the kernels' twin) against the float64 model
tests/prt_ref.py and the closed form A_l Y_i(n).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import prt_ref as pr
from surs_amd import _lib, native, render


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _twin(scene, dirs, offset, **kw):
    v, f, n = scene
    return native.mesh_prt_host(v, f, n, dirs, offset, **kw)


# ---------------------------------------------------------------- (a) rounding: the twin against the float64 sum
def test_twin_matches_float64_sum_on_convex_mesh():
    """Icosphere (convex: nothing is occluded), n = 8: the twin against the float64 sum over the same directions within pr.bound(D),
    derived there from D terms of at most 4 pi / D * 1.1 and fp32 accumulation."""
    scene = pr.icosphere(1)
    dirs = render.prt_directions(8, 0)
    prt, vis = _twin(scene, dirs, 0.05, want_visible=True)
    lit = pr.visibility(scene[0], scene[1], scene[2], dirs, 0.05)
    assert np.array_equal(lit, (scene[2] @ dirs.astype(np.float64).T) > 0)      # convex: lit wherever n . d > 0
    assert np.array_equal(vis.astype(bool), lit)
    want = pr.coefficients(scene[2], dirs, lit)
    gap = np.abs(prt - want).max()
    print("max gap %.3e, bound %.3e" % (gap, pr.bound(len(dirs))))
    assert gap <= pr.bound(len(dirs))


# ---------------------------------------------------------------- (b) sampling: the model against the closed form
def test_model_converges_to_closed_form():
    """The float64 model at n = 40 on the icosphere against A_l Y_i(n).  This is sampling error: the tolerance is MARGIN = 5 times
    the model's own spread (largest standard deviation of a coefficient over the seeds 0 .. 7).  Measured: spread 7.1e-3, largest
    error of seed 0 7.4e-3 (tolerance 3.6e-2); the twin at n = 40 sits within pr.bound(1600) of the model."""
    MARGIN = 5.0
    v, f, n = pr.icosphere(1)
    runs = []
    for seed in range(8):
        dirs = render.prt_directions(40, seed).astype(np.float64)
        lit = (n @ dirs.T) > 0
        if seed == 0:
            assert np.array_equal(pr.visibility(v, f, n, dirs, 0.05), lit)          # the model's visibility: convex, all lit
        runs.append(pr.coefficients(n, dirs, lit))
    runs = np.array(runs)
    spread = float(runs.std(0, ddof=1).max())
    err = float(np.abs(runs[0] - pr.closed_form(n)).max())
    print("spread %.3e, error of seed 0 %.3e, tolerance %.3e" % (spread, err, MARGIN * spread))
    assert err <= MARGIN * spread
    assert spread < 0.05                                                            # and the sum does converge: 4 pi 1.1 / sqrt(1600) scale
    twin = native.mesh_prt_host(v, f, n, render.prt_directions(40, 0), 0.05)
    assert np.abs(twin - runs[0]).max() <= pr.bound(1600)


# ---------------------------------------------------------------- (c) occlusion
SCENES = {"floor_roof": (pr.floor_roof, 1e-3), "torus": (pr.torus_scene, 0.5)}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_occlusion_equals_model(name):
    """Visibility per (vertex, direction) pair EQUALS the float64 model's, except pairs whose float64 ray passes within 1e-4 of the
    bounding-box diagonal of a triangle edge or has |n . d| < 1e-4 - at most 2 % of the pairs (checked: the model alone stays inside
    that cap).  The coefficients are compared with the model run on the twin's visibility for the left-out pairs."""
    make, offset = SCENES[name]
    scene = make()
    v, f, n = scene
    dirs = render.prt_directions(8, 3)
    prt, vis = _twin(scene, dirs, offset, want_visible=True)
    lit, unsure = pr.visibility(v, f, n, dirs, offset, margin=1e-4 * pr.diagonal(v))
    print("%s: %d pairs, %d left out, %d shadowed of %d cast" % (name, lit.size, unsure.sum(), ((n @ dirs.T > 0) & ~lit).sum(),
                                                                  (n @ dirs.T > 0).sum()))
    assert unsure.mean() <= 0.02
    assert ((n @ dirs.astype(np.float64).T > 0) & ~lit).sum() > 0.02 * lit.size           # the scene does shadow
    vis = vis.astype(bool)
    assert np.array_equal(vis[~unsure], lit[~unsure])
    want = pr.coefficients(n, dirs, np.where(unsure, vis, lit))
    assert np.abs(prt - want).max() <= pr.bound(len(dirs))


# ---------------------------------------------------------------- (d) degenerate input, bad arguments
def test_degenerate_input():
    v, f, n = pr.floor_roof()
    dirs = render.prt_directions(8, 1)
    base = native.mesh_prt_host(v, f, n, dirs, 1e-3)
    # a zero-area face over the floor's centre (three collinear points) and a repeated vertex (a face of two equal corners)
    v2 = np.concatenate([v, [[-0.25, 0.25, 0.0], [0.0, 0.25, 0.0], [0.25, 0.25, 0.0], [0.25, 0.25, 0.0]]])
    f2 = np.concatenate([f, [[13, 14, 15], [13, 16, 15], [13, 13, 14]]]).astype(np.int32)
    n2 = np.concatenate([n, np.tile([0.0, 1.0, 0.0], (4, 1))])
    got = native.mesh_prt_host(v2, f2, n2, dirs, 1e-3)
    assert np.array_equal(_bits(got[:len(v)]), _bits(base))                  # they hit nothing
    assert np.isfinite(got).all()
    # a NaN vertex: its own row is 0, its face hits nothing, the others keep their bits
    v3 = np.concatenate([v, [[np.nan, 0.25, 0.0]]])
    f3 = np.concatenate([f, [[9, 10, 13]]]).astype(np.int32)
    n3 = np.concatenate([n, [[0.0, 1.0, 0.0]]])
    got = native.mesh_prt_host(v3, f3, n3, dirs, 1e-3)
    assert np.array_equal(got[13], np.zeros(9, np.float32))
    keep = [i for i in range(13) if i not in (9, 10)]                        # 9 and 10 now skip the new face as their own: no change either
    assert np.array_equal(_bits(got[:13]), _bits(base))
    assert np.isfinite(got[keep]).all()
    n4 = n.copy()
    n4[4] = np.inf                                                           # a non-finite normal
    got = native.mesh_prt_host(v, f, n4, dirs, 1e-3)
    assert np.array_equal(got[4], np.zeros(9, np.float32))


def test_bad_arguments_are_invalid():
    lib = _lib.lib()
    v, f, n = pr.floor_roof()
    v, f, n = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32), np.ascontiguousarray(n, np.float32)
    d = render.prt_directions(2, 0)
    out = np.empty((len(v), 9), np.float32)
    good = [v.ctypes.data, len(v), f.ctypes.data, len(f), n.ctypes.data, d.ctypes.data, len(d), 0.01, out.ctypes.data, None]
    assert lib.surs_mesh_prt_host(*good) == 0
    for pos, bad in ((0, None), (2, None), (4, None), (5, None), (8, None), (1, 0), (3, 0), (6, 0), (7, -1.0), (7, float("nan")),
                     (7, float("inf")), (6, 2 ** 31 - 1)):
        args = list(good)
        args[pos] = bad
        assert lib.surs_mesh_prt_host(*args) == -1, (pos, bad)               # SURS_E_INVALID
    # the device entry refuses the same arguments, and a short or missing workspace, before it launches anything
    need = lib.surs_mesh_prt_workspace_bytes(len(v), len(d))
    assert need >= (len(v) * len(d) + 31) // 32 * 4 and lib.surs_mesh_prt_workspace_bytes(0, 4) == 0
    assert lib.surs_mesh_prt_workspace_bytes(len(v), len(d)) == lib.surs_mesh_prt_workspace_bytes(len(v), len(d))
    dev = good[:9] + [C.c_void_p(16), need - 1, None]
    assert lib.surs_mesh_prt(*dev) == -1
    dev = good[:9] + [None, need, None]
    assert lib.surs_mesh_prt(*dev) == -1
    with pytest.raises(_lib.SursError):
        native.mesh_prt_host(v, f, n, d, -0.5)


def test_workspace_is_bounded_by_visibility_bits():
    """nv ceil(D / 32) words plus a constant, whatever the number of faces (the entry does not even take it)."""
    lib = _lib.lib()
    for nv, D in ((1, 1), (13, 64), (1000, 1600), (100000, 1600), (7, 33)):
        assert lib.surs_mesh_prt_workspace_bytes(nv, D) <= nv * ((D + 31) // 32) * 4 + 256


# ---------------------------------------------------------------- (e) a vertex's bits are its own
def test_vertex_bits_do_not_depend_on_order_or_nv():
    v, f, n = pr.torus_scene()
    dirs = render.prt_directions(5, 2)          # D = 25: no multiple of 32
    base = native.mesh_prt_host(v, f, n, dirs, 0.5)
    perm = np.random.RandomState(5).permutation(len(v))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(v))
    got = native.mesh_prt_host(v[perm], inv[f].astype(np.int32), n[perm], dirs, 0.5)
    assert np.array_equal(_bits(got), _bits(base[perm]))
    far = np.array([[5000.0, 5000.0, 5000.0], [5001.0, 5000.0, 5000.0], [5000.0, 5001.0, 5000.0]])
    v2, n2 = np.concatenate([v, far]), np.concatenate([n, np.tile([0.0, 0.0, 1.0], (3, 1))])
    f2 = np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
    got = native.mesh_prt_host(v2, f2, n2, dirs, 0.5)
    assert np.array_equal(_bits(got[:len(v)]), _bits(base))


def test_default_directions():
    d = render.prt_directions()
    assert d.shape == (1600, 3) and d.dtype == np.float32
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(d, render.prt_directions(40, 0)) and not np.array_equal(d, render.prt_directions(40, 1))
    n = 6
    d = render.prt_directions(n, 9).astype(np.float64)
    i = np.arange(n * n) // n                   # stratum i holds cos theta in (1 - 2 (i + 1) / n, 1 - 2 i / n]
    assert ((d[:, 2] <= 1 - 2 * i / n + 1e-6) & (d[:, 2] >= 1 - 2 * (i + 1) / n - 1e-6)).all()
