"""Marching cubes' chunked, ranged and slab extraction against the oracle (and what tests/mc_slabs.py derives from it).

The vertex-id tables are a ring of planes (option mc_ring, default 258) walked in chunks of ring - 1 cell layers, so at the default
every volume of a few thousand cells is one chunk without a wrap.  Here the ring is driven small - 3, 4, 5, 6, 7, n0 - 1 planes - and
every path built around the one-piece core runs on such volumes: chunks, ranges through MeshStream, slabs, the capacity walk, NaN
behind the first chunk; plus what the small volumes of test_gpu_mc.py do not reach: extents of 2 (plain-division addressing),
levels a float cannot hold, more than one scan group.  Vertices, faces and values bit for bit, normals within 1e-4 (float
atomics reorder the sums).  No assertion compares one GPU path with another."""
import ctypes as C

import numpy as np
import pytest
import torch

import mc_slabs
import mc_volumes

pytestmark = pytest.mark.gpu

DEFAULT_RING = 258
E_CAPACITY = -6
IDENTITY = np.eye(4)[:3].reshape(-1)
# a non-identity index -> world matrix (rows 0..2 of the 4 x 4)
MAT = np.array([[0.5, 0.015625, -0.03125, -3.0], [0.046875, -0.25, 0.0625, 2.0], [0.0, 0.078125, 2.0, 0.5]])


def _smooth(shape):
    """The smooth field of test_gpu_mc.py::test_both_emit_paths_against_the_oracle."""
    ax = [np.linspace(-1, 1, n, dtype=np.float32) for n in shape]
    z, y, x = np.meshgrid(*ax, indexing="ij")
    return (1.0 / (1.0 + np.exp(9.0 * (np.sqrt(x * x + 1.3 * y * y + 0.8 * z * z) - 0.55)))).astype(np.float32)


VOLUMES = {
    "noise24": mc_volumes.CASES["noise24"],
    "aniso": mc_volumes.CASES["aniso"],
    "blob40": mc_volumes.CASES["blob40"],
    "smooth": lambda: (_smooth((23, 36, 30)), 0.5),
}


@pytest.fixture(scope="module")
def gpu():
    from surs_amd import native
    return native, native.require_gpu()


@pytest.fixture
def at_ring(gpu):
    """use(ring, shape, chunked=True) -> a FRESH native.Workspace with the library option mc_ring set to `ring` (None: the default is
    left alone); the option must not change under a workspace, and it is put back afterwards.  That the option took effect is asserted
    from the workspace size: n0 > ring planes under `ring` need what a volume of `ring` planes needs under the default."""
    native, dev = gpu
    lib = native.lib()
    prev = native.get_option("mc_ring")
    native.set_option("mc_ring", DEFAULT_RING)

    def use(ring, shape, chunked=True):
        n0, n1, n2 = shape
        if ring is not None:
            assert 3 <= ring < DEFAULT_RING
            probe = max(n0, ring + 1)
            want = lib.surs_mc_workspace_bytes(ring, n1, n2)       # under the default: ring planes, ring - 1 layers per chunk
            assert lib.surs_mc_workspace_bytes(probe, n1, n2) > want
            native.set_option("mc_ring", ring)
            assert native.get_option("mc_ring") == ring
            assert lib.surs_mc_workspace_bytes(probe, n1, n2) == want
            if chunked:
                assert ring < n0, "chunking is the point here: the volume must not fit the ring"
        return native.Workspace(dev)

    yield use
    native.set_option("mc_ring", prev)
    assert native.get_option("mc_ring") == prev


def _dev(gpu, a):
    return torch.from_numpy(np.array(a, order="C")).to(gpu[1])      # (a copy: the cached oracle arrays are read-only)


def _extract(gpu, ws, vol, level, key=None):
    v, f, n, val = gpu[0].marching_cubes_lewiner(_dev(gpu, vol), level, ws, key=key)
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), val.cpu().numpy()


def _assert_mesh(got, vol, level):
    V, F, N, VAL = mc_slabs.mesh(vol, level)
    v, f, n, val = got
    assert v.shape == V.shape and f.shape == F.shape
    assert np.array_equal(f, F)
    assert np.array_equal(v, V)
    assert np.array_equal(val, VAL)
    assert np.abs(n - N).max() < 1e-4


# ------------------------------------------------------------------ one-piece extraction in chunks

@pytest.mark.parametrize("ring", [3, 4, 7, "n0-1"])
@pytest.mark.parametrize("name", list(VOLUMES))
def test_chunked_extraction_against_the_oracle(gpu, at_ring, name, ring):
    """Rings of 3 and 4 planes wrap every one or two chunks, n0 - 1 gives one full chunk and a ragged one of a single layer.  Normals
    and values accumulate across the chunk edges."""
    vol, level = VOLUMES[name]()
    r = vol.shape[0] - 1 if ring == "n0-1" else ring
    ws = at_ring(r, vol.shape)
    _assert_mesh(_extract(gpu, ws, vol, level), vol, level)


@pytest.mark.parametrize("name", ["blob40", "smooth", "noise24"])
def test_reclassifying_emit_pass_in_chunks(gpu, at_ring, name):
    """mc_emit_reclassify = 1 at ring 4: the re-classifying emit pass on fields that take the stored codes otherwise, chunk by chunk."""
    native = gpu[0]
    vol, level = VOLUMES[name]()
    ws = at_ring(4, vol.shape)
    assert native.get_option("mc_emit_reclassify") == 0
    native.set_option("mc_emit_reclassify", 1)
    try:
        got = _extract(gpu, ws, vol, level)
    finally:
        native.set_option("mc_emit_reclassify", 0)
    _assert_mesh(got, vol, level)


# ------------------------------------------------------------------ thin volumes, levels, scan groups

@pytest.mark.parametrize("ring", [None, 3])
@pytest.mark.parametrize("shape", [(9, 2, 13), (11, 7, 2), (2, 9, 10), (13, 6, 5)])
def test_thin_volumes(gpu, at_ring, shape, ring):
    """An extent of 2 is one cell: n1 == 2 takes the plain-division addressing (cy < 2), n2 == 2 rows of one cell padded to four,
    n0 == 2 a ring of two planes."""
    vol = mc_volumes.noise(shape, 11 + sum(shape))
    ws = at_ring(ring, shape, chunked=False)
    _assert_mesh(_extract(gpu, ws, vol, 0.5), vol, 0.5)


@pytest.mark.parametrize("level", mc_slabs.TENTHS_LEVELS)
@pytest.mark.parametrize("shape", list(mc_slabs.TENTHS_EQUAL))
def test_levels_a_float_cannot_hold(gpu, at_ring, shape, level):
    """160 - 180 voxels equal (float)level; inside means (double)f - level > 0 with the level in double.  The oracle has 1747 vertices
    at 0.3 and 2103 at float32(0.3) (tests/test_mc_slabs_host.py): deciding in float on the wrong side cannot pass both.
    (12, 10, 14) takes the count pass's scalar rows, (12, 10, 16) - n2 a multiple of 4 - the wavefront masks every 512^3 field takes."""
    vol = mc_slabs.tenths_volume(shape)
    lo, hi = mc_slabs.TENTHS_EQUAL[shape]
    assert lo <= int((vol == np.float32(level)).sum()) <= hi
    ws = at_ring(None, vol.shape)
    _assert_mesh(_extract(gpu, ws, vol, level), vol, level)


def _wavy_column(shape):
    """A smooth field whose surface crosses every plane of axis 0: a column along axis 0 with a waist that wanders."""
    n0, n1, n2 = shape
    z, y, x = np.meshgrid(np.arange(n0, dtype=np.float64), np.linspace(-1, 1, n1), np.linspace(-1, 1, n2), indexing="ij")
    r = np.sqrt((x - 0.1 * np.sin(0.9 * z)) ** 2 + 1.2 * (y + 0.08 * np.cos(0.7 * z)) ** 2)
    return (1.0 / (1.0 + np.exp(14.0 * (r - 0.6 - 0.05 * np.sin(5.0 * x + z))))).astype(np.float32)


@pytest.mark.parametrize("field", ["noise", "smooth"])
def test_more_than_one_scan_group(gpu, at_ring, field):
    """The emit passes add group_offsets[block / 1024] to a block's offsets; 14 x 300 x 300 is 1139 blocks of 1024 padded cells:
    two groups.  Noise takes the re-classifying pass (more than half of the cells are active), the smooth field the stored codes."""
    shape = (14, 300, 300)
    n0, n1, n2 = shape
    padded = (n0 - 1) * (n1 - 1) * ((n2 - 1 + 3) // 4 * 4)
    assert padded > 1024 * 1024                     # blocks of 1024 cells, groups of 1024 blocks
    ncells = (n0 - 1) * (n1 - 1) * (n2 - 1)
    vol = mc_volumes.noise(shape, 21) if field == "noise" else _wavy_column(shape)
    V, F, _, _ = mc_slabs.mesh(vol, 0.5)
    if field == "noise":
        assert len(F) > 0.5 * ncells                # (every active cell has at least one triangle)
    else:
        assert 1000 < len(F) < 0.1 * ncells
        # cells of the second group: padded index >= 2^20, that is behind cell layer 2^20 / ((n1 - 1) * 300) = 11.7
        assert (V[:, 0] > 12.0).sum() > 100
    ws = at_ring(None, shape)
    _assert_mesh(_extract(gpu, ws, vol, 0.5), vol, 0.5)


# ------------------------------------------------------------------ ranges through MeshStream

def _schedules(n0, ring):
    long_step = min(n0 - 1, 2 + (ring if ring is not None else n0) + 1)        # one advance of more than ring - 1 layers
    return {
        "every_layer": list(range(1, n0)),
        "ragged": [5, 6, 17, n0 - 1],
        "long": [2, long_step, n0 - 1],
        "repeated": [4, 4, 9, 9, n0 - 1, n0 - 1],
    }


def _assert_world(world, V, mat):
    """mat[:3,:3] @ v + mat[:3,3] in float64: within the rounding of a three-term sum of products in double, in any order, with
    or without fused multiply-adds (4 u (|m| |v| + |t|), u = 2^-53) - seven decimal digits below a wrong vertex."""
    m = np.asarray(mat, np.float64).reshape(3, 4)
    v = V.astype(np.float64)
    ref = v @ m[:, :3].T + m[:, 3]
    bound = 4 * 2.0 ** -53 * (np.abs(v) @ np.abs(m[:, :3]).T + np.abs(m[:, 3]))
    assert world.shape == ref.shape and world.dtype == np.float64
    assert np.all(np.abs(world - ref) <= bound)


@pytest.mark.parametrize("schedule", ["every_layer", "ragged", "long", "repeated"])
@pytest.mark.parametrize("ring", [3, 6, None])
@pytest.mark.parametrize("name", ["noise24", "aniso"])
def test_ranges_through_meshstream(gpu, at_ring, name, ring, schedule):
    native, dev = gpu
    vol, level = VOLUMES[name]()
    n0 = vol.shape[0]
    V, F, N, VAL = mc_slabs.mesh(vol, level)
    pc = mc_slabs.prefix_counts(vol, level)
    ws = at_ring(ring, vol.shape)
    t = _dev(gpu, vol)
    _assert_mesh(_extract(gpu, ws, vol, level, key="field"), vol, level)      # the one-piece call that sizes the stream's buffers
    Vd, Fd = _dev(gpu, V), _dev(gpu, F)
    steps = _schedules(n0, ring)[schedule]
    if schedule == "long" and ring is not None:
        assert max(b - a for a, b in zip(steps, steps[1:])) > ring - 1
    s = native.MeshStream(ws, "field", t, MAT.reshape(-1), level, True)
    seen = 0
    for L in steps:
        s.advance(L)
        s.mc.synchronize()
        assert L >= seen
        seen = L
        assert s.layers == L and not s.overflow
        nv, nf = s.run.n_verts, s.run.n_faces
        assert (nv, nf) == tuple(pc[L])
        assert torch.equal(s.verts[:nv], Vd[:nv]) and torch.equal(s.faces[:nf], Fd[:nf])
        assert s.run.vmin == vol[:L + 1].min() and s.run.vmax == vol[:L + 1].max()     # the planes 0 .. L it has read
    world, faces, normals, values = s.finish()
    assert np.array_equal(faces, F)
    _assert_world(world, V, MAT)
    assert np.array_equal(values, VAL)
    assert np.abs(normals - N).max() < 1e-4
    assert np.array_equal(s.verts[:len(V)].cpu().numpy(), V)


@pytest.mark.parametrize("fits_layers", [0, 10])
def test_meshstream_overflow(gpu, at_ring, fits_layers):
    """Buffers sized too small (ws.mc_capacity): `overflow` is set, finish() returns None, what was extracted before stays a prefix,
    and the workspace extracts the volume correctly afterwards."""
    native, dev = gpu
    vol, level = VOLUMES["noise24"]()
    V, F, _, _ = mc_slabs.mesh(vol, level)
    pc = mc_slabs.prefix_counts(vol, level)
    ws = at_ring(3, vol.shape)
    _assert_mesh(_extract(gpu, ws, vol, level, key="field"), vol, level)
    ws.mc_capacity["field"] = (int(pc[fits_layers, 0]) + 7, int(pc[fits_layers, 1]) + 5)
    s = native.MeshStream(ws, "field", _dev(gpu, vol), IDENTITY, level, True)
    for L in range(1, fits_layers + 1):
        s.advance(L)
        assert not s.overflow
    s.advance(fits_layers + 1)
    s.advance(fits_layers + 5)
    assert s.overflow and s.layers == fits_layers
    nv, nf = int(pc[fits_layers, 0]), int(pc[fits_layers, 1])
    assert np.array_equal(s.verts[:nv].cpu().numpy(), V[:nv]) and np.array_equal(s.faces[:nf].cpu().numpy(), F[:nf])
    assert s.finish() is None
    _assert_mesh(_extract(gpu, ws, vol, level, key="field"), vol, level)


# ------------------------------------------------------------------ capacity, through the C ABI

@pytest.mark.parametrize("frac", [(0.6, 0.45), (0.3, 0.8), (0.05, 0.05)])
@pytest.mark.parametrize("name", ["noise24", "aniso"])
def test_capacity_walk_across_chunks(gpu, at_ring, name, frac):
    """surs_mc_lewiner at ring 4 (eight / seven chunks) with buffers below the need: SURS_E_CAPACITY, the counts of the whole mesh, the
    rows below the capacities are the mesh's and nothing is written behind them.  Vertices and faces run out in different chunks."""
    native, dev = gpu
    lib = native.lib()
    vol, level = VOLUMES[name]()
    n0, n1, n2 = vol.shape
    V, F, _, _ = mc_slabs.mesh(vol, level)
    ws = at_ring(4, vol.shape)
    cap_v, cap_f, tail = int(frac[0] * len(V)), int(frac[1] * len(F)), 64
    t = _dev(gpu, vol)
    w = ws.get(lib.surs_mc_workspace_bytes(n0, n1, n2))
    verts = torch.full((cap_v + tail, 3), -77.0, dtype=torch.float32, device=dev)
    normals = torch.full((cap_v + tail, 3), -77.0, dtype=torch.float32, device=dev)
    values = torch.full((cap_v + tail,), -77.0, dtype=torch.float32, device=dev)
    faces = torch.full((cap_f + tail, 3), -77, dtype=torch.int32, device=dev)
    counts = native._lib.McCounts()
    rc = lib.surs_mc_lewiner(native._ptr(t), n0, n1, n2, float(level), native._ptr(w), w.numel(), native._ptr(verts),
                             native._ptr(normals), native._ptr(values), cap_v, native._ptr(faces), cap_f, C.byref(counts),
                             native._stream())
    assert rc == E_CAPACITY                 # (returns with the stream synchronised, like the success path)
    assert (counts.n_verts, counts.n_faces) == (len(V), len(F))
    assert counts.vmin == vol.min() and counts.vmax == vol.max()
    for buf, cap in ((verts, cap_v), (normals, cap_v), (values, cap_v), (faces, cap_f)):
        assert bool((buf[cap:] == -77).all()), "written behind the capacity"
    assert np.array_equal(verts[:cap_v].cpu().numpy(), V[:cap_v])
    assert np.array_equal(faces[:cap_f].cpu().numpy(), F[:cap_f])
    _assert_mesh(_extract(gpu, ws, vol, level), vol, level)      # the workspace is usable afterwards


# ------------------------------------------------------------------ slab mode, in one process

def _slab_advances(n_layers):
    return sorted({a for a in (1, 2, 5, n_layers - 2) if 0 < a < n_layers})


def _forget_tables(ws, key):
    """Overwrite the field's private marching-cubes workspace (it persists between extractions) with a value that is no vertex id:
    what is read from it afterwards - the top-plane ids - was written by the extraction under test, not left by an earlier one."""
    w = ws.mesh_ws.get(key)
    if w is not None:
        w.fill_(0x7F)
        torch.cuda.synchronize()          # (the extraction may run on another stream)


@pytest.mark.parametrize("mode", ["one_piece", "stream"])
@pytest.mark.parametrize("ring", [3, 5, None])
@pytest.mark.parametrize("name", mc_slabs.SLAB_VOLUMES)
def test_slab_mode_against_the_derived_slabs(gpu, at_ring, name, ring, mode):
    """Every slab of ragged splits into 2, 3 and 5 (a slab of one cell layer among them): vertices, local faces with their
    -(2 + slot) references, counts and the top-plane ids as tests/mc_slabs.py derives them from the oracle; then the slabs
    chained through surs_mc_slab_fixup must be the oracle's mesh."""
    native, dev = gpu
    lib = native.lib()
    vol, level = mc_slabs.slab_volume(name)
    n0, n1, n2 = vol.shape
    V, F, _, _ = mc_slabs.mesh(vol, level)
    pc = mc_slabs.prefix_counts(vol, level)
    ws = at_ring(ring, vol.shape)
    t = _dev(gpu, vol)
    for bounds in mc_slabs.splits(n0):
        ref = mc_slabs.slabs(vol, level, bounds)
        got = []
        for i, (b0, b1) in enumerate(zip(bounds, bounds[1:])):
            key = ("slab", i)
            sv = t[b0:b1 + 1].contiguous()            # the slab with its halo plane
            _forget_tables(ws, key)
            world, faces, run, w = native.slab_mesh_one_piece(ws, key, sv, IDENTITY, level, b0)
            if mode == "stream":
                # (the one-piece call has sized the buffers, as in dist.reconstruction_sharded; its ids must not serve the check below)
                r1 = ref[i]
                assert (run.n_verts, run.n_faces) == r1["counts"][:2] and np.array_equal(faces.cpu().numpy(), r1["faces"])
                _forget_tables(ws, key)
                s = native.MeshStream(ws, key, sv, IDENTITY, level, False, zoff=b0)
                for L in _slab_advances(b1 - b0):
                    s.advance(L)
                    s.mc.synchronize()
                    assert s.layers == L and not s.overflow
                    assert (s.run.n_verts, s.run.n_faces) == tuple(pc[b0 + L] - pc[b0])
                world, faces = s.finish()
                run, w = s.run, s.w
            r = ref[i]
            assert (run.n_verts, run.n_faces, run.vmin, run.vmax) == r["counts"]
            assert np.array_equal(world.cpu().numpy(), r["verts"].astype(np.float64))     # whole-grid coordinates, identity matrix
            assert np.array_equal(faces.cpu().numpy(), r["faces"])
            top = torch.full((2, n1, n2), -12345, dtype=torch.int32, device=dev)
            native.check(lib.surs_mc_slab_top_ids(native._ptr(w), w.numel(), b1 - b0 + 1, n1, n2, native._ptr(top), native._stream()))
            defined = r["ids"] != mc_slabs.UNDEFINED
            assert defined.sum() >= 1
            assert np.array_equal(top.cpu().numpy()[defined], r["ids"][defined])
            got.append((world, faces.clone(), top, run.n_verts))
        offs = np.concatenate([[0], np.cumsum([g[3] for g in got])])
        for i, (world, faces, top, _) in enumerate(got):
            below = got[i - 1][2] if i else torch.zeros(1, dtype=torch.int32, device=dev)
            native.check(lib.surs_mc_slab_fixup(native._ptr(faces), faces.shape[0], int(offs[i]), native._ptr(below),
                                                int(offs[i - 1]) if i else 0, native._stream()))
        torch.cuda.synchronize()
        assert np.array_equal(torch.cat([g[1] for g in got]).cpu().numpy(), F)
        assert np.array_equal(torch.cat([g[0] for g in got]).cpu().numpy(), V.astype(np.float64))


# ------------------------------------------------------------------ NaN behind the first chunk

@pytest.mark.parametrize("where", [(23, 5, 7), (13, 23, 0), (12, 0, 23)])
def test_nan_beyond_the_first_chunk(gpu, at_ring, where):
    native, dev = gpu
    from surs_amd._lib import NonFiniteVolumeError
    vol, level = VOLUMES["noise24"]()
    ws = at_ring(4, vol.shape)
    bad = vol.copy()
    bad[where] = np.nan
    assert where[0] > 3                        # not in the planes of the first chunk
    with pytest.raises(NonFiniteVolumeError):
        native.marching_cubes_lewiner(_dev(gpu, bad), level, ws)
    _assert_mesh(_extract(gpu, ws, vol, level), vol, level)      # the workspace is usable afterwards
