"""tests/mc_slabs.py - the reference of tests/test_gpu_mc_ranges.py - checked on its own, without a GPU: the slabs it derives
from the oracle's mesh, chained through its numpy fixup, must give the oracle's mesh back, for every volume and split the GPU
tests use (n1 != n2, slabs of a single cell layer)."""
import numpy as np
import pytest

import mc_slabs


@pytest.mark.parametrize("name", mc_slabs.SLAB_VOLUMES)
def test_prefix_counts(name):
    vol, level = mc_slabs.slab_volume(name)
    V, F, _, _ = mc_slabs.mesh(vol, level)
    pc = mc_slabs.prefix_counts(vol, level)          # asserts the prefix property for every L
    assert pc.shape == (vol.shape[0], 2) and tuple(pc[0]) == (0, 0) and tuple(pc[-1]) == (len(V), len(F))
    assert np.all(np.diff(pc[:, 0]) > 0) and np.all(np.diff(pc[:, 1]) > 0)   # noise: every layer has a surface
    # a vertex of the first L layers lies in the planes 0 .. L, the first vertex after them does not lie below plane L - 1
    for L in range(1, vol.shape[0]):
        assert V[:pc[L, 0], 0].max() <= L
        if pc[L, 0] < len(V):
            assert V[pc[L, 0], 0] >= L


@pytest.mark.parametrize("name", mc_slabs.SLAB_VOLUMES)
def test_chained_slabs_give_the_oracle_mesh_back(name):
    vol, level = mc_slabs.slab_volume(name)
    V, F, _, _ = mc_slabs.mesh(vol, level)
    n0, n1, n2 = vol.shape
    all_splits = mc_slabs.splits(n0)
    assert [len(b) - 1 for b in all_splits] == [2, 3, 5]
    assert any(b1 - b0 == 1 for b in all_splits for b0, b1 in zip(b, b[1:]))     # a slab of one cell layer
    for bounds in all_splits:
        sl = mc_slabs.slabs(vol, level, bounds)
        assert sum(s["counts"][0] for s in sl) == len(V) and sum(s["counts"][1] for s in sl) == len(F)
        for s, b0, b1 in zip(sl, bounds, bounds[1:]):
            assert s["verts"].dtype == np.float32 and s["faces"].dtype == np.int32
            assert s["counts"][2] == vol[b0:b1 + 1].min() and s["counts"][3] == vol[b0:b1 + 1].max()
            assert s["verts"][:, 0].min() >= b0 and s["verts"][:, 0].max() <= b1
            f = s["faces"]
            assert f.max() < s["counts"][0] and f.min() >= -(2 + 2 * n1 * n2 - 1)
            assert (f < 0).any() == (b0 > 0)            # every upper slab refers to the slab below, the bottom one to nobody
            defined = s["ids"] != mc_slabs.UNDEFINED
            assert defined.sum() >= 1                   # (noise: hundreds)
            ids = s["ids"][defined]
            assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < s["counts"][0]
            assert np.all(s["verts"][ids, 0] == b1)
            # the slot formula with n1 != n2: entry [axis, y, x] is the vertex on the edge starting at voxel (b1, y, x)
            ax, y, x = np.nonzero(defined)
            p = s["verts"][s["ids"][ax, y, x]]
            assert np.all(np.floor(p[:, 1]) == y) and np.all(np.floor(p[:, 2]) == x)
            assert np.all((p[:, 2] != x) == (ax == 0)) and np.all((p[:, 1] != y) == (ax == 1))
        v, f = mc_slabs.chain(sl)
        assert np.array_equal(v, V) and np.array_equal(f, F)


def test_the_reference_can_fail():
    """A face that refers to an edge without a vertex is an error - ids stored one slot off hit such edges - and two ids
    exchanged give other faces."""
    vol, level = mc_slabs.slab_volume("aniso")
    V, F, _, _ = mc_slabs.mesh(vol, level)
    sl = mc_slabs.slabs(vol, level, mc_slabs.splits(vol.shape[0])[0])
    with pytest.raises(AssertionError):
        mc_slabs.fixup(sl[1]["faces"], sl[0]["counts"][0], np.full_like(sl[0]["ids"], mc_slabs.UNDEFINED), 0)
    ids = sl[0]["ids"]
    flat = ids.reshape(-1)
    defined = np.nonzero(flat != mc_slabs.UNDEFINED)[0]
    used = np.unique(-sl[1]["faces"][sl[1]["faces"] < 0] - 2)
    assert np.array_equal(used, defined)              # the slab above uses every vertex of the plane, and no other slot
    assert (np.roll(flat, 1)[used] == mc_slabs.UNDEFINED).any()
    with pytest.raises(AssertionError):
        mc_slabs.chain([dict(sl[0], ids=np.roll(flat, 1).reshape(ids.shape)), sl[1]])
    swapped = flat.copy()
    swapped[defined[[0, -1]]] = swapped[defined[[-1, 0]]]
    v, f = mc_slabs.chain([dict(sl[0], ids=swapped.reshape(ids.shape)), sl[1]])
    assert np.array_equal(v, V) and f.shape == F.shape and not np.array_equal(f, F)


def test_the_levels_a_float_cannot_hold():
    """The volumes of test_gpu_mc_ranges' level test: multiples of float32(0.1), so that a tenth of the voxels EQUAL the level rounded
    to float, and whether they are inside is decided by (double)f - level > 0 with the level in DOUBLE: 0.3 and float32(0.3) give
    different meshes."""
    for shape, (lo, hi) in mc_slabs.TENTHS_EQUAL.items():
        vol = mc_slabs.tenths_volume(shape)
        counts = {}
        for level in mc_slabs.TENTHS_LEVELS:
            n = int((vol == np.float32(level)).sum())
            assert lo <= n <= hi
            counts[level] = len(mc_slabs.mesh(vol, level)[0])
        assert counts[0.3] != counts[float(np.float32(0.3))]
        if shape == (12, 10, 14):
            assert counts[0.3] == 1747 and counts[float(np.float32(0.3))] == 2103
