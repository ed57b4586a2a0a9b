"""The column sweep's host sequence - workspace map, R-vector paths, kernel dispatch, batch loop, octree level, point runs, probe -
returns, byte for byte, what the library returned BEFORE that sequence was restructured (tests/golden/sweep_digests.json, written by
tools/gen_golden_sweep_digests.py under that library): the cases of tests/sweep_digests.py, which the 16-column grid of
tests/test_gpu_column_bits.py cannot reach.  Equality of SHA-256 digests: no tolerance."""
import json
import os

import numpy as np
import pytest

import sweep_digests as sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return sd.Context()


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, sd.FIXTURE)) as f:
        return json.load(f)


def _hold(name, words, recorded):
    assert words is not None, "%s: the library reported 0 columns" % name
    assert sd.is_a_field(words), "%s: not a finite, varying field" % name
    got, want = sd.digest(words), recorded["sha256"][name]
    print("%s: %d words, digest %s, recorded %s" % (name, words.size, got[:16], want[:16]))
    assert got == want, "%s differs from the recorded bytes" % name


def test_the_fixture_records_every_case(recorded):
    assert sorted(recorded["sha256"]) == sorted(sd.DIGEST_CASES)
    assert sorted(recorded["probe_bits"]) == sorted(n for n, _ in sd.PROBE)


@pytest.mark.parametrize("name,grid,gain,prec,kv", sd.DENSE, ids=[c[0] for c in sd.DENSE])
def test_dense_sweep_reproduces_the_recorded_bytes(ctx, recorded, name, grid, gain, prec, kv):
    words = ctx.dense(grid, gain, prec, kv)
    assert words.shape == (2,) + sd.GRIDS[grid]
    _hold(name, words, recorded)


@pytest.mark.parametrize("name,prec", sd.OCTREE, ids=[c[0] for c in sd.OCTREE])
def test_octree_level_reproduces_the_recorded_bytes(ctx, recorded, name, prec):
    words = ctx.octree(prec)
    assert words.shape == (2, len(sd.dirty_points()))
    _hold(name, words, recorded)


@pytest.mark.parametrize("name,prec", sd.POINT_RUNS, ids=[c[0] for c in sd.POINT_RUNS])
def test_point_runs_reproduce_the_recorded_bytes_on_both_calls(ctx, recorded, name, prec):
    first, second = ctx.point_runs(prec)      # (None: 0 columns reported)
    _hold(name + "_call1", first, recorded)
    _hold(name + "_call2", second, recorded)
    assert first.shape == second.shape == (2, sd.RUNS * sd.RUN_LEN)


@pytest.mark.parametrize("name,gain", sd.PROBE, ids=[c[0] for c in sd.PROBE])
def test_probe_reproduces_the_recorded_floats(ctx, recorded, name, gain):
    got = ["%08x" % int(b) for b in ctx.probe(gain)]
    print("%s: listed (lr, hr bound) = %s, bits %s, recorded %s" % (name, ctx.probe(gain).view(np.float32), got, recorded["probe_bits"][name]))
    assert got == recorded["probe_bits"][name], "%s differs from the recorded floats" % name
