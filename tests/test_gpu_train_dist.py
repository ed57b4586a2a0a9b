"""Data-parallel training end to end: each case is ONE run of tools/gpu_train_dist_check.py WORLD MODE, which starts WORLD gloo ranks
that share the one GPU (at most 4 processes) on the `tiny` case of tests/train_step_common.py and asserts on every rank - bits,
counts, file names, and in `fixture` the reference's float64 errors within the fixture's own resolution (the tool's docstring has
the modes).  Nothing here provokes a fault: the poison is a NaN VALUE in a gradient."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("world,mode", [(2, "same"), (2, "fixture"), (3, "odd"), (2, "poison"), (2, "app"), (2, "launch")])
def test_train_group(world, mode):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_train_dist_check.py"), str(world), mode], capture_output=True,
                       text=True, timeout=300)
    print(r.stdout[-4000:])
    print(r.stderr[-6000:])
    assert r.returncode == 0, (world, mode)
    assert "ok: %s" % mode in r.stdout
