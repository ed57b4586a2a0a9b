"""dist.reconstruction_sharded for a SurfaceClassifier shape other than the released one (s1): 2 and 3 processes (ragged slabs) on one
GPU against the single-process reconstruction - meshes bit-identical, both precisions, one-piece and streamed per-slab extraction,
want_normals False and True (tools/gpu_slab_check_shapes.py; gloo with host staging)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("world,R", [(2, 40), (3, 50)])
def test_sharded_reconstruction_of_another_shape_equals_single_process(world, R):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_slab_check_shapes.py"), str(world), str(R)], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("slab == one piece") == 6 and "MISMATCH" not in r.stdout, r.stdout
