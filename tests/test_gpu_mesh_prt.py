"""GPU checks of the PRT kernels (csrc/surs_mesh_prt.hip): held to surs_mesh_prt_host BIT FOR BIT - the same header looped on the host,
which tests/test_mesh_prt_host.py holds to the float64 model tests/prt_ref.py - on the occlusion scenes, a convex mesh, a face count
that crosses the LDS chunk several times and ends inside one, a vertex count that is no multiple of a workgroup's vertices and a
direction count that is no multiple of 32.  The same bits must come back from a second call with a workspace at another address."""
import numpy as np
import pytest
import torch

import mesh_ref as mr
import prt_ref as pr

pytestmark = pytest.mark.gpu


def _chunk_torus():
    from surs_amd import _lib
    chunk = _lib.MESH_PRT_CHUNK
    nu = (10 * chunk + chunk // 2) // 80 + 1            # 2 nu 40 faces: more than ten chunks, the last one partly filled
    v, f = mr.torus(nu, 40)
    assert len(f) > 10 * chunk and len(f) % chunk not in (0, chunk - 1)
    return v, f, pr.unit_normals(v, f)


# name -> (scene, n of the n x n directions, seed, offset)
CASES = {
    "floor_roof": (pr.floor_roof, 8, 3, 1e-3),
    "torus": (pr.torus_scene, 8, 3, 0.5),
    "icosphere320": (lambda: pr.icosphere(2), 8, 0, 0.05),
    "chunks": (_chunk_torus, 4, 1, 0.5),
    "ragged": (pr.torus_scene, 5, 2, 0.5),              # 288 vertices x 25 directions: 10.24 vertices a workgroup, D % 32 = 25
}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_is_the_host_loop_bit_for_bit(name):
    from surs_amd import _lib, native, render
    make, n, seed, offset = CASES[name]
    v, f, normals = make()
    dirs = render.prt_directions(n, seed)
    want = native.mesh_prt_host(v, f, normals, dirs, offset)
    mesh = native.Mesh(v, f)
    got = native.mesh_prt(mesh, normals, dirs, offset)
    assert got.shape == (len(v), 9) and got.dtype == torch.float32
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    if name in ("torus", "floor_roof"):
        assert np.abs(want).max() > 0.5 and len(np.unique(_bits(want[:, 0]))) > 3       # not a trivial answer
    # again, with a workspace of its own at another address, full of ones: the bits are only a transport
    need = _lib.lib().surs_mesh_prt_workspace_bytes(len(v), len(dirs))
    buf = torch.full((need + 512,), 255, dtype=torch.uint8, device=mesh.verts.device)
    again = native.mesh_prt(mesh, normals, dirs, offset, workspace=buf[256:256 + need])
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(want))
    assert bool((buf[:256] == 255).all()) and bool((buf[256 + need:] == 255).all())      # and nothing written outside it


def test_counted_variant_gives_the_same_bits_and_a_plausible_count():
    """surs_mesh_prt_counted (the timing tool's): the bits of surs_mesh_prt, and a number of executed tests between what the rays
    that find nothing must look at (every face) and all pairs."""
    from surs_amd import native, render
    v, f, normals = pr.torus_scene()
    dirs = render.prt_directions(8, 3)
    mesh = native.Mesh(v, f)
    want, vis = native.mesh_prt_host(v, f, normals, dirs, 0.5, want_visible=True)
    got, tests = native.mesh_prt(mesh, normals, dirs, 0.5, want_tests=True)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert int(vis.sum()) * len(f) <= tests <= vis.size * len(f)


def test_short_workspace_is_refused():
    from surs_amd import _lib, native, render
    v, f, normals = pr.floor_roof()
    mesh = native.Mesh(v, f)
    with pytest.raises(_lib.SursError):
        native.mesh_prt(mesh, normals, render.prt_directions(8, 0), 1e-3, workspace=torch.empty(4, dtype=torch.uint8, device=mesh.verts.device))
