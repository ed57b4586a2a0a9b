"""CPU checks of the multi-view evaluator for classifier shapes other than the released one (surs_mlp_fused_views.inc): the C ABI
is declared and exported, the shipped code object holds its six instantiations within the register budget and without scratch, the
plan covers every shape of the test matrix, and its limits are refused with the same message from Python and from C."""
import ctypes as C
import os
import re

import pytest

from surs_amd import _lib, native

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SURS_E_INVALID = -1
NEW = ("surs_query_points_generic_views", "surs_query_grid_generic_views", "surs_mlp_generic_views_info")

# (the shapes of tools/gen_golden_shapes.py: ((dims_lr, res_lr), (dims_hr, res_hr)))
S1 = (((321, 512, 256, 128, 1), (1, 2, 3)), ((322, 512, 256, 128, 1), (1, 2, 3)))
MATRIX = {
    "s1": S1,
    "nores": (((321, 1024, 512, 256, 128, 1), ()), ((322, 1024, 512, 256, 128, 1), ())),
    "deep": (((321, 1024, 1024, 512, 256, 128, 1), (2, 3, 4, 5)), ((322, 1024, 1024, 512, 256, 128, 1), (2, 3, 4, 5))),
    "odd": (((321, 1000, 500, 250, 100, 1), ()), ((322, 1000, 500, 250, 100, 1), ())),
    "res0": (((321, 1024, 512, 256, 128, 1), (0, 2)), ((322, 1024, 512, 256, 128, 1), (0, 2))),
    "l1": (((321, 1), ()), ((322, 1), ())),
    "l2": (((321, 64, 1), (1,)), ((322, 64, 1), (1,))),
    "mixed": (S1[0], ((322, 1000, 500, 250, 100, 1), ())),
    "released": native.DEFAULT_MLP_SHAPES,
}


def test_new_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "surs.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None


def test_views_kernels_use_no_scratch(tmp_path):
    """The six mlp_fused_views_kernel<NP, PB> instantiations: no scratch, at most 256 VGPR + AGPR per lane (eight waves per
    workgroup), LDS dynamic (surs_mlp_generic_views_info)."""
    import isa
    meta = {}
    for co in isa.code_objects(workdir=str(tmp_path)):
        meta.update(isa.kernel_metadata(co))
    views = {k: v for k, v in meta.items() if "mlp_fused_views_kernel" in k}
    assert len(views) == 6, sorted(views)
    for name, m in views.items():
        assert m[".private_segment_fixed_size"] == 0, name
        assert m[".vgpr_count"] + m.get(".agpr_count", 0) <= 256, name
        assert m[".group_segment_fixed_size"] == 0, name


@pytest.mark.parametrize("name", list(MATRIX))
@pytest.mark.parametrize("V", [1, 2, 4, 64])
def test_plan_for_every_shape(name, V):
    tp, lds = native.mlp_generic_views_info(MATRIX[name], V)
    assert tp in (16, 32) and 0 < lds <= 160 * 1024
    tp1, lds1, _ = native.mlp_generic_info(MATRIX[name])
    assert tp == tp1 and lds > lds1   # (the same tile as the single-view kernel for every shape of the matrix; + the feature sum)
    widest = max([32] + [-(-d // 32) * 32 for dims, _ in MATRIX[name] for d in dims[1:-1]])
    assert lds == tp * ((widest + 4 + 2 * 356) * 4 + 24)   # features, their view sum, activations [P][row]; 24 bytes per point


def _c_views_info(shapes, V):
    lr, hr = (native._shape_struct(*s) for s in shapes)
    tp, lds = C.c_int(0), C.c_int(0)
    rc = _lib.lib().surs_mlp_generic_views_info(C.byref(lr), C.byref(hr), V, C.byref(tp), C.byref(lds))
    return rc, _lib.lib().surs_last_error().decode()


@pytest.mark.parametrize("V", [0, -1, 65, 1000])
def test_view_count_limit(V):
    rc, msg = _c_views_info(S1, V)
    assert rc == SURS_E_INVALID
    assert "num_views must be in [1, 64]" in msg
    with pytest.raises(ValueError) as e:
        native.mlp_generic_views_info(S1, V)
    assert str(e.value) == msg


@pytest.mark.parametrize("width,ok", [(1824, True), (1825, False), (2048, False)])
def test_width_limit_of_the_lds_plan(width, ok):
    """The multi-view tile keeps the features AND their running view sum in LDS: the widest padded hidden layer a 16-point tile
    holds is 1824 (the single-view evaluator takes 2048)."""
    shapes = (((321, width, 1), ()), ((322, 64, 1), ()))
    native.mlp_generic_info(shapes)   # (the single-view evaluator takes it)
    rc, msg = _c_views_info(shapes, 2)
    if ok:
        assert rc == 0 and native.mlp_generic_views_info(shapes, 2)[0] == 16
        return
    assert rc == SURS_E_INVALID and "hidden widths must be at most 1824" in msg
    with pytest.raises(ValueError) as e:
        native.mlp_generic_views_info(shapes, 2)
    assert str(e.value) == msg


def test_shape_limits_still_named():
    rc, msg = _c_views_info((((321, 4096, 1), ()), ((322, 64, 1), ())), 2)
    assert rc == SURS_E_INVALID and "hidden widths must be between 1 and 2048" in msg
