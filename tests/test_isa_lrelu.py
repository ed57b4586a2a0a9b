"""The column kernels' LeakyReLU is ONE maximum per value, held in the SHIPPED ISA (CPU only, tests/isa.py).

In front of fmaxf hipcc canonicalises every operand it cannot prove free of signalling NaNs - `v_max_f32 vA, vB, vB` - and every
MFMA accumulator is such an operand: kernel v12 carried 912 of them per tile (14.5 % of its vector instructions), each an identity
in the kernels' float mode (ieee_mode 1, f32 denormals on; an MFMA produces no signalling NaN).  lrelu_max in surs_query.hip takes
them out.  What remains is the per-tile glue (the p range and z range reductions): at most 16 per kernel."""
import os
import re

import pytest

import isa

pytestmark = pytest.mark.skipif(not isa.available(), reason="llvm-objdump / llvm-readelf of /opt/rocm/lib/llvm or the built library missing")

CAP = 16
KERNELS = [r"grid_mlp_kernel_v12<1>", r"grid_mlp_kernel_v12<2>", r"grid_mlp_kernel_v10<1>", r"grid_mlp_kernel_v10<2>", r"grid_mlp_kernel_v11\b",
           r"grid_mlp_kernel_v3<1>", r"grid_mlp_kernel_v3<2>", r"grid_mlp_kernel_v5\b"]
_same = re.compile(r"^v_max_f32\w*\s+\w+,\s*(\w+),\s*(\w+)\s*$")


def canonicalisations(ins):
    """The v_max_f32 of `ins` (disassembly lines) whose two sources are the same register."""
    out = []
    for i in ins:
        m = _same.match(i)
        if m and m.group(1) == m.group(2) and m.group(1)[0] in "va":
            out.append(i)
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    so = os.environ.get("SURS_ISA_SO", isa.SO)
    out = {}
    for co in isa.code_objects(so, str(tmp_path_factory.mktemp("isa_lrelu"))):
        md, dis = isa.kernel_metadata(co), isa.disassembly(co)
        names = isa.demangle(list(md))
        for k in md:
            out[names[k]] = dis[k]
    return out


def test_the_counter_sees_what_it_counts():
    ins = ["v_max_f32_e32 v3, v3, v3", "v_max_f32_e32 v3, v4, v5", "v_max_f32_e64 v1, v200, v200", "v_max_f32_e32 v0, 0, v0",
           "v_max_f32_e32 v0, s4, s4", "v_mul_f32_e32 v4, v4, v4"]
    assert canonicalisations(ins) == ["v_max_f32_e32 v3, v3, v3", "v_max_f32_e64 v1, v200, v200"]


@pytest.mark.parametrize("pat", KERNELS)
def test_no_canonicalising_max_on_accumulator_values(kernels, pat):
    sel = {n: ins for n, ins in kernels.items() if re.search(pat, n)}
    assert len(sel) == 1, "expected one kernel for %s, found %s" % (pat, sorted(sel))
    (name, ins), = sel.items()
    assert len(ins) > 3000, "%s: %d instructions - not the column kernel's body" % (name[:60], len(ins))
    n = len(canonicalisations(ins))
    print("%s: %d v_max_f32 with equal sources" % (name[:60], n))
    assert n <= CAP, "%s: %d canonicalising v_max_f32 (cap %d): fmaxf on an MFMA result is back (lrelu_max, surs_query.hip)" % (name[:60], n, CAP)
