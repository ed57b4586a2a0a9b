"""tests/golden/column_bits_r296.npz: the volumes of every column kernel on the grid of tests/column_bits.py, as uint32 words, from
the library this process loads.  The fixture records what the kernels computed BEFORE a change that must keep their bits, so run it
on a GPU with SURS_LIB_PATH pointing at a build of the parent commit:

    SURS_LIB_PATH=<parent build of libsurs_hip.so> python tools/gen_golden_column_bits.py [out.npz]

The archive is written with fixed member times and order: two runs give identical files (compare them before trusting one)."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import column_bits as cb  # noqa: E402
from surs_amd import _lib  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", cb.FIXTURE)
    c = cb.Context()
    print("library:", _lib.LIB_PATH)
    for gain in cb.GAINS:
        print("gain %d: listed per 128-voxel tile lr %.1f, hr bound %.1f" % ((gain,) + c.listed(gain)))
    arrays = {}
    for gain, prec, kv in cb.CASES:
        a = c.bits(gain, prec, kv)
        f = a.view(np.float32)
        assert np.isfinite(f).all()
        arrays[cb.key(gain, prec, kv)] = a
        print("%-14s %d distinct words, range [%.4f, %.4f]" % (cb.key(gain, prec, kv), len(np.unique(a)), f.min(), f.max()))
    for prec in ("bf16", "fp16"):
        for gain in cb.GAINS:
            print("gain %d %s: kernel 12 == kernel 10: %s" % (gain, prec, np.array_equal(arrays[cb.key(gain, prec, 12)], arrays[cb.key(gain, prec, 10)])))
    with zipfile.ZipFile(out, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
