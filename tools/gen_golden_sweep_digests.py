"""tests/golden/sweep_digests.json: the SHA-256 digests of what the cases of tests/sweep_digests.py return from the library this
process loads, and the probe's two floats as bits.  The fixture records what the sweeps computed BEFORE a change that must keep
their bits, so run it on a GPU with SURS_LIB_PATH pointing at a build of the parent commit:

    SURS_LIB_PATH=<parent build of libsurs_hip.so> python tools/gen_golden_sweep_digests.py [out.json]

No digest is written for an output that holds a non-finite value or fewer than 64 distinct words, nor for a point-run call that the
library answered with 0 columns: a constant field would "match" whatever the sweep did."""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sweep_digests as sd  # noqa: E402
from surs_amd import _lib  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", sd.FIXTURE)
    c = sd.Context()
    print("library:", _lib.LIB_PATH)
    digests = {}
    for name, words in c.outputs():
        if words is None:
            sys.exit("%s: the library reported 0 columns" % name)
        if not sd.is_a_field(words):
            sys.exit("%s: non-finite values or fewer than %d distinct words - not recorded" % (name, sd.MIN_DISTINCT))
        f = words.view(np.float32)
        digests[name] = sd.digest(words)
        print("%-16s %9d words, %7d distinct, range [%.4f, %.4f]  %s" % (name, words.size, len(np.unique(words)), f.min(), f.max(),
                                                                        digests[name][:16]))
    assert list(digests) == sd.DIGEST_CASES
    probe = {}
    for name, gain in sd.PROBE:
        bits = c.probe(gain)
        f = bits.view(np.float32)
        if not (np.isfinite(f).all() and (f > 0).all()):
            sys.exit("%s: the probe did not run or counted nothing" % name)
        probe[name] = ["%08x" % int(b) for b in bits]
        print("%-16s listed lr %.3f, hr bound %.3f" % (name, f[0], f[1]))
    with open(out, "w") as fh:
        json.dump({"sha256": digests, "probe_bits": probe}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
