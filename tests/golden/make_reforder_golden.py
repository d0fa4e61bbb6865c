"""Stores the reference build's dendrograms (oracle/_ref: the reference's own FastClusterWrapper C++, built by oracle/Makefile) of every
input of tests/test_ahc_reforder_emul.py in tests/golden/ahc_reforder_golden.npz, with the SHA-256 of each input, so that the CPU
emulations of the reference-order selection are checked where the reference build cannot be made.
    python tests/golden/make_reforder_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
from test_ahc_reforder_emul import GOLDEN, stored_inputs  # noqa: E402


def main():
    oracle.build()
    assert oracle.ref_available(), "oracle/_ref is not built (needs the reference sources)"
    out = {}
    for key, x in stored_inputs():
        st, z = oracle.linkage_ref(x)
        assert st == 0, (key, st)
        out[key] = z
        out[key + "_sha256"] = np.array(hashlib.sha256(x.tobytes()).hexdigest())
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, len(out) // 2, "dendrograms")


if __name__ == "__main__":
    main()
