"""Writes tests/golden/hamming_small.npz: the inputs, the knn2 table and the match table of every case of tests/hamming_ref.py
(shape_cases, planted_cases).  tests/test_hamming_ref.py regenerates the arrays and compares them with the file.

    python tests/golden/make_hamming_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hamming_ref  # noqa: E402

PATH = os.path.join(HERE, "hamming_small.npz")


def arrays():
    out = {}
    cases = dict(hamming_ref.shape_cases())
    cases.update(hamming_ref.planted_cases())
    for name, (q, t) in cases.items():
        out[name + ".q"], out[name + ".t"] = q, t
        out[name + ".knn2"] = hamming_ref.knn2(q, t)
        out[name + ".match"] = hamming_ref.match_pair(q, t)[0]
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **arrays())
    print(PATH, os.path.getsize(PATH), "bytes")
