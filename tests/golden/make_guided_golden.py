"""Writes tests/golden/guided_small.npz: the inputs, the band, the knn2 tables and the match tables (one-way and cross-checked) of a
few cases of tests/guided_ref.py.  tests/test_guided_ref.py regenerates the arrays and compares them with the file;
tests/test_guided_band.py evaluates csrc/guided_band.h on the file's coordinates.

    python tests/golden/make_guided_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import guided_ref  # noqa: E402

PATH = os.path.join(HERE, "guided_small.npz")


def cases():
    return {
        "two_view_65_63": guided_ref.shape_case(65, 63, 40, seed=31),
        "two_view_120_90": guided_ref.shape_case(120, 90, 32, seed=32),
        "planted_counts": guided_ref.planted_counts_case(32),
        "all_in_band": guided_ref.all_in_band_case(5, 70, 32),
    }


def arrays():
    out = {}
    for name, (q, xy1, t, xy2, F) in cases().items():
        m = guided_ref.band(F, xy1, xy2, 3.0)
        idx, d2 = guided_ref.knn2(q, t, m)
        out[name + ".q"], out[name + ".xy1"], out[name + ".t"], out[name + ".xy2"], out[name + ".F"] = q, xy1, t, xy2, F
        out[name + ".band"] = np.packbits(m, axis=1) if m.size else np.zeros((len(xy1), 0), np.uint8)
        out[name + ".idx"], out[name + ".d2"] = idx, d2
        out[name + ".match"] = guided_ref.match_pair(q, xy1, t, xy2, F)[0]
        out[name + ".cross"] = guided_ref.match_pair(q, xy1, t, xy2, F, cross_check=1)[0]
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **arrays())
    print(PATH, os.path.getsize(PATH), "bytes")
