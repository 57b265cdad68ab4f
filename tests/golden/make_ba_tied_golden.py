"""Writes tests/golden/ba_tied_judge.npz: the judge of tests/ba_tied_ref.py on the cases of the GPU suite (tests/test_ba_tied_gpu.py),
so that the GPU run needs no scipy and spends no minutes of CPU.  Per case: the minimum by trust-region reflective (P, I, X, rms), what
dogbox differs from it by (spread: rms, poses, intrinsics, points), and the first LM step in long double (dP, dI, dX, rounded to float64)
with the error of the same step in float64 (eP, eI, eX).  tests/test_ba_tied_ref.py holds the record against a fresh run of the judge.

    PYTHONPATH=. python tests/golden/make_ba_tied_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ba_tied_ref as T  # noqa: E402


def record(name):
    sc, _ = T.case(name)
    Pa, Ia, Xa, ra = T.judged(name, "trf")
    Pb, Ib, Xb, rb = T.judged(name, "dogbox")
    seen = np.zeros(len(Xa), bool)
    seen[sc["obs_pt"]] = True
    out = {"P": Pa, "I": Ia, "X": Xa, "rms": np.float64(ra),
           "spread": np.array([abs(ra - rb), np.abs(Pa - Pb).max(), np.abs(Ia - Ib).max(), np.abs(Xa - Xb)[seen].max()])}
    ld, f64 = T.stepped(name, T.LD), T.stepped(name, np.float64)
    for k in ("P", "I", "X"):
        out["d" + k] = np.asarray(ld["d" + k], np.float64)
        out["e" + k] = np.asarray(np.abs(np.asarray(f64["d" + k], T.LD) - ld["d" + k]), np.float64)
    out["I0"] = np.asarray(ld["intr0"], np.float64)      # the intrinsics the step starts from: the scene's, projected onto the focal bound
    return {name + "." + k: v for k, v in out.items()}


if __name__ == "__main__":
    names = sys.argv[1:] or list(T.CASES)
    out = {}
    if sys.argv[1:] and os.path.exists(T.GOLDEN):
        with np.load(T.GOLDEN) as z:
            out = {k: z[k] for k in z.files}
    for name in names:
        out.update(record(name))
        print(name, "rms %.6f" % out[name + ".rms"], "spread", out[name + ".spread"], flush=True)
    np.savez(T.GOLDEN, **out)
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")
