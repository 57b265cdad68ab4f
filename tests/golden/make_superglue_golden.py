"""Writes tests/golden/superglue_small.npz: fp32 scores and the float64 results of tests/sg_ref.py for the small shared cases
(the larger ones are regenerated from their seeds by the tests)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sg_ref  # noqa: E402

out = {"shapes": np.array([(1, 1), (1, 5), (7, 3), (33, 47), (64, 64)], np.int32)}
for m, n in out["shapes"]:
    d0, d1, target = sg_ref.planted_case(int(m), int(n), sg_ref.case_seed(int(m), int(n)))
    S = sg_ref.scores(d0, d1).astype(np.float32)
    logP, u, v = sg_ref.assign(S)
    sel = sg_ref.select(logP)
    k = "_%d_%d" % (m, n)
    out["S" + k], out["logP" + k], out["target" + k] = S, logP, target.astype(np.int32)
    out["table" + k], out["mscores0" + k] = sel["table"].astype(np.int32), sel["mscores0"]
np.savez_compressed(os.path.join(HERE, "superglue_small.npz"), **out)
