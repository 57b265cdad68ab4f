"""The exact re-rank's whole-row gather (csrc/exact_gather.h, k_rerank_lds) on the hardware; run by tests/test_exact_gather_gpu.py in
a child process with RCN_LIB=tools/librcn_diag.so and the diagnostic switches of the case in the environment (RCN_FILTER_PASS,
RCN_RERANK_PASS, RCN_CHUNK_ROWS: read when a context is created).

  exact_gather_check.py <set>   one grid (all ordered pairs in both orientations and the self pairs, unless the set says otherwise)
                                against the oracle, twice; prints one JSON line with the statistics and the row counts the test asserts.
  sets: edges256, edges128, edges36, edges200   images of 1, 63, 64, 65, 193, 2, 3 and 130 rows of that many elements: the survivor
                                counts per pair and in total fall on, just under and just over multiples of a tile and of 64, a tile
                                of survivors spans pairs with different images, a 2-row train image never certifies, a 3-row one is
                                the smallest that does, and a 1-row train image sends nothing
        ragged                  the set of tools/mid_i8_check.py: exact duplicates and 1e-4 near-duplicates among the train rows
        empty                   the pairs (i, 0) of edges256 only: image 0 has one row, no row reaches the re-rank"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EDGE_ROWS = [1, 63, 64, 65, 193, 2, 3, 130]


def edge_set(D):
    """unit rows drawn from a common pool of 260, six in ten with 10 % noise and the rest as they are: pairs have true matches, exact
    copies and rows without a counterpart"""
    rng = np.random.default_rng(100 + D)
    pool = rng.standard_normal((260, D)).astype(np.float32)
    ims = []
    for k in EDGE_ROWS:
        pick = rng.choice(len(pool), k, replace=False)
        x = (pool[pick] + rng.standard_normal((k, D)) * 0.1 * (rng.random((k, 1)) < 0.6)).astype(np.float32)
        ims.append(x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32))
    return ims


def grid(name):
    from reconstructor_amd.matcher import all_pairs
    if name == "ragged":
        import mid_i8_check
        ims = mid_i8_check.data_set("ragged")
    else:
        ims = edge_set(256 if name == "empty" else int(name[len("edges"):]))
    n = len(ims)
    if name == "empty":
        return ims, np.array([[i, 0] for i in range(n)], np.int32)
    ap = all_pairs(n)
    return ims, np.concatenate([ap, ap[:, ::-1], np.array([[i, i] for i in range(n)], np.int32)]).astype(np.int32)


def main(name):
    import torch  # noqa: F401
    from oracle import orc
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    assert b"DIAGNOSTIC" in _lib.load().rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    ims, pairs = grid(name)
    exp, ec = orc.match_grid(ims, pairs, threads=8)
    K = [len(im) for im in ims]
    res = {"rows_train_ge2": int(sum(K[q] for q, t in pairs if K[t] >= 2)), "matches": int(ec.sum()), "all_minus_one": bool((exp == -1).all())}
    m = HipL2Matcher(device=0)                # (the switches are read here)
    for i, im in enumerate(ims):
        m.upload(i, im)
    for rep in range(2):
        out, cnt = m.match_grid(pairs, exp.shape[1])
        assert np.array_equal(out, exp) and np.array_equal(cnt, ec), (name, rep, "differs from the oracle", np.argwhere(out != exp)[:5].tolist())
    st = m.stats()
    res.update({k: int(st[k]) for k in ("rows_total", "rows_reranked", "rows_exact_fallback", "rows_brute_force", "chunks", "coarse_dtype")})
    m.ctx.close()
    print(json.dumps(res))
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1])
