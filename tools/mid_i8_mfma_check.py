"""The middle tier's int8 sweep on MFMA (csrc/mid_i8.h, k_mid_eval_i8) against its dot4 form (k_mid_eval_i8_dot4, RCN_MID_I8_MFMA=0) and
the oracle; run by tests/test_mid_i8_mfma_gpu.py in a child process with RCN_LIB=tools/librcn_diag.so and the diagnostic switches of the
case in the environment (RCN_RERANK_PASS, RCN_FILTER_PASS: read when a context is created).

  python tools/mid_i8_mfma_check.py <set>
      ragged   six 256-d images of 2, 17, 130, 512, 513 and 1100 rows, every ordered pair and the self pairs: train tiles of one 16-row
               block, of one wave's share, of exactly one tile, of a tile and one row, of three tiles with padded rows.  Image 5 holds a
               row forty times over that is the second neighbour of two planted query rows (whose ratio test is undecided in int8): forty-one
               equal accumulators under the threshold, more than a candidate list holds.  Two query rows carry a NaN: no integer threshold.
      bins     images of 1, 16, 17, 33, 130 and 513 rows chained 0 -> 1 -> 2 -> 3 -> 4: with every row sent to the tier the bins of the
               train images hold exactly 1, 16, 17 and 33 rows, the bins of images 0 and 5 are empty; one row of the 33 carries a NaN.
  Both arms must give the oracle's tables and must have launched their own kernel (rcn_diag_mid_sweep); through rcn_diag_mid, ccount must
  agree row for row between the arms and the candidate lists must be the same sets wherever they did not overflow.  The MFMA arm's lists are
  also checked against numpy on the device's own integers (rcn_diag_i8: the int8 rows and half-norms both kernels read): ccount is the
  size of {t : hn[t] - qq.tq <= thr_acc} and the list is that set; "on_threshold" counts the rows with an accumulator EQUAL to their
  threshold, which a < written for <= would lose.  Prints one JSON line, then OK."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIDCAP = 32
KS = {"ragged": [2, 17, 130, 512, 513, 1100], "bins": [1, 16, 17, 33, 130, 513]}


def data_set(name):
    from reconstructor_amd import synth
    rng = np.random.default_rng(11)
    ims = synth.descriptor_set("superpoint", 6, KS[name], n_world=1400, seed=41)
    if name == "ragged":
        def unit():
            v = rng.standard_normal(256)
            return (v / np.linalg.norm(v)).astype(np.float32)
        # two query rows of image 4 whose nearest rows in image 5 stand at the ratio test's boundary, read on distances (0.7) and
        # on squared distances (sqrt 0.7): the int8 coarse pass cannot decide either, both go to the re-rank and from there to the tier
        for q, t0, t1, rel in ((5, 10, 20, 0.7), (6, 11, 21, float(np.sqrt(0.7)))):
            ims[5][t1] = ims[4][q] + 0.3 * unit()
            ims[5][t0] = ims[4][q] + 0.3 * rel * (1.0 + 1e-4) * unit()
        ims[5][200:240] = ims[5][20]                 # forty exact duplicates of the second neighbour of query row 5
        ims[5][300:340] = ims[5][21]
        ims[4][7, 3] = np.nan                        # rows the coarse pass cannot place: no integer threshold (k_mid_eval's rows)
        ims[3][9, 200] = np.nan
        n = len(ims)
        i, j = np.triu_indices(n, 1)
        ap = np.stack([i, j], 1)
        pairs = np.concatenate([ap, ap[:, ::-1], np.array([[k, k] for k in range(n)])]).astype(np.int32)
    else:
        ims[3][4, 17] = np.nan
        pairs = np.array([[0, 1], [1, 2], [2, 3], [3, 4]], np.int32)
    return ims, pairs


def dump_mid(lib, m):
    n = C.c_int64(0)
    m.ctx.check(lib.rcn_diag_mid(m.ctx.h, C.byref(n), None, None, None, None, 0))
    n = int(n.value)
    ent, tacc, cc, cl = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, MIDCAP), np.int32)
    if n:
        nn = C.c_int64(0)
        m.ctx.check(lib.rcn_diag_mid(m.ctx.h, C.byref(nn), ent.ctypes.data, tacc.ctypes.data, cc.ctypes.data, cl.ctypes.data, n))
    o = np.argsort(ent, kind="stable")               # binned order depends on the scatter's atomics: compare by entry
    assert len(set(ent.tolist())) == n
    return ent[o], tacc[o], cc[o], cl[o]


def main(name):
    import torch  # noqa: F401
    from oracle import orc
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    lib = _lib.load()
    assert b"DIAGNOSTIC" in lib.rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    lib.rcn_diag_mid.restype = C.c_int
    lib.rcn_diag_mid.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.rcn_diag_mid_sweep.restype = C.c_int
    lib.rcn_diag_mid_sweep.argtypes = [C.c_void_p]
    lib.rcn_diag_i8.restype = C.c_int
    lib.rcn_diag_i8.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    ims, pairs = data_set(name)
    stride = (max(KS[name]) + 4) // 4 * 4           # rows of whole 16-byte groups with a tail: the table passes take their four-entry form
    exp, ec = orc.match_grid(ims, pairs, threads=8)
    exp = np.pad(exp, ((0, 0), (0, stride - exp.shape[1])), constant_values=-1)
    arms = {}
    for arm in ("mfma", "dot4"):
        if arm == "dot4":
            os.environ["RCN_MID_I8_MFMA"] = "0"
        m = HipL2Matcher(device=0)                   # (the switches are read here)
        for i, im in enumerate(ims):
            m.upload(i, im)
        out, cnt = m.match_grid(pairs, stride)
        assert np.array_equal(out, exp) and np.array_equal(cnt, ec), (name, arm, "differs from the oracle", np.argwhere(out != exp)[:5].tolist())
        st = m.stats()
        assert st["coarse_dtype"] == 2 and st["chunks"] == 1, st
        assert lib.rcn_diag_mid_sweep(m.ctx.h) == {"mfma": 1, "dot4": 2}[arm], (arm, "ran the other form of the sweep")
        if arm == "mfma":                            # the integers both kernels read
            dev, model = [], (C.c_double * 8)()
            for i, im in enumerate(ims):
                xq, hn, nn = np.zeros((len(im), 256), np.int8), np.zeros(len(im), np.int32), np.zeros((len(im), 2), np.float32)
                m.ctx.check(lib.rcn_diag_i8(m.ctx.h, model, i, xq.ctypes.data, hn.ctypes.data, nn.ctypes.data))
                dev.append((xq.astype(np.int64), hn.astype(np.int64)))
        arms[arm] = dump_mid(lib, m) + ({k: int(st[k]) for k in ("rows_total", "rows_reranked", "rows_exact_fallback", "rows_brute_force")},)
        m.ctx.close()
    (ea, ta, ca, la, sa), (eb, tb, cb, lb, sb) = arms["mfma"], arms["dot4"]
    assert sa == sb, (sa, sb)
    assert np.array_equal(ea, eb) and np.array_equal(ta, tb), "the two arms sent different rows to the tier"
    own = ta != 0
    assert np.array_equal(ca[own], cb[own]), ("ccount differs between the MFMA and the dot4 sweep", np.nonzero(own & (ca != cb))[0][:5].tolist())
    assert (ca[own] >= 2).all()
    for r in np.nonzero(own & (ca <= MIDCAP))[0]:
        assert np.array_equal(np.sort(la[r, :ca[r]]), np.sort(lb[r, :cb[r]])), (int(r), "candidate sets differ")
    for r in np.nonzero(own & (ca > MIDCAP))[0]:
        assert len(set(la[r].tolist())) == MIDCAP
    pr = pairs[(ea >> np.uint64(32)).astype(np.int64)]
    qrow = (ea & np.uint64(0xFFFFFFFF)).astype(np.int64)
    on_thr = 0
    for r in np.nonzero(own)[0]:
        (xq, _), (xt, hn) = dev[pr[r, 0]], dev[pr[r, 1]]
        acc = hn - xt @ xq[qrow[r]]
        want = np.nonzero(acc <= int(ta[r]))[0]
        assert ca[r] == want.size, (int(r), "ccount is not the number of rows under the threshold", int(ca[r]), int(want.size))
        if ca[r] <= MIDCAP:
            assert np.array_equal(np.sort(la[r, :ca[r]]), want), (int(r), "the emitted rows are not the rows under the threshold")
        else:
            assert np.isin(la[r], want).all()
        on_thr += int((acc == int(ta[r])).any())
    train = pr[:, 1]
    bins = np.bincount(train, minlength=len(ims))
    mixed = sorted(int(t) for t in set(train[~own].tolist()) & set(train[own].tolist()))
    res = {"rows": int(len(ea)), "own": int(own.sum()), "over": int((own & (ca > MIDCAP)).sum()), "longest": int(ca[own].max()) if own.any() else 0,
           "on_threshold": on_thr, "bins": bins.tolist(), "bins_with_both_kinds": mixed, "stats": sa}
    print(json.dumps(res))
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1])
