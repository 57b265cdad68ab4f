"""The middle tier's int8 sweep (csrc/mid_i8.h) on the hardware; run by tests/test_mid_i8_gpu.py in a child process with
RCN_LIB=tools/librcn_diag.so and the diagnostic switches of the case in the environment (RCN_RERANK_PASS, RCN_FILTER_PASS,
RCN_CHUNK_ROWS, RCN_MID_ROWS: read when a context is created).

  grid <set>   a small ragged grid (both orientations and self pairs) against the oracle, twice: with the int8 sweep and with
               RCN_MID_I8=0 (every row through the fp32 sweep, the behaviour before the int8 sweep existed).  Both tables must equal
               the oracle's, hence each other.  Prints one JSON line with the statistics of both runs.
               sets: ragged (256-d, 7 images), d200 (200-d rows: the tail chunks of the padded int8 rows are zero), mixed (a train
               image whose bin holds rows with and without an integer threshold: exact ties and a query row with a NaN element)
  lists        one 1024 x 1024 pair: the lists the sweep left (rcn_diag_mid) against the numpy model of tests/int8_emu.py -- for every row
               with an integer threshold, at least two rows, both K1 candidates among them, and exactly the set {t : acc <= thr_acc}."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIDCAP = 32


def plant_ties(ims, rng):
    for im in ims:                               # exact ties and near-ties for the top-2
        if len(im) >= 8:
            a, b, c, d = rng.integers(0, len(im), 4)
            im[a] = im[b]
            im[c] = im[d] + (rng.standard_normal(im.shape[1]) * 1e-4).astype(np.float32)


def data_set(name):
    from reconstructor_amd import synth
    rng = np.random.default_rng(3)
    if name == "ragged":
        ims = synth.descriptor_set("superpoint", 7, [700, 300, 1024, 64, 513, 2, 900], n_world=1500, seed=23)
        plant_ties(ims, rng)
        # forty 1e-4 near-ties of one train row: more rows under a threshold than a candidate list holds (RCN_MIDCAP = 32), so the
        # rows that meet them overflow to the brute-force kernel
        ims[2][100:140] = ims[2][50] + (rng.standard_normal((40, 256)) * 1e-4).astype(np.float32)
    elif name == "d200":
        ims = []
        for k in (300, 150, 513, 40):
            x = rng.standard_normal((k, 200)).astype(np.float32)
            ims.append(x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32))
        ims[1][:100] = ims[0][:100] + (rng.standard_normal((100, 200)) * 0.02).astype(np.float32)      # true matches
        ims[2][:120] = ims[0][100:220] + (rng.standard_normal((120, 200)) * 0.02).astype(np.float32)
        plant_ties(ims, rng)
    elif name == "mixed":
        ims = synth.descriptor_set("superpoint", 3, [600, 500, 300], n_world=900, seed=31)
        ims[1][20] = ims[1][10]                                                          # a duplicated train row ...
        ims[0][5] = ims[1][10] + (rng.standard_normal(256) * 1e-3).astype(np.float32)    # ... and queries whose two nearest neighbours tie
        ims[2][9] = ims[1][10]
        ims[0][7, 3] = np.nan                                                            # a query row the coarse pass cannot place: no integer threshold
        ims[2][11, 200] = np.nan
    else:
        raise ValueError(name)
    return ims


def check_grid(name):
    import torch  # noqa: F401
    from oracle import orc
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    assert b"DIAGNOSTIC" in _lib.load().rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    ims = data_set(name)
    n = len(ims)
    ap = all_pairs(n)
    pairs = np.concatenate([ap, ap[:, ::-1], np.array([[i, i] for i in range(n)], np.int32)]).astype(np.int32)
    exp, ec = orc.match_grid(ims, pairs, threads=8)
    K = [len(im) for im in ims]
    res = {"rows_train_ge3": int(sum(K[q] for q, t in pairs if K[t] >= 3)), "rows_train_ge2": int(sum(K[q] for q, t in pairs if K[t] >= 2))}
    for arm in ("i8", "f32"):
        if arm == "f32":
            os.environ["RCN_MID_I8"] = "0"
        m = HipL2Matcher(device=0)                # (the switches are read here)
        for i, im in enumerate(ims):
            m.upload(i, im)
        for rep in range(2):
            out, cnt = m.match_grid(pairs, exp.shape[1])
            assert np.array_equal(out, exp) and np.array_equal(cnt, ec), (name, arm, rep, "differs from the oracle", np.argwhere(out != exp)[:5].tolist())
        st = m.stats()
        res[arm] = {k: int(st[k]) for k in ("rows_total", "rows_reranked", "rows_exact_fallback", "rows_brute_force", "chunks", "coarse_dtype")}
        m.ctx.close()
    print(json.dumps(res))
    print("OK")


def check_lists():
    import torch  # noqa: F401
    import int8_emu as emu
    from reconstructor_amd import _lib, synth
    from reconstructor_amd.matcher import HipL2Matcher
    lib = _lib.load()
    assert b"DIAGNOSTIC" in lib.rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    lib.rcn_diag_coarse_table.restype = C.c_int
    lib.rcn_diag_coarse_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]
    lib.rcn_diag_i8.restype = C.c_int
    lib.rcn_diag_i8.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rcn_diag_mid.restype = C.c_int
    lib.rcn_diag_mid.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    ims = synth.descriptor_set("superpoint", 2, [1024, 1024], n_world=2048, seed=6)
    ims[1][700] = ims[1][3]                                      # an exact tie among the train rows
    rng = np.random.default_rng(4)
    ims[1][200:240] = ims[1][100] + (rng.standard_normal((40, 256)) * 1e-4).astype(np.float32)      # a cluster longer than a candidate list
    ims[0][5] = ims[1][100] + (rng.standard_normal(256) * 1e-3).astype(np.float32)                  # ... and a query that meets it
    m = HipL2Matcher(device=0)
    for i, im in enumerate(ims):
        m.upload(i, im)
    from oracle import orc
    pair = np.array([[0, 1]], np.int32)
    exp, ec = orc.match_grid(ims, pair, threads=8)
    out, cnt = m.match_grid(pair, 1024)
    assert np.array_equal(out, exp) and np.array_equal(cnt, ec), "differs from the oracle"
    st = m.stats()
    assert st["coarse_dtype"] == 2 and st["chunks"] == 1, st
    model = (C.c_double * 8)()
    m.ctx.check(lib.rcn_diag_i8(m.ctx.h, model, 0, None, None, None))
    s, bias, rho, tau, n_max = model[1], model[2], model[3], model[4], model[5]
    S = emu.fix_scale(ims)
    assert S is not None and S["s"] == s and S["bias"] == bias
    qq, rq, nq = emu.quantise(ims[0], s)
    tq, _, _ = emu.quantise(ims[1], s)
    acc = emu.accumulators(qq, tq, emu.half_norms(ims[1], S))    # the model's integers (tests/test_int8_gpu.py: the device's are the same)
    mdl = (C.c_double * 8)()
    m.ctx.check(lib.rcn_diag_coarse_table(m.ctx.h, None, 0, mdl))
    cand = np.zeros((int(mdl[4]), 2), np.uint32)
    m.ctx.check(lib.rcn_diag_coarse_table(m.ctx.h, cand.ctypes.data, cand.size, mdl))
    assert np.array_equal(cand[:1024], emu.keys_top2(acc))
    n = C.c_int64(0)
    m.ctx.check(lib.rcn_diag_mid(m.ctx.h, C.byref(n), None, None, None, None, 0))
    n = int(n.value)
    assert n == st["rows_exact_fallback"], (n, st)
    ent = np.zeros(n, np.uint64)
    tacc = np.zeros(n, np.uint32)
    cc = np.zeros(n, np.uint32)
    cl = np.zeros((n, MIDCAP), np.int32)
    nn = C.c_int64(0)
    m.ctx.check(lib.rcn_diag_mid(m.ctx.h, C.byref(nn), ent.ctypes.data, tacc.ctypes.data, cc.ctypes.data, cl.ctypes.data, n))
    q = (ent & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (ent >> np.uint64(32) == 0).all() and len(set(q.tolist())) == n
    # the threshold as the device must have computed it: eb from the two K1 candidates' fp64 distances
    i0, i1 = (cand[q, 0] & 0xFFF).astype(np.int64), (cand[q, 1] & 0xFFF).astype(np.int64)

    def d2_of(a, b):
        d = a.astype(np.float64) - b.astype(np.float64)
        o = np.zeros(len(d))
        for k in range(d.shape[1]):
            o += d[:, k] * d[:, k]
        return o
    eb = np.maximum(d2_of(ims[0][q], ims[1][i0]), d2_of(ims[0][q], ims[1][i1]))
    nq2 = (ims[0][q].astype(np.float64) ** 2).sum(1)
    E = (nq[q] * rho + rq[q] * (tau + rho)) * (1.0 + 1e-9) + 0.5 + 1.0e-3
    thr_model = np.floor(bias + 0.5 * s * s * (eb * (1 + 1e-9) + 1e-9 * (nq2 + n_max ** 2) - nq2) + E) + 1.0
    own = tacc != 0
    over = 0
    for r in np.nonzero(own)[0]:
        assert abs(float(tacc[r]) - thr_model[r]) <= 1.0, (int(r), int(tacc[r]), float(thr_model[r]))
        want = np.nonzero(acc[q[r]] <= int(tacc[r]))[0]
        assert cc[r] >= 2 and cc[r] == want.size, (int(r), int(cc[r]), want.size)
        assert i0[r] in want and i1[r] in want
        if cc[r] <= MIDCAP:
            assert np.array_equal(np.sort(cl[r, : cc[r]]), want), (int(r), "the emitted rows are not the rows under the threshold")
        else:
            over += 1
            assert np.isin(cl[r], want).all() and len(set(cl[r].tolist())) == MIDCAP
    print("rows in the tier %d, with an integer threshold %d, lists beyond %d rows: %d, longest %d" % (n, int(own.sum()), MIDCAP, over, int(cc.max()) if n else 0))
    assert own.sum() > 0
    print(json.dumps({"rows": n, "own": int(own.sum()), "over": over, "rows_brute_force": int(st["rows_brute_force"])}))
    print("OK")


if __name__ == "__main__":
    if sys.argv[1] == "grid":
        check_grid(sys.argv[2])
    else:
        check_lists()
