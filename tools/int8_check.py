"""The int8 coarse pass on the hardware against its numpy model (tests/int8_emu.py); run by tests/test_int8_gpu.py in a child
process with RCN_LIB=tools/librcn_diag.so (the diagnostic build returns the candidate table and the int8 images).

  keys   every int8 key the kernel left equals the exact integer accumulator of its (query, train) pair computed in numpy from
         the device's own quantised rows and half-norms, and those equal the model's; the stored norms are not below the true
         ones; the device's int8 / fp16 choice is the expected one per data kind.  RCN_COARSE_I8_S16=0 checks the other MFMA shape.
  grid   a ragged 256-d grid (both orientations, self pairs, repeated pairs, many pipeline chunks) against the oracle; prints a
         hash of the table so that the caller can compare the run with int8 forced off (RCN_COARSE_I8=0)."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def data_kinds():
    from reconstructor_amd import synth
    rng = np.random.default_rng(21)
    out = {}
    out["superpoint"] = (synth.descriptor_set("superpoint", 2, [1500, 2048], n_world=4096, seed=6), True)
    out["superpoint ragged small"] = (synth.descriptor_set("superpoint", 2, [63, 513], n_world=700, seed=7), True)
    ht = [rng.standard_t(2.5, (k, 256)).astype(np.float32) for k in (700, 640)]
    out["heavy-tailed"] = ([x / np.linalg.norm(x, axis=1, keepdims=True) for x in ht], False)
    huge = synth.descriptor_set("superpoint", 2, [600, 500], n_world=1500, seed=8)
    huge[0][200, 17] = 40.0
    out["one huge element"] = (huge, False)
    ints = [rng.integers(0, 4, (k, 256)).astype(np.float32) for k in (400, 600)]
    ints[1][300:330] = ints[1][:30]
    out["small integers (scale cap)"] = (ints, True)
    flat = np.full((64, 256), 0.37, np.float32)
    flat[1::2] *= -1.0
    out["all elements at the maximum"] = ([flat, flat[:50].copy()], True)
    out["sift 128-d"] = (synth.descriptor_set("sift", 2, [500, 700], n_world=1500, seed=3), False)
    return out


def check_keys():
    import torch  # noqa: F401
    import int8_emu as emu
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    lib = _lib.load()
    assert b"DIAGNOSTIC" in lib.rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    lib.rcn_diag_coarse_table.restype = C.c_int
    lib.rcn_diag_coarse_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]
    lib.rcn_diag_i8.restype = C.c_int
    lib.rcn_diag_i8.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    m = HipL2Matcher(device=0)
    for name, (ims, want_i8) in data_kinds().items():
        m.clear()
        for i, im in enumerate(ims):
            m.upload(i, im)
        pairs = np.array([[0, 1], [1, 0]], np.int32)
        kmax = max(len(x) for x in ims)
        m.match_grid(pairs[:1], kmax)                     # one pair: its candidate table is what the library keeps
        st = m.stats()
        model = (C.c_double * 8)()
        m.ctx.check(lib.rcn_diag_i8(m.ctx.h, model, 0, None, None, None))
        is_i8, s, bias, rho, tau = int(model[0]), model[1], model[2], model[3], model[4]
        print("%-30s int8 %d  s %.4f  BIAS %.0f  rho %.3f  tau %.2f  coarse_dtype %d" % (name, is_i8, s, bias, rho, tau, st["coarse_dtype"]), flush=True)
        assert is_i8 == int(want_i8), (name, "expected int8" if want_i8 else "expected fp16")
        assert st["coarse_dtype"] == (2 if want_i8 else 1) and st["used_mfma_path"] == 1, st
        if not want_i8:
            continue
        S = emu.fix_scale(ims)
        assert S is not None and S["s"] == s and S["bias"] == bias, (S, s, bias)
        dev = []
        for i, im in enumerate(ims):
            K = len(im)
            xq = np.zeros((K, 256), np.int8)
            hn = np.zeros(K, np.int32)
            nn = np.zeros((K, 2), np.float32)
            m.ctx.check(lib.rcn_diag_i8(m.ctx.h, model, i, xq.ctypes.data, hn.ctypes.data, nn.ctypes.data))
            q, rn, qn = emu.quantise(im, s)
            assert np.array_equal(xq.astype(np.int64), q), (name, i, "quantised rows differ from the model")
            assert np.array_equal(hn.astype(np.int64), emu.half_norms(im, S)), (name, i, "half-norms differ from the model")
            assert (nn[:, 0].astype(np.float64) >= qn).all() and (nn[:, 1].astype(np.float64) >= rn).all(), (name, i, "a stored norm is below the true one")
            assert (nn[:, 0] <= qn * (1 + 1e-6) + 1e-6).all() and (nn[:, 1] <= rn * (1 + 1e-6) + 2e-6).all(), (name, i, "a stored norm is far above the true one")
            assert rho >= nn[:, 1].max() and tau >= nn[:, 0].max()
            dev.append((q, hn.astype(np.int64)))
        assert rho <= emu.RES_MAX and tau <= S["M"]
        for qi, ti in ((0, 1), (1, 0)):
            m.match_grid(np.array([[qi, ti]], np.int32), kmax)
            mdl = (C.c_double * 8)()
            m.ctx.check(lib.rcn_diag_coarse_table(m.ctx.h, None, 0, mdl))
            kq_stride = int(mdl[4])
            cand = np.zeros((kq_stride, 2), np.uint32)
            m.ctx.check(lib.rcn_diag_coarse_table(m.ctx.h, cand.ctypes.data, cand.size, mdl))
            acc = emu.accumulators(dev[qi][0], dev[ti][0], dev[ti][1])
            assert acc.min() >= 1 and acc.max() < emu.PAD_ACC, (name, acc.min(), acc.max())
            want = emu.keys_top2(acc)
            got = cand[: len(ims[qi])]
            assert np.array_equal(got, want), (name, qi, ti, "keys differ from the exact integer accumulators", int((got != want).sum()))
    print("OK")


def check_grid():
    import torch  # noqa: F401
    from oracle import orc
    from reconstructor_amd import synth
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    m = HipL2Matcher(device=0)
    Ks = [4096, 1, 700, 2048, 0, 513, 63, 2, 3000, 1500]
    ims = synth.descriptor_set("superpoint", len(Ks), [max(k, 1) for k in Ks], n_world=6000, seed=12)
    ims = [np.ascontiguousarray(im[:k]) for im, k in zip(ims, Ks)]
    ims[2][5] = 0.0                                               # a zero row
    ims[3][100:110] = ims[3][:10]                                 # exact duplicates inside an image
    ap = all_pairs(len(Ks))
    selfp = np.array([[i, i] for i in range(len(Ks))], np.int32)
    pairs = np.concatenate([ap, ap[:, ::-1], selfp, ap[:7], ap[:7]]).astype(np.int32)
    exp, ec = orc.match_grid(ims, pairs, threads=8)
    for i, im in enumerate(ims):
        m.upload(i, im)
    h = hashlib.sha256()
    for rows in (0, 1 << 16, 1 << 14):                           # one chunk, then many (the last: a chunk per group)
        m.set_workspace_rows(rows)
        out, cnt = m.match_grid(pairs, exp.shape[1])
        st = m.stats()
        assert np.array_equal(out, exp) and np.array_equal(cnt, ec), ("differs from the oracle", rows, int((out != exp).sum()))
        h.update(out.tobytes()); h.update(cnt.tobytes())
        print("workspace rows %d: %d chunks, coarse_dtype %d, %d re-ranked, %d past the re-rank" % (rows, st["chunks"], st["coarse_dtype"], st["rows_reranked"], st["rows_exact_fallback"]), flush=True)
    m.set_workspace_rows(0)
    print("DTYPE", st["coarse_dtype"])
    print("HASH", h.hexdigest())
    print("OK")


if __name__ == "__main__":
    {"keys": check_keys, "grid": check_grid}[sys.argv[1]]()
