"""The two passes over the dense match table -- uniqueness (k_unique_pair, csrc/match.hip, through the diagnostic build's
rcn_diag_unique_pair) and the compaction to lists (k_cmp_fill, csrc/store.hip, through rcn_match_compact_begin) -- against a numpy
restatement; run by tests/test_table_passes_gpu.py in a child process with RCN_LIB=tools/librcn_diag.so.

  python tools/table_passes_check.py <K>:<stride>[:<offset>] ...
      per argument a table of five pairs of K query rows each, rows `stride` entries apart (stride > K, or stride == K), the entries past K filled
      with junk; offset: the table starts that many entries past a 16-byte boundary.
        pair 0   random matches, about a third of the rows, many train rows claimed by several queries: the smallest query keeps it
        pair 1   no match at all
        pair 2   every query claims one of seven train rows
        pair 3   every query claims its own train row (nothing changes)
        pair 4   as pair 0, other draws
      Uniqueness: the rewritten table and the counts equal numpy's.  Compaction: the lists equal numpy's, ascending in the query row;
      then once more with counts[0] and counts[3] made smaller than the rows' non-negative entries: the surplus is dropped and every
      other pair's list is what it was.  Prints OK."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def unique_ref(tab, K):
    out = tab.copy()
    out[:, K:] = -1
    cnt = np.zeros(len(tab), np.int32)
    for p in range(len(tab)):
        owner = {}
        for q in range(K):
            t = int(tab[p, q])
            if t >= 0 and t not in owner:
                owner[t] = q                        # ascending q: the first is the smallest
        for q in range(K):
            t = int(tab[p, q])
            if t >= 0 and owner[t] != q:
                out[p, q] = -1
        cnt[p] = int((out[p, :K] >= 0).sum())
    return out, cnt


def lists_ref(tab, cnt):
    offs = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    rows = []
    for p in range(len(tab)):
        q = np.flatnonzero(tab[p] >= 0)[:cnt[p]]
        rows.append(np.stack([q, tab[p, q]], 1).astype(np.int32))
    return offs, np.concatenate(rows) if rows else np.zeros((0, 2), np.int32)


def check(ctx, K, stride, offset):
    import torch
    lib = ctx.lib
    assert b"DIAGNOSTIC" in lib.rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    lib.rcn_diag_unique_pair.restype = C.c_int
    lib.rcn_diag_unique_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    rng = np.random.default_rng(1000 * K + stride)
    P, Kt = 5, max(K, 8)
    tab = rng.integers(0, 1 << 20, (P, stride)).astype(np.int32)       # junk past K; never an index
    if K:
        for p in (0, 4):
            row = rng.integers(0, max(1, Kt // 3), K)
            row[rng.random(K) > 0.35] = -1
            tab[p, :K] = row
        tab[1, :K] = -1
        tab[2, :K] = rng.integers(0, 7, K)
        tab[3, :K] = rng.permutation(Kt)[:K]
    kk = np.array([[K, Kt]] * P, np.int32)
    buf = torch.zeros(P * stride + 8, dtype=torch.int32, device="cuda")
    dev = buf[offset:offset + P * stride]
    dev.copy_(torch.from_numpy(tab.reshape(-1)))
    cnt = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.check(lib.rcn_diag_unique_pair(ctx.h, kk.ctypes.data, P, C.c_void_p(dev.data_ptr()), stride, C.c_void_p(cnt.data_ptr())))
    want, wc = unique_ref(tab, K)
    got, gc = dev.cpu().numpy().reshape(P, stride), cnt.cpu().numpy()
    assert np.array_equal(got, want), ("uniqueness: table", np.argwhere(got != want)[:5].tolist())
    assert np.array_equal(gc, wc), ("uniqueness: counts", gc.tolist(), wc.tolist())
    assert int(buf[:offset].abs().sum().item()) == 0 and int(buf[offset + P * stride:].abs().sum().item()) == 0, "wrote outside the table"
    if K >= 255:
        assert wc[0] < (tab[0, :K] >= 0).sum() and wc[2] == 7 and wc[3] == K and wc[1] == 0      # contested rows were there

    def lists(counts):
        c = torch.from_numpy(counts).cuda()
        offs = np.zeros(P + 1, np.int64)
        qt = np.full((int(counts.sum()) + 4, 2), -9, np.int32)
        total = C.c_int64(0)
        torch.cuda.synchronize()
        ctx.check(lib.rcn_match_compact_begin(ctx.h, C.c_void_p(dev.data_ptr()), stride, C.c_void_p(c.data_ptr()), P, offs.ctypes.data,
                                              qt.ctypes.data, len(qt), C.byref(total)))
        ctx.check(lib.rcn_match_compact_wait(ctx.h))
        return offs, qt, int(total.value)

    for short in (False, True):
        counts = wc.copy()
        if short:
            counts[0] = max(0, counts[0] - 3)
            counts[3] = counts[3] // 2
        offs, qt, total = lists(counts)
        woffs, wqt = lists_ref(want, counts)
        assert total == counts.sum() and np.array_equal(offs, woffs), ("compaction: offsets", short)
        assert np.array_equal(qt[:total], wqt), ("compaction: lists", short, np.argwhere(qt[:total] != wqt)[:5].tolist())
        assert (qt[total:] == -9).all(), "compaction wrote past the lists"
        for p in range(P):
            assert (np.diff(qt[offs[p]:offs[p + 1], 0]) > 0).all()
    print("K %d, stride %d, offset %d: %s kept" % (K, stride, offset, wc.tolist()))


def main(specs):
    import torch  # noqa: F401  (first: one shared HIP runtime)
    from reconstructor_amd import _lib
    ctx = _lib.Context(0)
    for spec in specs:
        f = [int(x) for x in spec.split(":")]
        check(ctx, f[0], f[1], f[2] if len(f) > 2 else 0)
    ctx.close()
    print("OK")


if __name__ == "__main__":
    main(sys.argv[1:])
