"""Guided matching on the GPU (csrc/guided.hip) against its contract (tests/guided_ref.py): every check is an equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import guided_ref

pytestmark = pytest.mark.gpu

RECT = guided_ref.RECT_F


def _matcher(ctx):
    from reconstructor_amd.matcher import HipL2Matcher
    m = HipL2Matcher(ctx=ctx)
    m.clear()
    m.set_workspace_rows(0)
    return m


def _upload(m, desc, coords):
    for i in sorted(desc):
        m.upload(i, desc[i])
        m.upload_coords(i, coords[i])


@functools.lru_cache(maxsize=None)
def _shape_ref(K1, K2, D):
    q, xy1, t, xy2, F = guided_ref.shape_case(K1, K2, D, seed=1000 + K1 + 7 * K2 + D)
    one, cand = guided_ref.match_pair(q, xy1, t, xy2, F)
    cross, _ = guided_ref.match_pair(q, xy1, t, xy2, F, cross_check=1)
    for a in (q, xy1, t, xy2, F, one, cross):
        a.setflags(write=False)
    return (q, xy1, t, xy2, F), one, cross, cand


@pytest.mark.parametrize("D", guided_ref.DIMS)
def test_shapes_one_way_and_cross_checked(gpu_ctx, D):
    """Two-view scenes of every shape: K2 = 63, 64, 65 straddle the 64-row train tile, 300 x 515 takes several blocks per pair.  All four
    widths ride the whole-row path (D = 40: a row shorter than the wave's 64 x 16 bytes); test_generic_width covers the other path."""
    from reconstructor_amd import guided
    some = 0
    for K1, K2 in guided_ref.SHAPES:
        case, one, cross, cand = _shape_ref(K1, K2, D)
        got = guided.match_pair(gpu_ctx, *case)
        assert np.array_equal(got, one), (K1, K2)
        got = guided.match_pair(gpu_ctx, *case, guided.options(cross_check=1))
        assert np.array_equal(got, cross), (K1, K2)
        some += int((one >= 0).sum())
    assert some > 100


@pytest.mark.parametrize("D", [30, 258, 300])
def test_generic_width(gpu_ctx, D):
    """D % 4 != 0 and D > 256: every candidate lane walks its chain out of global memory; the same contract."""
    from reconstructor_amd import guided
    for K1, K2 in ((65, 63), (40, 130)):
        case, one, cross, _ = _shape_ref(K1, K2, D)
        assert np.array_equal(guided.match_pair(gpu_ctx, *case), one)
        assert np.array_equal(guided.match_pair(gpu_ctx, *case, guided.options(cross_check=1)), cross)
    q, xy1, t, xy2, F = guided_ref.planted_counts_case(D)
    assert np.array_equal(guided.match_pair(gpu_ctx, q, xy1, t, xy2, F), guided_ref.match_pair(q, xy1, t, xy2, F)[0])


@pytest.mark.parametrize("D", guided_ref.DIMS)
def test_planted_candidate_counts(gpu_ctx, D):
    """Rectified F: 0, 1, 2, 23, 24, 25, 49 and 65 candidates per row (around the 24-row gather batch and the 64-lane sweep), and all of K2."""
    from reconstructor_amd import guided
    m = _matcher(gpu_ctx)
    cases = [guided_ref.planted_counts_case(D), guided_ref.all_in_band_case(3, 130, D), guided_ref.all_in_band_case(70, 200, D)]
    for n, (q, xy1, t, xy2, F) in enumerate(cases):
        _upload(m, {2 * n: q, 2 * n + 1: t}, {2 * n: xy1, 2 * n + 1: xy2})
    pairs = np.array([(0, 1), (2, 3), (4, 5)], np.int32)
    Fs = np.stack([c[4] for c in cases])
    idx, d2 = guided.knn2(gpu_ctx, pairs, Fs, 80)
    out, counts, cand = guided.match_guided(gpu_ctx, pairs, Fs, 80)
    assert list(idx[0, :8, 2]) == guided_ref.PLANT_COUNTS
    assert (idx[1, :3, 2] == 130).all() and (idx[2, :70, 2] == 200).all()
    for p, (q, xy1, t, xy2, F) in enumerate(cases):
        wi, wd = guided_ref.knn2(q, t, guided_ref.band(F, xy1, xy2))
        K1 = len(q)
        assert np.array_equal(idx[p, :K1], wi) and np.array_equal(d2[p, :K1], wd), p
        assert (idx[p, K1:] == [-1, -1, 0, 0]).all() and np.isinf(d2[p, K1:]).all()
        want, wc = guided_ref.match_pair(q, xy1, t, xy2, F, stride=80)
        assert np.array_equal(out[p], want) and counts[p] == (want >= 0).sum() and cand[p] == wc, p
    m.clear()


def _planted():
    """One rectified pair, query row r at y = 100 r; the answers are stated in test_planted_answers."""
    rng = np.random.default_rng(11)
    D = 64
    q = rng.standard_normal((8, D)).astype(np.float32)
    t = (3 + rng.standard_normal((16, D))).astype(np.float32)        # far from every query row
    ty = np.full(16, 5000)                                             # in nobody's band unless placed below
    # 0: the nearest row (an exact copy, row 0) is out of band, the second nearest (row 1) in band with a far third (row 2)
    t[0], t[1] = q[0], q[0] + np.float32(0.01)
    ty[0], ty[1], ty[2] = 4, 3, -3
    # 1: duplicate train rows 3 and 5, the lower index out of band
    t[3] = t[5] = q[1] + np.float32(0.01)
    ty[3], ty[5], ty[4] = 100 + 4, 100 + 2, 100 - 1
    # 2: duplicates 6 and 7 both in band
    t[6] = t[7] = q[2] + np.float32(0.01)
    ty[6], ty[7] = 200, 201
    # 3: a lone, far candidate (row 8)
    ty[8] = 300 - 3
    # 4 .. 6: integer rows at distances (7, 10), (14, 20), (70, 100) from their query row; 7: (6, 10)
    q[4:] = 0
    t[9:15] = 0
    q[4:, :3] = [5, -2, 9]
    t[9:15, :3] = [5, -2, 9]
    t[9, 7], t[10, 9] = 7, 10          # query 4: d2 = 49, 100
    t[11, 7], t[12, 9] = 14, 20        # query 5: 196, 400
    t[13, 7], t[14, 9] = 70, 100       # query 6: 4900, 10000
    ty[9], ty[10], ty[11], ty[12], ty[13], ty[14] = 400, 401, 500, 499, 600, 603
    t[15] = 0
    t[15, :3] = [5, -2, 9]
    t[15, 20] = 6                      # query 7: row 15 (d2 = 36) and row 16, a copy of row 10 (d2 = 100)
    xy1 = np.c_[rng.integers(0, 800, 8), 100 * np.arange(8)].astype(np.int32)
    t = np.concatenate([t, t[10:11]])  # row 16 = row 10: d2 = 100 from query 7
    ty = np.concatenate([ty, [702]])
    ty[15] = 700
    xy2 = np.c_[rng.integers(0, 800, len(t)), ty].astype(np.int32)
    return q, xy1, t, xy2


def test_planted_answers(gpu_ctx):
    from reconstructor_amd import guided
    q, xy1, t, xy2 = _planted()
    m = _matcher(gpu_ctx)
    _upload(m, {0: q, 1: t}, {0: xy1, 1: xy2})
    pairs = np.array([(0, 1)], np.int32)
    idx, d2 = guided.knn2(gpu_ctx, pairs, RECT, 8)
    idx, d2 = idx[0], d2[0]
    out = guided.match_pair(gpu_ctx, q, xy1, t, xy2, RECT)
    assert list(idx[0]) == [1, 2, 2, 0] and out[0] == 1                    # the exact copy (row 0) is out of band
    assert list(idx[1]) == [5, 4, 2, 0] and out[1] == 5                    # of the twins 3 and 5, only 5 is in band
    assert list(idx[2]) == [6, 7, 2, 0] and d2[2, 0] == d2[2, 1] and out[2] == -1      # twins in band: the lower first, the ratio test fails
    assert list(idx[3]) == [8, -1, 1, 0] and np.isinf(d2[3, 1]) and out[3] == 8       # a lone candidate is accepted
    assert [list(d2[r]) for r in (4, 5, 6)] == [[49.0, 100.0], [196.0, 400.0], [4900.0, 10000.0]]      # integer rows: exact integers
    assert list(out[4:7]) == [-1, -1, -1]                                  # 7 < fl32(0.7) * 10 is false in fp32, and so on
    assert list(d2[7]) == [36.0, 100.0] and out[7] == 15                   # 6 < fl32(0.7) * 10
    dist = np.sqrt(np.float32(d2[3, 0]))
    at = guided.match_pair(gpu_ctx, q, xy1, t, xy2, RECT, guided.options(max_distance=float(dist)))
    below = guided.match_pair(gpu_ctx, q, xy1, t, xy2, RECT, guided.options(max_distance=float(np.nextafter(dist, np.float32(0)))))
    assert at[3] == 8 and below[3] == -1
    # everything above once more through the contract
    assert np.array_equal(out, guided_ref.match_pair(q, xy1, t, xy2, RECT)[0])
    wi, wd = guided_ref.knn2(q, t, guided_ref.band(RECT, xy1, xy2))
    assert np.array_equal(idx, wi) and np.array_equal(d2, wd)
    assert np.array_equal(below, guided_ref.match_pair(q, xy1, t, xy2, RECT, max_distance=float(np.nextafter(dist, np.float32(0))))[0])
    m.clear()


def test_whole_image_band_equals_the_unguided_grid(gpu_ctx):
    """Rectified F with max_error_px = 1e4 and +inf: every train row is a candidate, so the table is rcn_match_grid_device's."""
    from reconstructor_amd import guided
    desc, coords, pairs, Ftrue = guided_ref.ragged_grid()
    m = _matcher(gpu_ctx)
    _upload(m, desc, coords)
    want, wc = m.match_grid(pairs, 130)
    Fs = np.tile(RECT, (len(pairs), 1))
    for err in (1e4, np.inf):
        out, counts, cand = guided.match_guided(gpu_ctx, pairs, Fs, 130, guided.options(max_error_px=err))
        assert np.array_equal(out, want) and np.array_equal(counts, wc)
        assert list(cand) == [len(desc[a]) * len(desc[b]) for a, b in pairs]
    assert wc.sum() > 100
    m.clear()


def test_cross_check(gpu_ctx):
    from reconstructor_amd import guided
    desc, coords, pairs, Ftrue = guided_ref.ragged_grid()
    m = _matcher(gpu_ctx)
    _upload(m, desc, coords)
    Fs = Ftrue
    opt = guided.options(cross_check=1, max_error_px=2.0)
    out, counts, _ = guided.match_guided(gpu_ctx, pairs, Fs, 130, opt)
    fwd = guided.knn2(gpu_ctx, pairs, Fs, 130, 2.0)
    Ft = np.ascontiguousarray(Fs.reshape(-1, 3, 3).transpose(0, 2, 1)).reshape(-1, 9)
    bwd = guided.knn2(gpu_ctx, pairs[:, ::-1], Ft, 130, 2.0)
    want = guided_ref.match_grid(desc, coords, pairs, Fs, 130, max_error_px=2.0, cross_check=1)
    for p, (a, b) in enumerate(pairs):
        K1, K2 = len(desc[a]), len(desc[b])
        r, rt = guided_ref.raw(fwd[0][p, :K1], fwd[1][p, :K1]), guided_ref.raw(bwd[0][p, :K2], bwd[1][p, :K2])
        both = np.full(130, -1, np.int32)
        for i, j in enumerate(r):
            if j >= 0 and rt[j] == i:
                both[i] = j
        assert np.array_equal(out[p], both), p
        kept = out[p][out[p] >= 0]
        assert len(set(kept.tolist())) == len(kept)
    assert np.array_equal(out, want[0]) and np.array_equal(counts, want[1]) and counts.sum() > 100
    m.clear()


def test_grid_with_the_filters_models(gpu_ctx):
    """Six ragged images (one empty), scrambled pairs with repeats: the model-keeping filter against the plain one and against the CSR
    entry's out_F; the guided grid on those models against the contract, chunked three ways, twice; rcn_match_grid_guided against the
    three calls made one by one."""
    import torch
    from reconstructor_amd import fmat, guided
    desc, coords, pairs, Ftrue = guided_ref.ragged_grid()
    P, stride = len(pairs), 133
    m = _matcher(gpu_ctx)
    _upload(m, desc, coords)
    raw_table, _ = m.match_grid(pairs, stride)

    def matched():
        t_d = torch.full((P, stride), -7, dtype=torch.int32, device="cuda")
        c_d = torch.zeros(P, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.match_grid_device(pairs, t_d.data_ptr(), stride, c_d.data_ptr())
        return t_d, c_d
    t0, c0 = matched()
    s0 = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.filter_table_device(pairs, t0.data_ptr(), stride, c0.data_ptr(), s0.data_ptr())
    t1, c1 = matched()
    s1, F_d = guided.filter_model_device(gpu_ctx, pairs, t1, c1)
    gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
    assert torch.equal(t0, t1) and torch.equal(c0, c1) and torch.equal(s0, s1)
    status, Fs = s1.cpu().numpy(), F_d.cpu().numpy()
    assert (status > 0).sum() >= 4 and (status <= 0).any()
    # the CSR entry on the same lists
    off, a, b = fmat.matches_to_csr([coords[i] for i in range(6)], pairs, raw_table)
    d = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (off, a if len(a) else np.zeros((1, 2), np.int32), b if len(b) else np.zeros((1, 2), np.int32))]
    mask_d = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device="cuda")
    cnt_d, it_d = torch.zeros(P, dtype=torch.int32, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    F2 = torch.full((P, 9), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.check(gpu_ctx.lib.rcn_fmat_filter_grid_device(gpu_ctx.h, P, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), mask_d.data_ptr(),
                                                          cnt_d.data_ptr(), it_d.data_ptr(), F2.data_ptr()))
    gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
    assert np.array_equal(F2.cpu().numpy().view(np.int64), Fs.view(np.int64)) and np.array_equal(cnt_d.cpu().numpy(), status)
    assert (Fs[status <= 0] == 0).all() and (Fs[status > 0, 8] == 1).all()

    # the guided grid on those models: the contract, whatever the chunking, bit for bit on a second run
    want = guided_ref.match_grid(desc, coords, pairs, Fs, stride)
    rows = sum(len(desc[b]) for _, b in pairs)
    seen = []
    for budget in (0, rows // 2 + 1, 1, 1):
        m.set_workspace_rows(budget)
        out, counts, cand = guided.match_guided_device(gpu_ctx, pairs, F_d, stride)
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        seen.append((out.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes(), cand.cpu().numpy().tobytes()))
    m.set_workspace_rows(0)
    assert all(s == seen[0] for s in seen)
    assert seen[0] == (want[0].tobytes(), want[1].tobytes(), want[2].tobytes())
    assert (want[1][status <= 0] == 0).all() and want[1].sum() > 100
    idx, d2 = guided.knn2(gpu_ctx, pairs, Fs, stride)
    for p, (a_, b_) in enumerate(pairs):
        wi, wd = guided_ref.knn2(desc[a_], desc[b_], guided_ref.band(Fs[p], coords[a_], coords[b_]))
        assert np.array_equal(idx[p, :len(wi)], wi) and np.array_equal(d2[p, :len(wd)], wd), p

    # the whole pair-loop body in one call: pairs with a model are re-matched, the others keep the filtered table
    filtered = t1.cpu().numpy()
    exp = np.where((status > 0)[:, None], want[0], filtered)
    out, counts, st = guided.grid_guided(gpu_ctx, pairs, stride)
    assert np.array_equal(st, status) and np.array_equal(out, exp) and np.array_equal(counts, (exp >= 0).sum(axis=1))
    m.clear()


def test_argument_errors(gpu_ctx):
    from reconstructor_amd import _lib, guided
    desc, coords, pairs, _ = guided_ref.ragged_grid(D=32)
    m = _matcher(gpu_ctx)
    _upload(m, desc, coords)
    m.upload(7, desc[0])                                  # descriptors without coordinates
    m.upload_coords(8, coords[0])                         # coordinates without descriptors
    m.upload(9, desc[0])
    m.upload_coords(9, coords[0][:-1])                    # counts differ
    F = np.tile(RECT, (1, 1))

    def code(fn):
        with pytest.raises(_lib.RcnError) as e:
            fn()
        return e.value.code
    for bad in ((0, 7), (7, 0), (0, 8), (0, 55)):
        assert code(lambda: guided.match_guided(gpu_ctx, [bad], F, 200)) == -5
        assert code(lambda: guided.knn2(gpu_ctx, [bad], F, 200)) == -5
        assert code(lambda: guided.grid_guided(gpu_ctx, [bad], 200)) == -5
    assert code(lambda: guided.match_guided(gpu_ctx, [(0, 9)], F, 200)) == -1
    assert code(lambda: guided.match_guided(gpu_ctx, [(0, 2)], F, len(desc[0]) - 1)) == -1      # stride below the query image
    assert code(lambda: guided.knn2(gpu_ctx, [(0, 2)], F, len(desc[0]) - 1)) == -1
    for kw in ({"ratio": 0.0}, {"ratio": -1.0}, {"ratio": float("nan")}, {"ratio": float("inf")}, {"max_error_px": 0.0}, {"max_error_px": -3.0},
               {"max_error_px": float("nan")}):
        assert code(lambda: guided.match_guided(gpu_ctx, [(0, 2)], F, 200, guided.options(**kw))) == -1, kw
        assert code(lambda: guided.match_pair(gpu_ctx, desc[0], coords[0], desc[2], coords[2], RECT, guided.options(**kw))) == -1, kw
        assert code(lambda: guided.grid_guided(gpu_ctx, [(0, 2)], 200, opt=guided.options(**kw))) == -1, kw
    assert code(lambda: guided.knn2(gpu_ctx, [(0, 2)], F, 200, max_error_px=0.0)) == -1
    guided.match_guided(gpu_ctx, [(0, 2)], F, 200, guided.options(max_error_px=float("inf")))     # allowed
    L, h = gpu_ctx.lib, gpu_ctx.h
    pr = np.array([(0, 2)], np.int32)
    o = guided.options()
    buf = np.zeros(400, np.int64)
    assert L.rcn_match_guided(h, pr.ctypes.data, 1, None, C.byref(o), buf.ctypes.data, 200, buf.ctypes.data, None) == -1
    assert L.rcn_match_guided(h, pr.ctypes.data, 1, F.ctypes.data, None, buf.ctypes.data, 200, buf.ctypes.data, None) == -1
    assert L.rcn_match_guided(h, pr.ctypes.data, 1, F.ctypes.data, C.byref(o), None, 200, buf.ctypes.data, None) == -1
    assert L.rcn_match_guided(h, None, 1, F.ctypes.data, C.byref(o), buf.ctypes.data, 200, buf.ctypes.data, None) == -1
    assert L.rcn_match_guided_device(h, pr.ctypes.data, 1, None, C.byref(o), None, 200, None, None) == -1
    assert L.rcn_guided_knn2_device(h, pr.ctypes.data, 1, None, 3.0, None, None, 200) == -1
    assert L.rcn_match_table_filter_model_device(h, pr.ctypes.data, 1, None, 200, None, None, None) == -1
    assert L.rcn_match_pair_guided(h, None, 3, None, None, 3, None, 32, F.ctypes.data, C.byref(o), None, None) == -1
    assert L.rcn_guided_default_options(None) == -1
    assert (o.ratio, o.max_error_px, o.max_distance, o.cross_check) == (np.float32(0.7), 3.0, 0.0, 0)
    assert guided.match_guided(gpu_ctx, np.zeros((0, 2), np.int32), np.zeros((0, 9)), 5)[0].shape == (0, 5)      # no pairs: nothing to do
    m.clear()


def test_smoke(gpu_ctx):
    from reconstructor_amd import guided
    rows, matches = guided.smoke(gpu_ctx)
    assert rows == matches == 96
