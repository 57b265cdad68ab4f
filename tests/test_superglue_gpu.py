"""GPU suite of SuperGlue's optimal-matching layer (csrc/superglue.hip) against tests/sg_ref.py.

Tolerance: logP within TOL = 4 x DEV32 of the float64 reference, DEV32 = 2.55e-5 being what the fp32 torch transcription of
the published forward deviates on the same cases (measured and printed by tests/test_superglue_ref.py); the factor 4 allows
for the other reduction order (bands, lanes) and the device's 1-2 ulp expf / logf against libm's < 1.  Measured on an
MI355X: see the printed figures (DESIGN section 20 records them).  Selection is compared on the rows and columns whose
decision cannot turn within that tolerance; the undecided ones are at most 2 % of a case.

Every case runs on both device paths where the pair fits the fused path's LDS budget; where it does not, forcing the fused
path is RCN_ERR_UNSUPPORTED, and that is what is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest

import sg_ref
from test_superglue_ref import TOL, case, row_residual, tie_case

pytestmark = pytest.mark.gpu

AUTO, FUSED, BANDED = 0, 1, 2
UNSUPPORTED, ERR_ARG = -4, -1


def fits(m, n):
    return (m + 1) * (n + 1) * 4 <= 131072


def sg():
    from reconstructor_amd import superglue
    return superglue


def run(ctx, S, path=AUTO, m=None, n=None, want_logp=True, **opt):
    """assign on a numpy batch [B][M][N] (or one matrix); returns numpy arrays."""
    import torch
    S = np.asarray(S, np.float32)
    S3 = S[None] if S.ndim == 2 else S
    dev = lambda c: None if c is None else torch.tensor(c, dtype=torch.int32).cuda()
    r = sg().assign(ctx, torch.from_numpy(S3.copy()).cuda(), dev(m), dev(n), sg().options(ctx, path=path, **opt), want_logp=want_logp)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


def same(a, b, keys=("matches0", "matches1", "mscores0", "mscores1", "table", "counts", "status", "logP")):
    return all(a[k] is None or a[k].tobytes() == b[k].tobytes() for k in keys)


def check_pair(r, b, m, n, logP, target=None, tag=""):
    """Pair b of result r (capacity M x N) against the float64 logP [m + 1][n + 1]."""
    M, N = r["matches0"].shape[1], r["matches1"].shape[1]
    got = r["logP"][b].astype(np.float64)
    inner_dev = np.abs(got[:m, :n] - logP[:m, :n]).max()
    dust_dev = max(np.abs(got[:m, N] - logP[:m, n]).max(), np.abs(got[M, :n] - logP[m, :n]).max(), abs(got[M, N] - logP[m, n]))
    print("%s (%d, %d): max |logP - f64| = %.3g inner, %.3g dustbins (allowed %.3g)" % (tag, m, n, inner_dev, dust_dev, TOL))
    assert inner_dev <= TOL and dust_dev <= TOL
    sel = sg_ref.select(logP)
    rows, cols = sg_ref.undecided(logP, TOL)
    assert rows.sum() <= 0.02 * m and cols.sum() <= 0.02 * n
    assert np.abs(r["mscores0"][b, :m] - sel["mscores0"])[~rows].max(initial=0) <= TOL
    assert np.abs(r["mscores1"][b, :n] - sel["mscores1"])[~cols].max(initial=0) <= TOL
    assert np.array_equal(r["matches0"][b, :m][~rows], sel["matches0"][~rows])
    assert np.array_equal(r["matches1"][b, :n][~cols], sel["matches1"][~cols])
    assert np.array_equal(r["table"][b, :m][~rows], sel["table"][~rows])
    assert r["counts"][b] == (r["table"][b] >= 0).sum() and r["status"][b] == 0
    # padding: -1 / 0
    assert (r["matches0"][b, m:] == -1).all() and (r["matches1"][b, n:] == -1).all() and (r["table"][b, m:] == -1).all()
    assert (r["mscores0"][b, m:] == 0).all() and (r["mscores1"][b, n:] == 0).all()
    if target is not None:
        planted = target >= 0
        assert ((r["table"][b, :m] == target) & planted & ~rows).sum() >= 0.5 * planted.sum()


@pytest.mark.parametrize("path", [FUSED, BANDED], ids=["fused", "banded"])
@pytest.mark.parametrize("m,n", sg_ref.SHAPES)
def test_logp_and_selection(gpu_ctx, m, n, path):
    S, logP, u, v, target = case(m, n)
    if path == FUSED and not fits(m, n):
        from reconstructor_amd import _lib
        with pytest.raises(_lib.RcnError) as e:
            run(gpu_ctx, S, FUSED)
        assert e.value.code == UNSUPPORTED
        return
    r = run(gpu_ctx, S, path)
    check_pair(r, 0, m, n, logP, target, "fused" if path == FUSED else "banded")
    # marginals of the device's own logP (independent of the reference but for the convergence figure of the case)
    norm, log_mu, log_nu = sg_ref.marginals(m, n)
    P = np.exp(r["logP"][0].astype(np.float64) + norm)
    assert np.abs(P.sum(0) / np.exp(log_nu) - 1).max() <= TOL
    assert np.abs(P.sum(1) / np.exp(log_mu) - 1).max() <= np.expm1(np.abs(row_residual(S, u, v)).max()) + TOL
    # run to run
    assert same(r, run(gpu_ctx, S, path))


@functools.lru_cache(maxsize=None)
def ragged():
    M = N = 272
    S = np.full((4, M, N), np.nan, np.float32)
    for b, (m, n) in enumerate(sg_ref.RAGGED):
        if m and n:
            S[b, :m, :n] = case(m, n)[0]
    S.setflags(write=False)
    return S, [s[0] for s in sg_ref.RAGGED], [s[1] for s in sg_ref.RAGGED]


@pytest.mark.parametrize("path", [AUTO, BANDED], ids=["auto", "banded"])
def test_ragged_batch(gpu_ctx, path):
    S, ms, ns = ragged()
    r = run(gpu_ctx, S, path, ms, ns)
    for b, (m, n) in enumerate(sg_ref.RAGGED):
        if m == 0 or n == 0:
            assert (r["matches0"][b] == -1).all() and (r["matches1"][b] == -1).all() and (r["table"][b] == -1).all()
            assert not r["mscores0"][b].any() and not r["mscores1"][b].any() and r["counts"][b] == 0 and r["status"][b] == 0
            assert not r["logP"][b].any()
            continue
        check_pair(r, b, m, n, case(m, n)[1], case(m, n)[4], "batch")
        assert not r["logP"][b, m:272].any() and not r["logP"][b, :, n:272].any()       # padding of logP: zeros
        # the pair alone, at its own size: bit for bit
        alone = run(gpu_ctx, S[b, :m, :n], path)
        for k in ("matches0", "mscores0", "table"):
            assert r[k][b, :m].tobytes() == alone[k][0].tobytes(), k
        for k in ("matches1", "mscores1"):
            assert r[k][b, :n].tobytes() == alone[k][0].tobytes(), k
        assert r["logP"][b, :m, :n].tobytes() == alone["logP"][0, :m, :n].tobytes()
        assert r["logP"][b, 272, :n].tobytes() == alone["logP"][0, m, :n].tobytes() and r["logP"][b, :m, 272].tobytes() == alone["logP"][0, :m, n].tobytes()
        assert r["counts"][b] == alone["counts"][0]
    # every pair its own chunk: bit for bit
    sg().set_chunk_bytes(gpu_ctx, 1)
    try:
        assert same(r, run(gpu_ctx, S, path, ms, ns))
    finally:
        sg().set_chunk_bytes(gpu_ctx, 0)
    # counts outside 0..M / 0..N are clamped
    assert same(r, run(gpu_ctx, S, path, [200, -3, 33, 9999], [257, 40, 47, 272]))


def test_strided_scores(gpu_ctx):
    import torch
    S = case(33, 47)[0]
    big = np.full((2, 33 * 2, 47 * 3 + 1), np.nan, np.float32)
    big[:, ::2, 1::3] = S
    want = run(gpu_ctx, S)
    view = torch.from_numpy(big).cuda()[:, ::2, 1::3]
    assert not view.is_contiguous()
    for path in (FUSED, BANDED):
        want = run(gpu_ctx, S, path)
        r = sg().assign(gpu_ctx, view, opt=sg().options(gpu_ctx, path=path), want_logp=True)
        for b in range(2):
            assert all(r[k][b].cpu().numpy().tobytes() == want[k][0].tobytes() for k in ("matches0", "matches1", "mscores0", "mscores1", "table", "logP"))
    # the transposed view: the pair (n, m)
    t = sg().assign(gpu_ctx, torch.from_numpy(np.ascontiguousarray(S.T)).cuda()[None].transpose(1, 2), want_logp=False)
    assert t["matches0"][0].cpu().numpy().tobytes() == want["matches0"][0].tobytes()


@pytest.mark.parametrize("channel_first", [False, True], ids=["BKD", "BDK"])
def test_scores_bound_and_match_is_scores_then_assign(gpu_ctx, channel_first):
    import torch
    B, M, N, D = 3, 75, 101, 256                 # no multiples of the 32 x 32 tile
    ms, ns = [75, 37, 0], [101, 53, 40]
    rng = np.random.default_rng(21)
    d0 = np.full((B, M, D), np.nan, np.float32)
    d1 = np.full((B, N, D), np.nan, np.float32)
    for b in range(B):
        a, c, _ = sg().planted_pair(rng, max(ms[b], 1), ns[b], 20)
        d0[b, :ms[b]], d1[b, :ns[b]] = a[:ms[b]], c
    t0, t1 = torch.from_numpy(d0).cuda(), torch.from_numpy(d1).cuda()
    if channel_first:
        t0, t1 = t0.transpose(1, 2).contiguous(), t1.transpose(1, 2).contiguous()      # [B][D][K], the network's layout
    mm, nn = torch.tensor(ms, dtype=torch.int32).cuda(), torch.tensor(ns, dtype=torch.int32).cuda()
    S = sg().scores(gpu_ctx, t0, t1, mm, nn, channel_first=channel_first)
    Sh = S.cpu().numpy()
    worst = 0.0
    for b in range(B):
        m, n = ms[b], ns[b]
        assert np.isnan(Sh[b, m:]).all() and np.isnan(Sh[b, :, n:]).all()              # padding not written
        if m == 0:
            continue
        a, c = d0[b, :m].astype(np.float64), d1[b, :n].astype(np.float64)
        bound = (D + 2) * 2.0 ** -24 * (np.abs(a) @ np.abs(c).T) / np.sqrt(D)
        err = np.abs(Sh[b, :m, :n] - a @ c.T / np.sqrt(D))
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    print("scores: largest error / bound = %.3g" % worst)
    r1 = sg().assign(gpu_ctx, S, mm, nn, want_logp=True)
    r2 = sg().match(gpu_ctx, t0, t1, mm, nn, channel_first=channel_first, want_logp=True)
    for k in r1:
        assert r1[k].cpu().numpy().tobytes() == r2[k].cpu().numpy().tobytes(), k
    assert r1["counts"].cpu().numpy()[0] >= 10


@pytest.mark.parametrize("path", [FUSED, BANDED], ids=["fused", "banded"])
def test_exact_ties_go_to_the_lower_index(gpu_ctx, path):
    import torch
    d0, d1, i, c1, c2 = tie_case()
    S = sg().scores(gpu_ctx, torch.from_numpy(d0[None]).cuda(), torch.from_numpy(d1[None]).cuda())
    Sh = S.cpu().numpy()[0]
    assert np.array_equal(Sh[:, c1], Sh[:, c2])
    r = run(gpu_ctx, Sh, path)
    assert np.array_equal(r["logP"][0][:, c1], r["logP"][0][:, c2]), "identical columns got different potentials"
    assert r["matches0"][0, i] == c1 and r["matches1"][0, c1] == i and r["matches1"][0, c2] == -1 and r["mscores1"][0, c2] == 0
    sel = sg_ref.select(sg_ref.assign(Sh)[0])
    assert abs(r["mscores0"][0, i] - sel["mscores0"][i]) <= TOL
    # duplicated rows of d0 as well: identical rows, the lower row keeps the column
    St = np.ascontiguousarray(Sh.T)
    rt = run(gpu_ctx, St, path)
    assert np.array_equal(rt["logP"][0][c1, :], rt["logP"][0][c2, :])
    assert rt["matches1"][0, i] == c1 and rt["matches0"][0, c1] == i and rt["matches0"][0, c2] == -1


@pytest.mark.parametrize("path", [FUSED, BANDED], ids=["fused", "banded"])
def test_zero_iterations_and_dustbin_dominated(gpu_ctx, path):
    S = case(33, 47)[0]
    r = run(gpu_ctx, S, path, iterations=0)
    logP = sg_ref.assign(S, iterations=0)[0]
    assert np.abs(r["logP"][0].astype(np.float64) - logP).max() <= 2.0 ** -22 * 16          # one rounding of sums below 16
    sel = sg_ref.select(logP)
    rows, cols = sg_ref.undecided(logP, TOL)
    assert np.array_equal(r["matches0"][0][~rows], sel["matches0"][~rows]) and np.array_equal(r["table"][0][~rows], sel["table"][~rows])
    # pure noise under a large alpha: everything goes to the dustbins
    noise = np.random.default_rng(3).standard_normal((40, 50)).astype(np.float32)
    r = run(gpu_ctx, noise, path, alpha=20.0)
    assert (r["matches0"] == -1).all() and (r["matches1"] == -1).all() and (r["table"] == -1).all() and r["counts"][0] == 0
    assert r["status"][0] == 0 and np.abs(r["logP"][0].astype(np.float64) - sg_ref.assign(noise, alpha=20.0)[0]).max() <= TOL


@pytest.mark.parametrize("path", [AUTO, BANDED], ids=["auto", "banded"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_non_finite_score_clears_that_pair_only(gpu_ctx, path, bad):
    S = np.stack([case(33, 47)[0]] * 3).copy()
    S[1, 20, 11] = bad
    r = run(gpu_ctx, S, path)
    assert r["status"].tolist() == [0, 1, 0] and r["counts"][1] == 0 and r["counts"][0] == r["counts"][2] > 0
    assert (r["matches0"][1] == -1).all() and (r["matches1"][1] == -1).all() and (r["table"][1] == -1).all()
    assert not r["mscores0"][1].any() and not r["mscores1"][1].any()
    good = run(gpu_ctx, S[0], path)
    for b in (0, 2):
        assert all(r[k][b].tobytes() == good[k][0].tobytes() for k in ("matches0", "matches1", "mscores0", "mscores1", "table", "logP"))
    # a score of -inf is a legitimate "never": the pair stays valid
    S[1, 20, 11] = -np.inf
    r = run(gpu_ctx, S, path)
    assert r["status"].tolist() == [0, 0, 0] and r["matches0"][1, 20] != 11


def test_table_feeds_compaction_and_the_resident_lists():
    """table -> rcn_match_compact_begin / _wait -> rcn_match_lists_upload(mirror = 1): the lists are injective and hold the
    std::map of the reference at its threshold 0.5."""
    import torch
    from reconstructor_amd import _lib, nextview
    ctx = _lib.Context(0)
    try:
        S, ms, ns = ragged()
        r = sg().assign(ctx, torch.from_numpy(S.copy()).cuda(), torch.tensor(ms, dtype=torch.int32).cuda(), torch.tensor(ns, dtype=torch.int32).cuda(),
                        table_stride=300)
        B = len(ms)
        offsets = np.zeros(B + 1, np.int64)
        qt = np.zeros((B * 272, 2), np.int32)
        total = C.c_int64()
        ctx.check(ctx.lib.rcn_match_compact_begin(ctx.h, r["table"].data_ptr(), 300, r["counts"].data_ptr(), B, offsets.ctypes.data, qt.ctypes.data,
                                                  len(qt), C.byref(total)))
        ctx.check(ctx.lib.rcn_match_compact_wait(ctx.h))
        table = r["table"].cpu().numpy()
        assert (table[:, 272:] == -1).all() and total.value == offsets[-1] == (table >= 0).sum()
        for b, (m, n) in enumerate(sg_ref.RAGGED):
            got = {int(q): int(t) for q, t in qt[offsets[b]:offsets[b + 1]]}
            if m == 0 or n == 0:
                assert not got
                continue
            logP = case(m, n)[1]
            sel, (rows, _) = sg_ref.select(logP), sg_ref.undecided(logP, TOL)
            want = {i: int(sel["matches0"][i]) for i in range(m) if sel["matches0"][i] != -1 and sel["mscores0"][i] > 0.5}      # FeatureMatcherSuperglue.cpp:82
            assert {k: v for k, v in got.items() if not rows[k]} == {k: v for k, v in want.items() if not rows[k]}
            assert list(got) == sorted(got) and len(set(got.values())) == len(got)
        rng = np.random.default_rng(1)
        for img in range(B + 1):
            xy = rng.integers(0, 400, (272, 2)).astype(np.int32)
            ctx.check(ctx.lib.rcn_coords_upload(ctx.h, img, xy.ctypes.data, len(xy)))
        pairs = np.array([(b, b + 1) for b in range(B)], np.int32)
        nextview.upload_lists(ctx, pairs, offsets, qt[:total.value], mirror=True)
        ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
    finally:
        ctx.close()


def test_argument_errors(gpu_ctx):
    import torch
    from reconstructor_amd import _lib
    L, h = gpu_ctx.lib, gpu_ctx.h
    B, M, N, D = 2, 8, 9, 16
    S = torch.zeros((B, M, N), dtype=torch.float32).cuda()
    d0, d1 = torch.zeros((B, M, D)).cuda(), torch.zeros((B, N, D)).cuda()
    m0, cnt = torch.zeros((B, 16), dtype=torch.int32).cuda(), torch.zeros((B,), dtype=torch.int32).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())

    def assign(S_=S, B_=B, M_=M, N_=N, opt=None, m0_=m0, table=None, ts=0, counts=None):
        return L.rcn_sg_assign_device(h, p(S_) if S_ is not None else None, M * N, N, 1, None, None, B_, M_, N_, C.byref(opt) if opt else None,
                                      p(m0_) if m0_ is not None else None, None, None, None, p(table) if table is not None else None, ts,
                                      p(counts) if counts is not None else None, None, None)

    def scores(d0_=d0, d1_=d1, out=S, B_=B, M_=M, N_=N, D_=D):
        q = lambda t: p(t) if t is not None else None
        return L.rcn_sg_scores_device(h, q(d0_), M * D, D, 1, q(d1_), N * D, D, 1, None, None, B_, M_, N_, D_, q(out))

    o = lambda **kw: sg().options(gpu_ctx, **kw)
    assert assign() == 0 and scores() == 0
    assert assign(S_=None) == ERR_ARG and assign(m0_=None) == ERR_ARG
    assert assign(B_=-1) == ERR_ARG and assign(M_=0) == ERR_ARG and assign(N_=0) == ERR_ARG
    assert assign(table=m0, ts=M - 1, counts=cnt) == ERR_ARG and assign(table=m0, ts=16, counts=None) == ERR_ARG
    assert assign(table=m0, ts=16, counts=cnt) == 0
    assert assign(opt=o(iterations=-1)) == ERR_ARG and assign(opt=o(path=3)) == ERR_ARG
    for bad in (-0.1, 1.0, float("nan")):
        assert assign(opt=o(match_threshold=bad)) == ERR_ARG and assign(opt=o(score_threshold=bad)) == ERR_ARG
    assert assign(opt=o(alpha=float("inf"))) == ERR_ARG and assign(opt=o(alpha=float("nan"))) == ERR_ARG
    assert assign(M_=4097) == UNSUPPORTED and assign(N_=4097) == UNSUPPORTED
    assert b"bad argument" in L.rcn_last_error(h) or b"above" in L.rcn_last_error(h)
    assert scores(d0_=None) == ERR_ARG and scores(d1_=None) == ERR_ARG and scores(out=None) == ERR_ARG
    assert scores(B_=-1) == ERR_ARG and scores(M_=0) == ERR_ARG and scores(N_=0) == ERR_ARG and scores(D_=0) == ERR_ARG and scores(M_=4097) == UNSUPPORTED
    # B == 0 launches nothing (null buffers would fault if it did)
    assert assign(B_=0) == 0 and scores(B_=0) == 0
    match = lambda D_=D, d0_=d0: L.rcn_sg_match_device(h, p(d0_) if d0_ is not None else None, M * D, D, 1, p(d1), N * D, D, 1, None, None, B, M, N, D_, None,
                                                        p(m0), None, None, None, None, 0, None, None, None)
    assert match() == 0 and match(D_=0) == ERR_ARG and match(d0_=None) == ERR_ARG
    assert L.rcn_sg_set_chunk_bytes(None, 0) == ERR_ARG
    gpu_ctx.check(L.rcn_synchronize(h))
    dflt = _lib.SgOptions()
    L.rcn_sg_default_options(C.byref(dflt))
    assert (dflt.alpha, dflt.match_threshold, dflt.score_threshold, dflt.iterations, dflt.path) == (1.0, 0.2, 0.5, 100, 0)
