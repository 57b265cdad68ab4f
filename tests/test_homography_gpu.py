"""GPU suite: batched homography RANSAC (rcn_homography_ransac*, csrc/homography.hip) against tests/homography_ref.py bit
for bit -- H, mask, count, iterations; the wave, workgroup and LDS edges of the scoring loop; a ragged batch against its
pairs one at a time; the options; argument errors; the device entry against the host entry with guard words around every
output."""
import os

import numpy as np
import pytest

import homography_ref as hr
import nextview_ref as nr
import tri_ref
from reconstructor_amd import _lib, homography, nextview

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "homography_small.npz")
ERR_ARG = -1
KEYS = ("H", "mask", "count", "iterations")


def _batch(pairs):
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([len(p[0]) for p in pairs])
    xy1 = np.concatenate([np.asarray(p[0], np.int32).reshape(-1, 2) for p in pairs])
    xy2 = np.concatenate([np.asarray(p[1], np.int32).reshape(-1, 2) for p in pairs])
    return off, xy1, xy2


def _assert_same(got, want, what):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k in ("count", "iterations"):
            assert g.tolist() == w.tolist(), (what, k, g, w)
        else:
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, k)


@pytest.mark.parametrize("seed", (1, 2))
@pytest.mark.parametrize("share", (0.0, 0.3, 0.6))
def test_scenes_equal_the_restatement_bit_for_bit(gpu_ctx, seed, share):
    s = hr.scene(seed, share)
    off, xy1, xy2 = _batch([(s["xy1"], s["xy2"])])
    got = homography.find(gpu_ctx, off, xy1, xy2)
    _assert_same(got, hr.find_batch(off, xy1, xy2), (seed, share))
    assert got["count"][0] >= 0.8 * int((~s["wrong"]).sum())
    if share == 0.6:
        assert got["iterations"][0] > 3 * 32                # hundreds of iterations: several rounds


def test_edge_cases_equal_the_restatement_bit_for_bit(gpu_ctx):
    """All of them in one call."""
    cases = hr.edge_cases()
    off, xy1, xy2 = _batch([c[1:] for c in cases])
    got = homography.find(gpu_ctx, off, xy1, xy2)
    _assert_same(got, hr.find_batch(off, xy1, xy2), [c[0] for c in cases])
    assert not np.isnan(got["H"]).any()
    count = dict(zip([c[0] for c in cases], got["count"].tolist()))
    assert (count["n0"], count["n3"], count["n4"], count["identical"], count["line"], count["flip4"], count["n4_collinear"]) == (-2, -2, 4, -1, -1, -1, -1)


def test_golden(gpu_ctx):
    with np.load(GOLD) as g:
        got = homography.find(gpu_ctx, g["off"], g["xy1"], g["xy2"])
        _assert_same(got, {k: g[k] for k in KEYS}, "golden")


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 2047, 2048, 2049))
def test_sizes_at_the_edges_of_the_scoring_loop(gpu_ctx, n):
    """The wave (64) and workgroup (256) edges of the scoring loop and the count the kernel keeps in LDS (2048), at a share
    of 0.6 so that the search crosses several rounds."""
    s = hr.scene(40 + n % 7, 0.6, n=n)
    off, xy1, xy2 = _batch([(s["xy1"], s["xy2"])])
    got = homography.find(gpu_ctx, off, xy1, xy2)
    _assert_same(got, hr.find_batch(off, xy1, xy2), n)
    assert got["count"][0] >= 0.8 * int((~s["wrong"]).sum()) and got["iterations"][0] > 32


def test_batch_equals_single_calls(gpu_ctx):
    """A ragged batch gives every pair the bits of its single call, whatever its position."""
    sizes = [300, 0, 5, 2049, 64]
    pairs = [(lambda s: (s["xy1"], s["xy2"]))(hr.scene(60 + k, 0.15 * k, n=n)) for k, n in enumerate(sizes)]
    for order in ([0, 1, 2, 3, 4], [3, 4, 1, 0, 2]):
        sel = [pairs[k] for k in order]
        off, xy1, xy2 = _batch(sel)
        got = homography.find(gpu_ctx, off, xy1, xy2)
        for p, (a, b) in enumerate(sel):
            one = homography.find(gpu_ctx, [0, len(a)], a, b)
            lo, hi = int(off[p]), int(off[p + 1])
            assert got["H"][p].tobytes() == one["H"][0].tobytes() and got["mask"][lo:hi].tobytes() == one["mask"].tobytes(), (order, p)
            assert (got["count"][p], got["iterations"][p]) == (one["count"][0], one["iterations"][0]), (order, p)
    assert got["count"][2] == -2 and (got["count"] > 0).sum() == 4


def test_options_reach_the_kernel(gpu_ctx):
    s = hr.scene(3, 0.5, n=250)
    off, xy1, xy2 = _batch([(s["xy1"], s["xy2"])])
    o = homography.default_options(gpu_ctx)
    assert (o.threshold, o.confidence, o.max_iterations) == (3.0, 0.995, 2000)
    base = homography.find(gpu_ctx, off, xy1, xy2)
    for field, val in (("threshold", 0.8), ("confidence", 0.5), ("max_iterations", 7)):
        o = homography.default_options(gpu_ctx)
        setattr(o, field, val)
        got = homography.find(gpu_ctx, off, xy1, xy2, o)
        _assert_same(got, hr.find_batch(off, xy1, xy2, {field: val}), field)
        assert (got["count"][0], got["iterations"][0]) != (base["count"][0], base["iterations"][0]), field


def test_argument_errors(gpu_ctx):
    s = hr.scene(3, 0.0, n=120)
    xy1, xy2 = s["xy1"], s["xy2"]
    off = np.array([0, len(xy1)], np.int64)
    lib, h = gpu_ctx.lib, gpu_ctx.h
    H, mask, cnt, it = np.zeros(9), np.zeros(len(xy1), np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(off=off, xy1=xy1, xy2=xy2, opt=None, H=H, mask=mask, cnt=cnt, it=it, npairs=1):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.rcn_homography_ransac(h, npairs, p(off), p(xy1), p(xy2), opt, p(H), p(mask), p(cnt), p(it))

    assert call() == _lib.RCN_OK and cnt[0] > 100
    assert call(it=None) == _lib.RCN_OK
    for kw in (dict(off=None), dict(xy1=None), dict(xy2=None), dict(H=None), dict(mask=None), dict(cnt=None)):
        assert call(**kw) == ERR_ARG, kw
    assert call(npairs=-1) == ERR_ARG
    assert call(off=np.array([0, 10, 5], np.int64), npairs=2) == ERR_ARG
    assert call(off=np.array([1, len(xy1)], np.int64)) == ERR_ARG
    for field, val in (("confidence", 0.0), ("confidence", 1.0), ("threshold", 0.0), ("threshold", -1.0), ("max_iterations", 0)):
        o = homography.default_options(gpu_ctx)
        setattr(o, field, val)
        assert call(opt=o) == ERR_ARG, field
        assert lib.rcn_last_error(h)
    assert lib.rcn_homography_ransac(None, 1, off.ctypes.data, None, None, None, None, None, None, None) == ERR_ARG
    assert call() == _lib.RCN_OK                                    # the ctx is still usable


GUARD = 0x5A
NOT_RESIDENT = (7, 9)         # a pair of the scene whose list is left out of the upload (in both directions)


def _upload_coords(ctx, coords):
    for i, xy in coords.items():
        a = np.ascontiguousarray(np.asarray(xy, np.int32).reshape(-1, 2))
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))


def _resident(ctx, L):
    """The loop scene's coordinates and canonical i < j lists resident in the ctx (mirror on), one pair left out."""
    _upload_coords(ctx, L["coords"])
    lists = {k: v for k, v in nr.canonical_lists(L["feature_matches"]).items() if k != NOT_RESIDENT}
    nextview.upload_feature_matches(ctx, lists, mirror=True)


def _host_entries(L, i, j):
    qt = sorted(L["feature_matches"][(i, j)].items())
    return (np.array(qt, np.int32).reshape(-1, 2), np.array([L["coords"][i][f] for f, _ in qt], np.int32).reshape(-1, 2),
            np.array([L["coords"][j][g] for _, g in qt], np.int32).reshape(-1, 2))


def test_device_entry_equals_host_entry(gpu_ctx):
    """rcn_homography_ransac_device behind rcn_match_lists_upload and rcn_coords_upload against the host entry on the same
    pairs -- a stored orientation, mirrored ones, a pair without a list, a pair beyond `capacity` -- into outputs with guard
    words behind them, enqueued, one rcn_synchronize; then list entries outside the coordinates."""
    import torch
    ctx = gpu_ctx
    dev = torch.device("cuda", ctx.device)
    L = tri_ref.loop_containers(25, 1500, obs_per_point=10, seed=31, wrong_rate=0.0)
    _resident(ctx, L)
    try:
        pairs = [(20, 22), (22, 20), (0, 1), NOT_RESIDENT[::-1], (1, 0)]
        ents = [_host_entries(L, i, j) if (i, j) != NOT_RESIDENT[::-1] else (np.zeros((0, 2), np.int32),) * 3 for i, j in pairs]
        off = np.concatenate([[0], np.cumsum([len(e[0]) for e in ents])]).astype(np.int64)
        want = homography.find(ctx, off, np.concatenate([e[1] for e in ents]), np.concatenate([e[2] for e in ents]))
        assert (want["count"] > 0).sum() == 4 and want["count"][3] == -2
        total, n = int(off[-1]), len(pairs)
        pr = np.ascontiguousarray(pairs, np.int32)

        def run(cap):
            bufs = dict(off=torch.full((n + 1 + 4,), -7, dtype=torch.int64, device=dev), qt=torch.full((2 * cap + 8,), -7, dtype=torch.int32, device=dev),
                        H=torch.full((9 * n + 4,), 7.5, dtype=torch.float64, device=dev), mask=torch.full((cap + 16,), GUARD, dtype=torch.uint8, device=dev),
                        count=torch.full((n + 4,), -7, dtype=torch.int32, device=dev), iterations=torch.full((n + 4,), -7, dtype=torch.int32, device=dev))
            torch.cuda.synchronize(dev)
            ctx.check(ctx.lib.rcn_homography_ransac_device(ctx.h, n, pr.ctypes.data, None, cap, bufs["off"].data_ptr(), bufs["qt"].data_ptr(),
                                                           bufs["H"].data_ptr(), bufs["mask"].data_ptr(), bufs["count"].data_ptr(),
                                                           bufs["iterations"].data_ptr()))
            ctx.check(ctx.lib.rcn_synchronize(ctx.h))
            out = {k: v.cpu().numpy() for k, v in bufs.items()}
            assert (out["off"][n + 1:] == -7).all() and (out["qt"][2 * cap:] == -7).all() and (out["H"][9 * n:] == 7.5).all()
            assert (out["mask"][cap:] == GUARD).all() and (out["count"][n:] == -7).all() and (out["iterations"][n:] == -7).all()
            return out

        for cap in (total, total + 100):
            got = run(cap)
            assert got["off"][:n + 1].tolist() == off.tolist()
            assert got["qt"][:2 * total].tobytes() == np.concatenate([e[0] for e in ents]).tobytes()
            assert got["H"][:9 * n].tobytes() == want["H"].tobytes() and got["mask"][:total].tobytes() == want["mask"].tobytes(), cap
            assert got["count"][:n].tolist() == want["count"].tolist() and got["iterations"][:n].tolist() == want["iterations"].tolist()
        got = run(total - 1)                                          # no room for the last pair: count -2, the others untouched
        assert got["off"][:n + 1].tolist() == off[:-1].tolist() + [int(off[-2])] and got["count"][n - 1] == -2
        assert got["H"][:9 * (n - 1)].tobytes() == want["H"][:n - 1].tobytes() and not got["H"][9 * (n - 1):9 * n].any()
        # malformed: image 22's coordinates replaced by their first 40 rows; list entries that name later features are ignored
        _upload_coords(ctx, {22: np.asarray(L["coords"][22], np.int32).reshape(-1, 2)[:40]})
        r = homography.find_device(ctx, [(20, 22), (22, 20)], 600, device=dev)
        ctx.check(ctx.lib.rcn_synchronize(ctx.h))
        qt, xy1, xy2 = _host_entries(L, 20, 22)
        keep = qt[:, 1] < 40
        o = r["off"].cpu().numpy()
        assert o.tolist() == [0, int(keep.sum()), 2 * int(keep.sum())]
        w = homography.find(ctx, [0, int(keep.sum())], xy1[keep], xy2[keep])
        assert r["count"].cpu().numpy()[0] == w["count"][0] and r["mask"].cpu().numpy()[:o[1]].tobytes() == w["mask"].tobytes()
        assert r["H"].cpu().numpy()[0].tobytes() == w["H"][0].tobytes()
        with pytest.raises(_lib.RcnError) as e:
            homography.find_device(ctx, [(20, 20)], 100, device=dev)
        assert e.value.code == ERR_ARG
        with pytest.raises(_lib.RcnError) as e:
            homography.find_device(ctx, [(20, 99)], 100, device=dev)
        assert e.value.code == -5
    finally:
        ctx.check(ctx.lib.rcn_match_lists_clear(ctx.h))
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
