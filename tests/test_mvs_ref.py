"""CPU suite of the plane sweep's contract (tests/mvs_ref.py): the numpy contract against an independent, slow
restatement in Python integers and floats, its properties on ray-cast scenes, the library's pure-host entries against it bit for bit, and
the golden file.  No GPU."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import mvs_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mvs_small.npz")


# ---- the independent restatement: one pixel, one plane, one source at a time; every window position warped by itself --------------

def slow_sample(img, H, x, y):
    rows, cols = len(img), len(img[0])
    w = (H[6] * x + H[7] * y) + H[8]
    if not w > 0.0:
        return None
    u, v = ((H[0] * x + H[1] * y) + H[2]) / w, ((H[3] * x + H[4] * y) + H[5]) / w
    if math.isnan(u) or math.isnan(v) or math.isinf(u) or math.isinf(v):
        return None
    qu, qv = math.floor(u * 32.0 + 0.5), math.floor(v * 32.0 + 0.5)
    if not (0 <= qu <= 32 * (cols - 1) and 0 <= qv <= 32 * (rows - 1)):
        return None
    x0, y0, wx, wy = qu // 32, qv // 32, qu % 32, qv % 32
    x1, y1 = min(x0 + 1, cols - 1), min(y0 + 1, rows - 1)
    return (32 - wy) * ((32 - wx) * img[y0][x0] + wx * img[y0][x1]) + wy * ((32 - wx) * img[y1][x0] + wx * img[y1][x1])


def slow_sweep(gray, ref, srcs, H, inv, R, min_sources, max_cost):
    imgs = [[[int(v) for v in row] for row in g] for g in gray]
    rows, cols = len(imgs[0]), len(imgs[0][0])
    n, D = (2 * R + 1) ** 2, len(inv)
    plane = np.full((rows, cols), -1, np.int16)
    depth, cost = np.zeros((rows, cols), np.float32), np.full((rows, cols), np.inf, np.float32)
    exact = []
    for y in range(rows):
        for x in range(cols):
            costs = [math.inf] * D
            if R <= x < cols - R and R <= y < rows - R:
                win = [(x + dx, y + dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
                a = [imgs[ref][py][px] for px, py in win]
                Sa, Saa = sum(a), sum(v * v for v in a)
                Va = n * Saa - Sa * Sa
                for k in range(D):
                    tot, cnt = 0.0, 0
                    for s, src in enumerate(srcs):
                        if src < 0 or Va <= 0:
                            continue
                        b = [slow_sample(imgs[src], [float(v) for v in H[s][k]], px, py) for px, py in win]
                        if any(v is None for v in b):
                            continue
                        Sb, Sbb, Sab = sum(b), sum(v * v for v in b), sum(p * q for p, q in zip(a, b))
                        Vb, A = n * Sbb - Sb * Sb, n * Sab - Sa * Sb
                        if Vb <= 0:
                            continue
                        c = 1.0 - float(A) / math.sqrt(float(Va) * float(Vb))
                        exact.append((c, Fraction(A * A, Va * Vb), A >= 0))
                        tot += c
                        cnt += 1
                    if cnt >= min_sources and cnt > 0:
                        costs[k] = tot / cnt
            k = min(range(D), key=lambda i: (costs[i], i))
            if math.isinf(costs[k]) or costs[k] > max_cost:
                continue
            r = float(inv[k])
            if 0 < k < D - 1 and math.isfinite(costs[k - 1]) and math.isfinite(costs[k + 1]):
                den = (costs[k - 1] - 2.0 * costs[k]) + costs[k + 1]
                if den > 0.0:
                    off = max(-0.5, min(0.5, (0.5 * (costs[k - 1] - costs[k + 1])) / den))
                    if off > 0.0:
                        r = float(inv[k]) + off * (float(inv[k + 1]) - float(inv[k]))
                    elif off < 0.0:
                        r = float(inv[k]) + off * (float(inv[k]) - float(inv[k - 1]))
            plane[y, x], depth[y, x], cost[y, x] = k, np.float32(1.0 / r), np.float32(costs[k])
    return plane, depth, cost, exact


def test_contract_equals_the_slow_restatement():
    """24 x 20, D = 5, S = 2 (one more source slot empty): every output bit, and the fp64 cost against the exact rational ZNCC."""
    sc, inv = M.small_case(20, 24, n=3, D=5)
    srcs = [1, -1, 2]
    H = M.homographies(sc["poses34"], sc["intrinsics"], 0, srcs, inv)
    for R, min_sources, max_cost in ((3, 2, 0.5), (1, 1, 0.05)):
        got = M.sweep_view(sc["gray"], 0, srcs, H, inv, radius=R, min_sources=min_sources, max_cost=max_cost)
        want = slow_sweep(sc["gray"], 0, srcs, H, inv, R, min_sources, max_cost)
        for g, w in zip(got, want[:3]):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
        assert (got[0] >= 0).sum() > 50
        assert (got[0] < 0).sum() > (0 if R == 3 else 20)                  # (R = 1 at max_cost 0.05 drops some pixels)
        for c, rho2, pos in want[3][::97]:
            rho = math.sqrt(float(rho2)) * (1 if pos else -1)
            assert abs((1.0 - c) - rho) < 1e-12


# ---- properties on the ray-cast scenes -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def walls():
    out = {}
    for kind in ("fronto", "slanted"):
        sc, inv = M.wall_case(kind)
        views = np.array([[0, 1, 2, 3]], np.int32)
        H = M.view_homographies(sc["poses34"], sc["intrinsics"], views, inv[None])
        plane, depth, cost = M.sweep_view(sc["gray"], 0, [1, 2, 3], H[0], inv, radius=3, min_sources=2, max_cost=0.5)
        for a in (plane, depth, cost):
            a.setflags(write=False)
        out[kind] = (sc, inv, plane, depth, cost)
    return out


def test_fronto_parallel_wall_lands_on_its_plane(walls):
    """The wall exactly on plane 13 of camera 0 (D = 32 over 1/8 .. 1/3, R = 3, three sources, min_sources 2).  Measured with this
    contract: the argmin is plane 13 at 5167 of 5371 valid pixels (96.2 %); asserted as the whole percent below."""
    sc, inv, plane, depth, cost = walls["fronto"]
    valid = plane >= 0
    hit = int((plane[valid] == 13).sum())
    print("fronto-parallel wall: plane 13 at %d of %d valid pixels (%.1f %%)" % (hit, valid.sum(), 100.0 * hit / valid.sum()))
    assert valid.sum() > 5000
    assert hit >= 0.96 * valid.sum()


def test_slanted_wall_is_within_one_plane(walls):
    """0.25 x + 0.1 y + z = 5.  Measured with this contract: 5248 of 5381 valid pixels within one plane of the truth (97.5 %)."""
    sc, inv, plane, depth, cost = walls["slanted"]
    valid = plane >= 0
    tk = M.true_planes(sc, inv)
    near = int((np.abs(plane[valid].astype(np.int64) - tk[valid]) <= 1).sum())
    print("slanted wall: %d of %d valid pixels within one plane (%.1f %%)" % (near, valid.sum(), 100.0 * near / valid.sum()))
    assert valid.sum() > 5000
    assert near >= 0.97 * valid.sum()


def test_a_repeated_plane_value_yields_the_lower_index(walls):
    sc, inv, plane, _, _ = walls["fronto"]
    twice = np.repeat(inv[10:17], 2)                                       # planes 2k and 2k + 1 are the same plane: exact ties
    H = M.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 2, 3], twice)
    p2, d2, c2 = M.sweep_view(sc["gray"], 0, [1, 2, 3], H, twice, radius=3, min_sources=2, max_cost=0.5)
    assert (p2 >= 0).sum() > 5000 and (p2[p2 >= 0] % 2 == 0).all()
    H1 = M.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 2, 3], inv[10:17])
    p1, d1, c1 = M.sweep_view(sc["gray"], 0, [1, 2, 3], H1, inv[10:17], radius=3, min_sources=2, max_cost=0.5)
    assert np.array_equal(p2 >= 0, p1 >= 0) and np.array_equal(p2[p2 >= 0] // 2, p1[p1 >= 0]) and np.array_equal(c1, c2)
    # (the depths differ where the parabola applied: a repeated neighbour has no gap to move across)
    same = np.array_equal(d1, d2)
    assert not same and np.array_equal(d2[p2 >= 0], (1.0 / twice[p2[p2 >= 0]]).astype(np.float32))


def test_a_constant_reference_patch_is_invalid(walls):
    sc, inv, plane, _, _ = walls["fronto"]
    gray = sc["gray"].copy()
    gray[0, 20:40, 30:60] = 77
    H = M.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 2, 3], inv)
    p, d, c = M.sweep_view(gray, 0, [1, 2, 3], H, inv, radius=3, min_sources=2, max_cost=0.5)
    assert (p[23:37, 33:57] == -1).all() and (d[23:37, 33:57] == 0).all() and np.isinf(c[23:37, 33:57]).all()      # windows wholly inside the patch: Va = 0
    assert (p[10:18, 10:90] >= 0).mean() > 0.9


def test_sources_behind_and_out_of_frame_contribute_nothing(walls):
    sc, inv, plane, _, _ = walls["fronto"]
    poses, intr = sc["poses34"].copy(), sc["intrinsics"]
    poses = np.concatenate([poses, np.zeros((2, 12))])
    intr = np.concatenate([intr, intr[:2]])
    poses[4] = np.array([[-1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, -1, 0]]).reshape(12)       # looks the other way: w < 0 on every plane
    poses[5] = np.array([[1.0, 0, 0, -60.0], [0, 1, 0, 0], [0, 0, 1, 0]]).reshape(12)       # 60 to the side: wholly out of frame
    gray = np.concatenate([sc["gray"], sc["gray"][:2]])
    Hb = M.homographies(poses, intr, 0, [1, 4, 5], inv)
    qu, qv, ok = M.warp(Hb[1, 13], 72, 96)
    assert not ok.any() and (Hb[1, :, 8] < 0).all()
    assert not M.warp(Hb[2, 13], 72, 96)[2].any() and (Hb[2, :, 8] > 0).all()
    got = M.sweep_view(gray, 0, [1, 4, 5], Hb, inv, radius=3, min_sources=1, max_cost=0.5)
    Ha = M.homographies(poses, intr, 0, [1, -1, -1], inv)
    want = M.sweep_view(gray, 0, [1, -1, -1], Ha, inv, radius=3, min_sources=1, max_cost=0.5)
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    assert (got[0] >= 0).sum() > 4000
    none = M.sweep_view(gray, 0, [1, 4, 5], Hb, inv, radius=3, min_sources=2, max_cost=0.5)       # min_sources above what is there
    assert (none[0] == -1).all() and (none[1] == 0).all() and np.isinf(none[2]).all()


@pytest.fixture(scope="module")
def chain():
    sc, inv = M.wall_case("fronto")
    views = M.all_views(4, 3)
    out = M.dense_cloud(sc["poses34"], sc["intrinsics"], sc["gray"], sc["rgb"], views, np.tile(inv, (4, 1)), radius=3, min_sources=2, min_consistent=2,
                        max_cost=0.5, rel_tol=0.01)
    return sc, inv, views, out


def test_consistency_keeps_the_wall_and_rejects_a_shifted_map(chain):
    """On the true depth maps of the wall the check keeps every pixel that at least min_consistent sources see, and nothing of a map
    shifted by 3 rel_tol; on the swept maps it keeps more than nine in ten valid pixels."""
    sc, inv, views, out = chain
    valid = out["plane"] >= 0
    assert np.array_equal(out["counts"], out["mask"].reshape(4, -1).sum(1)) and not (out["mask"].astype(bool) & ~valid).any()
    assert out["mask"][0].sum() > 0.9 * valid[0].sum()
    truth = np.stack([M.true_depths(sc, v) for v in range(4)]).astype(np.float32)
    plane = np.zeros(truth.shape, np.int16)
    mask, counts = M.consistency(views, sc["poses34"], sc["intrinsics"], plane, truth, rel_tol=0.01, min_consistent=2)
    seen = np.zeros(truth.shape[1:], np.int64)
    for s in (1, 2, 3):
        u, v, z = M.project(sc["poses34"][s], sc["intrinsics"][s], M.lift(sc["poses34"][0], sc["intrinsics"][0], truth[0]))
        seen += (np.floor(u + 0.5) >= 0) & (np.floor(u + 0.5) <= 95) & (np.floor(v + 0.5) >= 0) & (np.floor(v + 0.5) <= 71)
    assert np.array_equal(mask[0], seen >= 2) and counts[0] == (seen >= 2).sum() > 6000
    shifted = truth.copy()
    shifted[0] = (truth[0].astype(np.float64) * (1.0 + 3 * 0.01)).astype(np.float32)
    mask, counts = M.consistency(views, sc["poses34"], sc["intrinsics"], plane, shifted, rel_tol=0.01, min_consistent=2)
    assert counts[0] == 0 and mask[0].sum() == 0
    plane[0, 10:20] = -1                                                    # invalid pixels are never kept
    mask, counts = M.consistency(views, sc["poses34"], sc["intrinsics"], plane, truth, rel_tol=0.01, min_consistent=2)
    assert mask[0, 10:20].sum() == 0 and mask[0, 20:30].sum() > 0


def test_fusion_order_capacity_and_distance_to_the_wall(chain):
    """Every fused vertex of the fronto-parallel scene lies within 0.05 of the wall z = 1 / inv[13] (measured: the worst is printed)."""
    sc, inv, views, out = chain
    v = out["vertices"]
    assert len(v) == out["written"] == out["total"] == int(out["mask"].sum())
    worst = float(np.abs(v["z"].astype(np.float64) - sc["d"]).max())
    print("fused vertices: %d, worst distance to the wall %.4f" % (len(v), worst))
    assert worst < 0.05
    ys, xs = np.nonzero(out["mask"][0])
    assert np.array_equal(v["red"][:len(xs)], out["rgb"][0, ys, xs, 0]) and (v["alpha"] == 255).all()
    half, (w, t) = M.fuse(views, sc["poses34"], sc["intrinsics"], out["rgb"], out["depth"], out["mask"], stride=2)
    assert t == int(out["mask"][:, ::2, ::2].sum()) == w == len(half)
    cut, (w, t) = M.fuse(views, sc["poses34"], sc["intrinsics"], out["rgb"], out["depth"], out["mask"], stride=1, capacity=1000)
    rows_sum = np.cumsum(out["mask"].reshape(-1, out["mask"].shape[2]).sum(1))
    assert t == out["total"] and w == rows_sum[rows_sum <= 1000].max() and np.array_equal(cut, v[:w]) and 900 < w <= 1000


def test_undistort_is_the_identity_without_distortion_and_moves_bytes_with_it():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 53, 3)).astype(np.uint8)
    K = np.array([61.3, 58.9, 25.7, 18.2, 0.0, 0.0])
    assert np.array_equal(M.undistort(img, K), img) and np.array_equal(M.undistort(img[..., 1], K), img[..., 1])
    K[4:] = 0.3, -0.1
    out = M.undistort(img, K)
    assert np.array_equal(out[..., 2], M.undistort(np.ascontiguousarray(img[..., 2]), K))
    assert (out != img).mean() > 0.5 and (out[-1, -1] == 0).all()           # the additive term pushes the lower right corner's sample outside: 0
    cy, cx = 18, 26
    assert np.abs(out[cy, cx].astype(int) - img[cy, cx].astype(int)).max() <= 3      # next to the principal point almost nothing moves


# ---- the library's pure-host entries -----------------------------------------------------------------------------------------------------

def test_host_entries_equal_the_contract_bit_for_bit():
    from reconstructor_amd import _lib, mvs
    sc, inv = M.wall_case("slanted")
    got = mvs.inv_depths(3.0, 8.0, 32)
    assert np.array_equal(got.view(np.uint64), inv.view(np.uint64))
    assert np.array_equal(mvs.inv_depths(2.0, 9.0, 1), M.inv_depths(2.0, 9.0, 1))
    for srcs, planes in (([1, 2, 3], inv), ([3, -1], inv[::-1].copy()), ([2], inv[5:6])):
        H = mvs.homographies(sc["poses34"], sc["intrinsics"], 0, srcs, planes)
        assert np.array_equal(H.view(np.uint64), M.homographies(sc["poses34"], sc["intrinsics"], 0, srcs, planes).view(np.uint64))
    for bad in (lambda: mvs.inv_depths(0.0, 1.0, 4), lambda: mvs.inv_depths(1.0, 2.0, 1025), lambda: mvs.inv_depths(1.0, 2.0, 0),
                lambda: mvs.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 0], inv), lambda: mvs.homographies(sc["poses34"], sc["intrinsics"], 0, [1] * 17, inv),
                lambda: mvs.layout(72, 96, 4, 32, 3, radius=6), lambda: mvs.layout(72, 96, 4, 1025, 3), lambda: mvs.layout(0, 96, 4, 32, 3)):
        with pytest.raises(_lib.RcnError):
            bad()
    z = mvs.layout(72, 96, 4, 32, 3)
    assert (z["tile"], z["tiles_x"], z["tiles_y"]) == (16, 6, 5) and z["pixels"] == 4 * 72 * 96 and z["h_doubles"] == 4 * 3 * 32 * 9 and z["samples"] == z["pixels"] * 96
    assert z["lds_bytes"] == 16640
    o = mvs.options()
    assert (o.radius, o.min_sources, o.min_consistent, o.stride, o.max_cost, o.rel_tol) == tuple(M.DEFAULTS[k] for k in ("radius", "min_sources", "min_consistent", "stride", "max_cost", "rel_tol"))


def test_golden_file_matches():
    g = np.load(GOLDEN)
    names = sorted({k.split(".")[0] for k in g.files})
    assert len(names) >= 3
    for n in names:
        opt = dict(zip(("radius", "min_sources", "min_consistent", "stride"), (int(v) for v in g[n + ".iopt"])))
        opt.update(zip(("max_cost", "rel_tol"), (float(v) for v in g[n + ".fopt"])))
        cap = int(g[n + ".capacity"])
        out = M.dense_cloud(g[n + ".poses34"], g[n + ".intrinsics"], g[n + ".gray"], g[n + ".rgb"], g[n + ".views"], g[n + ".inv"], capacity=None if cap < 0 else cap, **opt)
        for k in ("plane", "depth", "cost", "mask", "counts", "vertices"):
            assert np.array_equal(np.ascontiguousarray(out[k]).view(np.uint8), np.ascontiguousarray(g[n + "." + k]).view(np.uint8)), (n, k)
        assert (out["written"], out["total"]) == tuple(int(v) for v in g[n + ".fused"]), n
