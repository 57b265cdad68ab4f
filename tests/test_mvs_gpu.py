"""GPU suite: the plane sweep on the device (rcn_mvs_sweep_device, csrc/mvs.hip k_mvs_sweep) against the contract tests/mvs_ref.py.  Every
check is an equality of bits: plane int16, depth float32, cost float32 of every pixel, with guard words behind each output."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvs_ref as M

pytestmark = pytest.mark.gpu

GUARD = 64                       # elements behind every output, filled with a pattern the kernel must leave alone
SHAPES = [(24, 40), (17, 33), (72, 96), (9, 12)]      # rows x cols: no multiple of the 16-pixel tile in either axis; 9 x 12 is smaller than one tile + halo


def run_sweep(ctx, gray, views, H, inv, **opt):
    """rcn_mvs_sweep_device into guarded outputs; gray a numpy array [n][rows][cols] or a CUDA tensor (dense last dimension)."""
    import torch
    from reconstructor_amd import mvs
    g = torch.as_tensor(np.array(gray)).cuda() if isinstance(gray, np.ndarray) else gray
    n, rows, cols = g.shape
    views = np.ascontiguousarray(views, np.int32)
    V, S = views.shape[0], views.shape[1] - 1
    inv = np.ascontiguousarray(inv, np.float64).reshape(V, -1)
    D = inv.shape[1]
    Hd, invd = torch.as_tensor(np.array(H, np.float64)).cuda(), torch.as_tensor(np.array(inv)).cuda()
    npx = V * rows * cols
    plane = torch.full((npx + GUARD,), -12345, dtype=torch.int16, device="cuda")
    depth = torch.full((npx + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    cost = torch.full((npx + GUARD,), -7.5, dtype=torch.float32, device="cuda")
    o = mvs.options(**opt)
    torch.cuda.synchronize()
    ctx.check(ctx.lib.rcn_mvs_sweep_device(ctx.h, C.c_void_p(g.data_ptr()), g.stride(0), g.stride(1), n, rows, cols, views.ctypes.data, V, S,
                                           C.c_void_p(Hd.data_ptr()), C.c_void_p(invd.data_ptr()), D, C.byref(o), C.c_void_p(plane.data_ptr()),
                                           C.c_void_p(depth.data_ptr()), C.c_void_p(cost.data_ptr())))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    p, d, c = plane.cpu().numpy(), depth.cpu().numpy(), cost.cpu().numpy()
    assert (p[npx:] == -12345).all() and (d[npx:] == -7.5).all() and (c[npx:] == -7.5).all(), "a guard word was written"
    return p[:npx].reshape(V, rows, cols), d[:npx].reshape(V, rows, cols), c[:npx].reshape(V, rows, cols)


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("plane", "depth", "cost")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.nonzero(np.ascontiguousarray(g).view(np.uint8).reshape(-1) != np.ascontiguousarray(w).view(np.uint8).reshape(-1))[0]
        assert len(bad) == 0, "%s %s: %d bytes differ, the first at %d" % (what, name, len(bad), bad[0])


@functools.lru_cache(maxsize=None)
def shape_case(rows, cols):
    """Five views of rows x cols and a batch of three reference views with 3, 2 and 1 sources (-1 padding in every position)."""
    sc, _ = M.small_case(rows, cols, n=5, seed=rows + cols)
    views = np.array([[0, 1, 2, 3], [1, 2, -1, 0], [2, -1, -1, 4]], np.int32)
    for a in (sc["gray"], sc["poses34"], sc["intrinsics"], views):
        a.setflags(write=False)
    return sc, views


@functools.lru_cache(maxsize=None)
def shape_ref(rows, cols, R, D, min_sources=1, max_cost=0.5):
    """The contract's answer, computed once per case and shared."""
    sc, views = shape_case(rows, cols)
    base = M.inv_depths(3.0, 8.0, D)
    ties = np.repeat(base, 2)[:D] if D > 1 else base          # view 2: every plane twice (exact ties), as far as D reaches
    inv = np.stack([base, base[::-1], ties])
    H = M.view_homographies(sc["poses34"], sc["intrinsics"], views, inv)
    want = M.sweep(sc["gray"], views, H, inv, radius=R, min_sources=min_sources, max_cost=max_cost)
    for a in (inv, H) + want:
        a.setflags(write=False)
    return inv, H, want


@pytest.mark.parametrize("R", [1, 3, 5])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes_radii_and_plane_counts(gpu_ctx, rows, cols, R):
    """D = 1, 2, 3: the parabola has no, one, two neighbours; D = 32: the full list.  Ascending, descending and repeated lists in one batch."""
    sc, views = shape_case(rows, cols)
    valid = 0
    for D in (1, 2, 3, 32):
        inv, H, want = shape_ref(rows, cols, R, D)
        got = run_sweep(gpu_ctx, sc["gray"], views, H, inv, radius=R, min_sources=1, max_cost=0.5)
        same(got, want, "%dx%d R=%d D=%d" % (cols, rows, R, D))
        valid += int((want[0] >= 0).sum())
    if rows > 2 * R and cols > 2 * R:
        assert valid > 0
    else:
        assert valid == 0                                     # no window fits: everything invalid, nothing out of bounds


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_source_counts_padding_and_min_sources(gpu_ctx, S):
    sc, _ = shape_case(24, 40)
    inv = M.inv_depths(3.0, 8.0, 6)[None]
    order = [3, 1, 4, 2][:S]
    for pad in range(S):                                      # the same list with one slot emptied
        srcs = list(order)
        if S > 1:
            srcs[pad] = -1
        views = np.array([[0] + srcs], np.int32)
        H = M.view_homographies(sc["poses34"], sc["intrinsics"], views, inv)
        there = sum(s >= 0 for s in srcs)
        for ms in sorted({1, there, there + 1}):
            want = M.sweep(sc["gray"], views, H, inv, radius=2, min_sources=ms, max_cost=0.5)
            same(run_sweep(gpu_ctx, sc["gray"], views, H, inv, radius=2, min_sources=ms, max_cost=0.5), want, "S=%d pad=%d min_sources=%d" % (S, pad, ms))
            if ms > there:
                assert (want[0] == -1).all()                  # min_sources above the number available
        if S == 1:
            break


def test_a_view_does_not_depend_on_its_batch_and_runs_repeat(gpu_ctx):
    sc, views = shape_case(72, 96)
    inv, H, want = shape_ref(72, 96, 3, 32)
    batch = run_sweep(gpu_ctx, sc["gray"], views, H, inv, radius=3, min_sources=1, max_cost=0.5)
    same(batch, want)
    same(run_sweep(gpu_ctx, sc["gray"], views, H, inv, radius=3, min_sources=1, max_cost=0.5), batch, "second run")
    for v in range(3):
        one = run_sweep(gpu_ctx, sc["gray"], views[v:v + 1], H[v:v + 1], inv[v:v + 1], radius=3, min_sources=1, max_cost=0.5)
        same(one, tuple(a[v:v + 1] for a in batch), "view %d alone" % v)
    flipped = run_sweep(gpu_ctx, sc["gray"], views[::-1], H[::-1], inv[::-1], radius=3, min_sources=1, max_cost=0.5)
    same(flipped, tuple(a[::-1] for a in batch), "the batch reversed")


def test_padded_strides(gpu_ctx):
    import torch
    sc, views = shape_case(17, 33)
    inv, H, want = shape_ref(17, 33, 3, 3)
    buf = torch.full((5, 17 + 3, 33 + 11), 255, dtype=torch.uint8, device="cuda")
    g = buf[:, 2:19, 5:38]
    g.copy_(torch.as_tensor(np.array(sc["gray"])).cuda())
    assert g.stride() == (20 * 44, 44, 1)
    same(run_sweep(gpu_ctx, g, views, H, inv, radius=3, min_sources=1, max_cost=0.5), want)


@functools.lru_cache(maxsize=None)
def wall():
    sc, inv = M.wall_case("fronto")
    H = M.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 2, 3], inv)
    want = M.sweep_view(sc["gray"], 0, [1, 2, 3], H, inv, radius=3, min_sources=2, max_cost=0.5)
    return sc, inv, H, want


def test_the_wall_planted_ties_and_a_textureless_patch(gpu_ctx):
    sc, inv, H, want = wall()
    views = np.array([[0, 1, 2, 3]], np.int32)
    got = run_sweep(gpu_ctx, sc["gray"], views, H[None], inv[None], radius=3, min_sources=2, max_cost=0.5)
    same(got, tuple(a[None] for a in want))
    ok = got[0][0] >= 0
    assert (got[0][0][ok] == 13).mean() >= 0.96                # the wall on its plane (tests/test_mvs_ref.py states the measured share)
    twice = np.repeat(inv[10:17], 2)
    H2 = M.homographies(sc["poses34"], sc["intrinsics"], 0, [1, 2, 3], twice)
    want2 = M.sweep_view(sc["gray"], 0, [1, 2, 3], H2, twice, radius=3, min_sources=2, max_cost=0.5)
    got2 = run_sweep(gpu_ctx, sc["gray"], views, H2[None], twice[None], radius=3, min_sources=2, max_cost=0.5)
    same(got2, tuple(a[None] for a in want2), "ties")
    assert (got2[0][got2[0] >= 0] % 2 == 0).all() and (got2[0] >= 0).sum() > 5000
    gray = sc["gray"].copy()
    gray[0, 20:40, 30:60] = 77
    want3 = M.sweep_view(gray, 0, [1, 2, 3], H, inv, radius=3, min_sources=2, max_cost=0.5)
    got3 = run_sweep(gpu_ctx, gray, views, H[None], inv[None], radius=3, min_sources=2, max_cost=0.5)
    same(got3, tuple(a[None] for a in want3), "textureless")
    assert (got3[0][0, 23:37, 33:57] == -1).all() and np.isinf(got3[2][0, 23:37, 33:57]).all()


def test_sources_behind_and_out_of_frame(gpu_ctx):
    sc, inv, _, _ = wall()
    poses = np.concatenate([sc["poses34"], np.zeros((2, 12))])
    intr = np.concatenate([sc["intrinsics"], sc["intrinsics"][:2]])
    poses[4] = np.array([[-1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, -1, 0]]).reshape(12)
    poses[5] = np.array([[1.0, 0, 0, -60.0], [0, 1, 0, 0], [0, 0, 1, 0]]).reshape(12)
    gray = np.concatenate([sc["gray"], sc["gray"][:2]])
    views = np.array([[0, 1, 4, 5], [0, 1, -1, -1], [0, 4, 5, -1]], np.int32)
    invs = np.tile(inv, (3, 1))
    H = M.view_homographies(poses, intr, views, invs)
    want = M.sweep(gray, views, H, invs, radius=3, min_sources=1, max_cost=0.5)
    got = run_sweep(gpu_ctx, gray, views, H, invs, radius=3, min_sources=1, max_cost=0.5)
    same(got, want)
    same(tuple(a[0:1] for a in got), tuple(a[1:2] for a in got), "the two dead sources contribute nothing")
    assert (got[0][0] >= 0).sum() > 4000 and (got[0][2] == -1).all() and (got[1][2] == 0).all() and np.isinf(got[2][2]).all()


def test_max_cost_cuts_exactly_at_a_pixels_cost(gpu_ctx):
    sc, inv, H, want = wall()
    vol = M.cost_volume(sc["gray"], 0, [1, 2, 3], H, 3, 2)
    best = vol.min(0)
    y, x = 36, 48
    assert want[0][y, x] >= 0 and np.isfinite(best[y, x])
    views = np.array([[0, 1, 2, 3]], np.int32)
    for cut, stays in ((best[y, x], True), (np.nextafter(best[y, x], -np.inf), False)):
        w = M.sweep_view(sc["gray"], 0, [1, 2, 3], H, inv, radius=3, min_sources=2, max_cost=float(cut))
        g = run_sweep(gpu_ctx, sc["gray"], views, H[None], inv[None], radius=3, min_sources=2, max_cost=float(cut))
        same(g, tuple(a[None] for a in w), "max_cost %r" % cut)
        assert (g[0][0, y, x] >= 0) == stays
    inf = run_sweep(gpu_ctx, sc["gray"], views, H[None], inv[None], radius=3, min_sources=2, max_cost=float("inf"))
    same(inf, tuple(a[None] for a in M.sweep_view(sc["gray"], 0, [1, 2, 3], H, inv, radius=3, min_sources=2, max_cost=np.inf)), "no cut")
