"""GPU suite: the stages around the plane sweep (csrc/mvs.hip) against the contract tests/mvs_ref.py -- the undistortion resample, the
views and depth ranges of a BA session, the consistency check, the fusion with capacities and strides, reconstructor_amd.mvs.dense_cloud
end to end, and the argument errors.  Every comparison is an equality of bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvs_ref as M

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.as_tensor(np.array(a)).cuda()


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_undistort_identity_contract_channels_and_strides(gpu_ctx):
    import torch
    from reconstructor_amd import mvs
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (3, 37, 53, 3)).astype(np.uint8)
    K = np.array([[61.3, 58.9, 25.7, 18.2, 0.0, 0.0], [61.3, 58.9, 25.7, 18.2, 0.3, -0.1], [40.0, 45.0, 30.1, 10.4, -0.2, 0.05]])
    got3 = mvs.undistort(gpu_ctx, _t(img), K).cpu().numpy()
    got1 = mvs.undistort(gpu_ctx, _t(img[..., 1]), K).cpu().numpy()
    assert np.array_equal(got3[0], img[0]) and np.array_equal(got1[0], img[0, ..., 1])          # k1 = k2 = 0: the identity on every byte
    for i in range(3):
        assert np.array_equal(got3[i], M.undistort(img[i], K[i])) and np.array_equal(got1[i], M.undistort(np.ascontiguousarray(img[i, ..., 1]), K[i]))
    assert (got3[1] != img[1]).mean() > 0.5
    buf = torch.full((3, 40, 53 * 3 + 7), 9, dtype=torch.uint8, device="cuda")                     # padded rows and images, guard words behind the output
    src = buf[:, 1:38, :159].unflatten(2, (53, 3))
    src.copy_(_t(img))
    out = torch.full((3 * 37 * 53 * 3 + 64,), 171, dtype=torch.uint8, device="cuda")
    Kd = _t(K)
    gpu_ctx.check(gpu_ctx.lib.rcn_img_undistort_device(gpu_ctx.h, C.c_void_p(src.data_ptr()), src.stride(0), src.stride(1), 3, 3, 37, 53, C.c_void_p(Kd.data_ptr()),
                                                       C.c_void_p(out.data_ptr())))
    gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
    o = out.cpu().numpy()
    assert np.array_equal(o[:-64].reshape(3, 37, 53, 3), got3) and (o[-64:] == 171).all()


def test_session_views_against_a_numpy_count(gpu_ctx):
    from reconstructor_amd import ba, mvs, synth_ba
    sc = synth_ba.make_scene(9, 500, obs_per_point=4, seed=32)
    ses = ba.BaSession(gpu_ctx)
    try:
        for p, k in zip(sc["poses"], sc["intrinsics"]):
            ses.add_camera(p, k)
        ses.add_camera(sc["poses"][0], sc["intrinsics"][0])                 # camera 9: no landmark at all
        pts = np.concatenate([sc["points"], [[0.0, 0.0, 500.0]]])           # one landmark far behind some of its cameras
        ses.add_points(pts)
        obs_pt = np.concatenate([sc["obs_pt"], [500, 500, 500, 2, 2]]).astype(np.int32)      # and a landmark seen twice by one camera
        obs_cam = np.concatenate([sc["obs_cam"], [0, 4, 8, int(sc["obs_cam"][sc["obs_pt"] == 2][0]), 3]]).astype(np.int32)
        order = np.argsort(obs_pt, kind="stable")
        ses.add_observations(obs_pt[order], obs_cam[order], np.zeros((len(obs_pt), 2), np.int32))
        P34 = ba.poses34_from_angle_axis(ses.cameras()[0])
        z500 = [((P34[c][8] * 0 + P34[c][9] * 0) + P34[c][10] * 500.0) + P34[c][11] for c in (0, 4, 8)]
        assert min(z500) < 0 < max(z500)
        for S in (1, 4, 16):
            want = M.session_views(10, obs_pt, obs_cam, pts, P34, S)
            got = mvs.session_views(ses, S, P34, want_counts=True)
            for g, w in zip(got, want):
                assert _bytes_equal(g, w)
            assert (got[0][9] == -1).all() and got[1][9].tolist() == [0.0, 0.0] and (got[1][:9, 0] > 0).all()
        assert np.array_equal(mvs.session_views(ses, 3)[0], M.session_views(10, obs_pt, obs_cam, pts, P34, 3)[0])      # poses34 from the session
        for cam in (0, 5):                                                  # the rule of rcn_ba_session_covisible
            near, counts = ses.covisible(cam, 4)
            assert np.array_equal(near, got[0][cam][:4][got[0][cam][:4] >= 0]) and np.array_equal(counts, got[2][cam])
    finally:
        ses.close()


@functools.lru_cache(maxsize=None)
def chain_ref(stride=1, capacity=None):
    sc, inv = M.wall_case("fronto")
    views = M.all_views(4, 3)
    out = M.dense_cloud(sc["poses34"], sc["intrinsics"], sc["gray"], sc["rgb"], views, np.tile(inv, (4, 1)), capacity=capacity, radius=3, min_sources=2,
                        min_consistent=2, max_cost=0.5, rel_tol=0.01, stride=stride)
    return sc, inv, views, out


def test_consistency_and_fusion_with_capacities_and_strides(gpu_ctx):
    import torch
    from reconstructor_amd import mvs
    sc, inv, views, ref = chain_ref()
    plane, depth = _t(ref["plane"]), _t(ref["depth"])
    for tol, mc in ((0.01, 2), (0.0005, 1), (0.01, 4), (0.01, 0)):
        mask, counts = mvs.consistency(gpu_ctx, views, sc["poses34"], sc["intrinsics"], plane, depth, mvs.options(rel_tol=tol, min_consistent=mc))
        wm, wc = M.consistency(views, sc["poses34"], sc["intrinsics"], ref["plane"], ref["depth"], rel_tol=tol, min_consistent=mc)
        assert _bytes_equal(mask.cpu().numpy(), wm) and _bytes_equal(counts.cpu().numpy(), wc), (tol, mc)
        if mc == 4:
            assert wc.sum() == 0                                            # more than the three sources there are
        if mc == 0:
            assert np.array_equal(wm.astype(bool), ref["plane"] >= 0)
    shifted = ref["depth"].copy()
    shifted[0] = (shifted[0].astype(np.float64) * 1.03).astype(np.float32)
    mask, counts = mvs.consistency(gpu_ctx, views, sc["poses34"], sc["intrinsics"], plane, _t(shifted), mvs.options(rel_tol=0.01, min_consistent=2))
    wm, wc = M.consistency(views, sc["poses34"], sc["intrinsics"], ref["plane"], shifted, rel_tol=0.01, min_consistent=2)
    assert _bytes_equal(mask.cpu().numpy(), wm) and wc[0] < 0.01 * ref["counts"][0]
    # a subset of the views: sources outside the batch agree with nothing
    sub = views[[0, 2]]
    mask, counts = mvs.consistency(gpu_ctx, sub, sc["poses34"], sc["intrinsics"], plane[[0, 2]].contiguous(), depth[[0, 2]].contiguous(), mvs.options(min_consistent=1))
    wm, wc = M.consistency(sub, sc["poses34"], sc["intrinsics"], ref["plane"][[0, 2]], ref["depth"][[0, 2]], min_consistent=1)
    assert _bytes_equal(mask.cpu().numpy(), wm) and _bytes_equal(counts.cpu().numpy(), wc) and wc.min() > 0

    rgb, mask = _t(ref["rgb"]), _t(ref["mask"])
    total = int(ref["mask"].sum())
    rows = np.cumsum(ref["mask"].reshape(-1, 96).sum(1))
    for stride, cap in ((1, None), (2, None), (3, None), (1, 1000), (1, 0), (1, total - 1), (1, total), (2, 777), (1, int(rows[0]))):
        want, (ww, wt) = M.fuse(views, sc["poses34"], sc["intrinsics"], ref["rgb"], ref["depth"], ref["mask"], stride=stride, capacity=cap)
        room = (cap if cap is not None else wt) + 16
        out = torch.full((room, 16), 205, dtype=torch.uint8, device="cuda")          # guard records behind the capacity
        cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        P, K = _t(sc["poses34"]), _t(sc["intrinsics"])
        o = mvs.options(stride=stride)
        gpu_ctx.check(gpu_ctx.lib.rcn_mvs_fuse_device(gpu_ctx.h, views.ctypes.data, 4, 3, C.c_void_p(P.data_ptr()), C.c_void_p(K.data_ptr()), 4, C.c_void_p(rgb.data_ptr()),
                                                      72, 96, C.c_void_p(depth.data_ptr()), C.c_void_p(mask.data_ptr()), C.byref(o), room - 16,
                                                      C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())))
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        assert cnt.cpu().tolist() == [ww, wt, -1], (stride, cap)
        got = out.cpu().numpy()
        assert _bytes_equal(got[:ww].reshape(-1).view(M.VERTEX_DTYPE), want) and (got[ww:] == 205).all(), (stride, cap)
    black, _ = mvs.fuse(gpu_ctx, views, sc["poses34"], sc["intrinsics"], None, depth, mask)
    want, _ = M.fuse(views, sc["poses34"], sc["intrinsics"], None, ref["depth"], ref["mask"])
    assert _bytes_equal(black, want)


def test_dense_cloud_end_to_end(gpu_ctx, tmp_path):
    """mvs.dense_cloud on the ray-cast wall gives the contract's vertices byte for byte; every vertex lies within 0.05 of the wall (the
    contract itself reaches 0.0453 on the CPU, tests/test_mvs_ref.py)."""
    from reconstructor_amd import mvs
    sc, inv, views, ref = chain_ref()
    path = str(tmp_path / "dense.ply")
    out = mvs.dense_cloud((gpu_ctx, sc["poses34"], sc["intrinsics"]), _t(sc["gray"]), _t(sc["rgb"]), views, np.tile(inv, (4, 1)),
                          opt=mvs.options(radius=3, min_sources=2, min_consistent=2, max_cost=0.5, rel_tol=0.01), path=path)
    for k in ("plane", "depth", "cost", "mask", "counts"):
        assert _bytes_equal(out[k].cpu().numpy(), ref[k]), k
    assert _bytes_equal(out["vertices"], ref["vertices"]) and (out["written"], out["total"]) == (ref["written"], ref["total"])
    worst = float(np.abs(out["vertices"]["z"].astype(np.float64) - sc["d"]).max())
    print("dense cloud: %d vertices, worst distance to the wall %.4f" % (len(out["vertices"]), worst))
    assert len(out["vertices"]) > 15000 and worst < 0.05
    with open(path, "rb") as f:
        blob = f.read()
    assert blob.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(out["vertices"])) and blob.endswith(out["vertices"].tobytes())
    # with distortion in the cameras the chain undistorts first
    K = sc["intrinsics"].copy()
    K[:, 4:] = 0.05, -0.01
    want = M.dense_cloud(sc["poses34"], K, sc["gray"][:, :40, :56], sc["rgb"][:, :40, :56], views[:2], np.tile(inv[8:20], (2, 1)), radius=2, min_sources=1,
                         min_consistent=1, stride=2)
    got = mvs.dense_cloud((gpu_ctx, sc["poses34"], K), _t(sc["gray"][:, :40, :56]), _t(sc["rgb"][:, :40, :56]), views[:2], np.tile(inv[8:20], (2, 1)),
                          opt=mvs.options(radius=2, min_sources=1, min_consistent=1, stride=2))
    assert _bytes_equal(got["vertices"], want["vertices"]) and _bytes_equal(got["plane"].cpu().numpy(), want["plane"])


def test_dense_cloud_from_a_session(gpu_ctx):
    """The session supplies cameras, sources and ranges: the same cloud as the contract run on what session_views returned."""
    from reconstructor_amd import ba, mvs, synth_ba
    sc, inv, views, ref = chain_ref()
    ses = ba.BaSession(gpu_ctx)
    try:
        for i in range(4):
            R = sc["poses34"][i].reshape(3, 4)
            ses.add_camera(np.concatenate([synth_ba.rot_to_angle_axis(R[:, :3]), R[:, 3]]), sc["intrinsics"][i])
        rng = np.random.default_rng(9)
        pts = np.c_[rng.uniform(-1.5, 1.5, 60), rng.uniform(-1, 1, 60), np.full(60, sc["d"])]
        ses.add_points(pts)
        ses.add_observations(np.repeat(np.arange(60), 4), np.tile(np.arange(4), 60), np.zeros((240, 2), np.int32))
        P34 = ba.poses34_from_angle_axis(ses.cameras()[0])
        out = mvs.dense_cloud(ses, _t(sc["gray"]), _t(sc["rgb"]), S=3, D=16, widen=1.4, opt=mvs.options(radius=3))
        src, rng_, _ = M.session_views(4, np.repeat(np.arange(60), 4), np.tile(np.arange(4), 60), pts, P34, 3)
        assert np.array_equal(out["views"], np.c_[np.arange(4), src]) and (rng_[:, 0] > 0).all()
        assert _bytes_equal(out["inv"], np.stack([M.inv_depths(r[0] / 1.4, r[1] * 1.4, 16) for r in rng_]))
        want = M.dense_cloud(P34, sc["intrinsics"], sc["gray"], sc["rgb"], out["views"], out["inv"], radius=3)
        assert _bytes_equal(out["vertices"], want["vertices"]) and len(want["vertices"]) > 5000
        assert np.abs(out["vertices"]["z"] - sc["d"]).max() < 0.1
    finally:
        ses.close()


def test_argument_errors(gpu_ctx):
    import torch
    from reconstructor_amd import _lib, mvs
    sc, inv, views, ref = chain_ref()
    g, rgb = _t(sc["gray"]), _t(sc["rgb"])
    invs = np.tile(inv, (4, 1))
    H = M.view_homographies(sc["poses34"], sc["intrinsics"], views, invs)
    plane, depth, mask = _t(ref["plane"]), _t(ref["depth"]), _t(ref["mask"])
    own = views.copy()
    own[2, 2] = 2
    far = views.copy()
    far[1, 1] = 4
    wide = np.full((4, 18), -1, np.int32)                                   # S = 17
    wide[:, 0] = np.arange(4)
    bad = [lambda: mvs.sweep(gpu_ctx, g, views, H, invs, mvs.options(radius=0)), lambda: mvs.sweep(gpu_ctx, g, views, H, invs, mvs.options(radius=6)),
           lambda: mvs.sweep(gpu_ctx, g, own, H, invs), lambda: mvs.sweep(gpu_ctx, g, far, H, invs), lambda: mvs.sweep(gpu_ctx, g, views, H, invs, mvs.options(min_sources=0)),
           lambda: mvs.sweep(gpu_ctx, g, wide, np.zeros((4, 17, 32, 9)), invs),
           lambda: mvs.sweep(gpu_ctx, g, views, np.zeros((4, 3, 1025, 9)), np.zeros((4, 1025))),
           lambda: mvs.sweep(gpu_ctx, g, views, H, invs, mvs.options(max_cost=float("nan"))),
           lambda: mvs.consistency(gpu_ctx, own, sc["poses34"], sc["intrinsics"], plane, depth), lambda: mvs.consistency(gpu_ctx, views, sc["poses34"], sc["intrinsics"], plane, depth, mvs.options(rel_tol=-1.0)),
           lambda: mvs.fuse(gpu_ctx, views, sc["poses34"], sc["intrinsics"], rgb, depth, mask, mvs.options(stride=0)),
           lambda: mvs.fuse(gpu_ctx, views, sc["poses34"], sc["intrinsics"], rgb, depth, mask, capacity=-1)]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.RcnError) as e:
            f()
        assert e.value.code == -1 and len(str(e.value)) > 25, (i, str(e.value))
    lib, h = gpu_ctx.lib, gpu_ctx.h
    o = mvs.options()
    Hd, invd = _t(H), _t(invs)
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.zeros(4 * 72 * 96, dtype=torch.float32, device="cuda")
    assert lib.rcn_mvs_sweep_device(h, None, 72 * 96, 96, 4, 72, 96, views.ctypes.data, 4, 3, p(Hd), p(invd), 32, C.byref(o), p(plane), p(out), p(out)) == -1
    assert lib.rcn_mvs_sweep_device(h, p(g), 72 * 96, 96, 4, 72, 96, views.ctypes.data, 4, 3, p(Hd), p(invd), 32, C.byref(o), None, p(out), p(out)) == -1
    assert lib.rcn_mvs_sweep_device(h, p(g), 72 * 96, 95, 4, 72, 96, views.ctypes.data, 4, 3, p(Hd), p(invd), 32, C.byref(o), p(plane), p(out), p(out)) == -1
    assert lib.rcn_mvs_sweep_device(h, p(g), 72 * 96, 96, 4, 0, 96, views.ctypes.data, 4, 3, p(Hd), p(invd), 32, C.byref(o), p(plane), p(out), p(out)) == -1
    assert lib.rcn_mvs_sweep_device(h, p(g), 72 * 96, 96, 4, 72, 96, views.ctypes.data, -1, 3, p(Hd), p(invd), 32, C.byref(o), p(plane), p(out), p(out)) == -1
    assert lib.rcn_mvs_sweep_device(h, p(g), 72 * 96, 96, 4, 1 << 15, 1 << 15, views.ctypes.data, 4, 3, p(Hd), p(invd), 32, C.byref(o), p(plane), p(out), p(out)) == -1
    assert b"rows * cols" in lib.rcn_last_error(h)
    assert lib.rcn_img_undistort_device(h, p(g), 72 * 96, 96, 2, 4, 72, 96, p(invd), p(out)) == -1 and lib.rcn_img_undistort_device(h, p(g), 72 * 96, 96, 1, 4, 72, 96, None, p(out)) == -1
    # zero views launch nothing and touch nothing
    out.fill_(3.0)
    assert lib.rcn_mvs_sweep_device(h, None, 0, 96, 4, 72, 96, None, 0, 3, None, None, 32, None, None, None, None) == 0
    assert lib.rcn_mvs_consistency_device(h, None, 0, 3, None, None, 4, 72, 96, None, None, None, None, None) == 0
    assert lib.rcn_img_undistort_device(h, None, 0, 96, 1, 0, 72, 96, None, None) == 0
    cnt = torch.full((2,), 5, dtype=torch.int64, device="cuda")
    assert lib.rcn_mvs_fuse_device(h, None, 0, 3, None, None, 4, None, 72, 96, None, None, None, 10, None, p(cnt)) == 0
    gpu_ctx.check(lib.rcn_synchronize(h))
    assert cnt.cpu().tolist() == [0, 0] and (out == 3.0).all().item()
    # the context still works
    same = mvs.sweep(gpu_ctx, g, views[:1], H[:1], invs[:1], mvs.options(radius=3))
    und = ref["gray"]
    assert np.array_equal(und, sc["gray"]) and _bytes_equal(same[0].cpu().numpy(), ref["plane"][:1])
