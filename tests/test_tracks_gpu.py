"""GPU suite: track building on the device (rcn_tracks_*, csrc/tracks.hip) against the contract tests/tracks_ref.py, every output array
bit for bit: degenerate input, track lengths at the sort's boundaries (one wavefront, the workgroup path and its edges), contended
unions under shuffled entry orders, a giant component under both conflict policies, planted conflicts, selection, both length
limits, capacities with guard words, feat_track and the statistics, the chain into rcn_triangulate_device, repeatability, the
argument errors.  tests/test_tracks_ref.py checks that every scene has the property it is named for."""
import ctypes as C

import numpy as np
import pytest

import tracks_ref as T
from reconstructor_amd import _lib, nextview, synth_ba, tracks
from reconstructor_amd import triangulate as tri

pytestmark = pytest.mark.gpu
PAD = 5
_REF = {}


@pytest.fixture(autouse=True, scope="module")
def _leave_the_ctx_clean(gpu_ctx):
    yield
    nextview.clear_lists(gpu_ctx)
    gpu_ctx.check(gpu_ctx.lib.rcn_coords_clear(gpu_ctx.h))


def ref_of(name, fm, K, coords, **kw):
    """The contract's answer, computed once per (scene, options) and shared."""
    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        _REF[key] = T.build(*T.lists_of(fm), K, coords=coords, **kw)
    return _REF[key]


def put(ctx, fm, K, coords, mirror=False):
    ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
    for i in K:
        a = np.ascontiguousarray(coords[i], np.int32).reshape(-1, 2)
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, int(i), a.ctypes.data if len(a) else None, len(a)))
    nextview.upload_lists(ctx, *T.lists_of(fm), mirror=mirror)


def run(ctx, cap_t, cap_o, **kw):
    opt = tracks.options(**{k: kw[k] for k in ("min_length", "max_length", "conflict") if k in kw})
    out = tracks.build_device(ctx, cap_t, cap_o, options=opt, select=kw.get("select"), pad=PAD)
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def assert_equals_contract(got, ref, cap_t, cap_o):
    want = T.truncate(ref, cap_t, cap_o)
    end = len(want["obs_img"])
    guard = lambda a, n: a.shape[0] == n + PAD and (a[n:] == -7).all()
    assert guard(got["counts"], 2) and np.array_equal(got["counts"][:2], ref["counts"])          # the full result's, whatever the capacities
    assert guard(got["trk_off"], cap_t + 1) and np.array_equal(got["trk_off"][:cap_t + 1], want["trk_off"])
    for k in ("obs_img", "obs_feat", "obs_cam"):
        if want[k] is None:
            assert got[k] is None
            continue
        assert guard(got[k], cap_o) and np.array_equal(got[k][:end], want[k]) and (got[k][end:] == -7).all(), k
    assert guard(got["obs_xy"], 2 * cap_o) and np.array_equal(got["obs_xy"][:2 * end].reshape(-1, 2), want["obs_xy"]) and (got["obs_xy"][2 * end:] == -7).all()
    n = len(ref["feat_track"])
    assert guard(got["feat_track"], n) and np.array_equal(got["feat_track"][:n], want["feat_track"])
    assert guard(got["stats"], 8) and np.array_equal(got["stats"][:8], ref["stats"])
    return want


def check(ctx, name, fm, K, upload=None, caps=None, **kw):
    coords = T.coords_of(K)
    ref = ref_of(name, fm, K, coords, **kw)
    put(ctx, upload if upload is not None else fm, K, coords)
    cap_t, cap_o = caps if caps is not None else (int(ref["counts"][0]), int(ref["counts"][1]))
    return assert_equals_contract(run(ctx, cap_t, cap_o, **kw), ref, cap_t, cap_o), ref


def test_layout_and_degenerate_input(gpu_ctx):
    fm, K = T.scene_degenerate()                              # images with K = 0, empty lists, a feature matched nowhere
    want, ref = check(gpu_ctx, "degenerate", fm, K)
    assert want["tracks"] == [[(1, 0), (2, 1)]]
    ids, off = tracks.layout(gpu_ctx)
    assert np.array_equal(ids, ref["img_ids"]) and np.array_equal(off, ref["node_off"])
    fm, K = {(4, 9): []}, {4: 3, 9: 0}                        # one pair with an empty list
    want, _ = check(gpu_ctx, "one_empty", fm, K, caps=(2, 3))
    assert want["written"] == 0
    put(gpu_ctx, {}, {}, {})                                  # no pairs at all
    got = run(gpu_ctx, 1, 1)
    assert got["counts"][:2].tolist() == [0, 0] and got["trk_off"][:2].tolist() == [0, 0] and got["stats"][:8].tolist() == [0] * 8
    assert (got["obs_img"] == -7).all() and got["feat_track"].shape[0] == PAD


@pytest.mark.parametrize("L", [2, 63, 64, 65, 1024, 1025])
def test_track_lengths_at_the_sort_boundaries(gpu_ctx, L):
    fm, K = T.scene_chain(L)
    want, _ = check(gpu_ctx, "chain%d" % L, fm, K, upload=T.shuffled(fm, L))
    assert want["written"] == 2 and np.array_equal(np.diff(want["trk_off"]), [L, L])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_contended_unions_star(gpu_ctx, seed):
    fm, K = T.scene_star()
    check(gpu_ctx, "star", fm, K, upload=T.shuffled(fm, seed))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_contended_unions_grid(gpu_ctx, seed):
    fm, K = T.scene_grid()
    check(gpu_ctx, "grid", fm, K, upload=T.shuffled(fm, seed))


@pytest.mark.parametrize("conflict", [T.DROP_TRACK, T.DROP_IMAGE])
def test_giant_component(gpu_ctx, conflict):
    fm, K = T.scene_giant()
    _, ref = check(gpu_ctx, "giant", fm, K, caps=(4, 16), conflict=conflict)
    assert ref["stats"][4] > len(K)


@pytest.mark.parametrize("conflict", [T.DROP_TRACK, T.DROP_IMAGE])
def test_planted_conflict(gpu_ctx, conflict):
    fm, K = T.scene_conflict()
    want, _ = check(gpu_ctx, "conflict", fm, K, conflict=conflict)
    assert len(want["tracks"]) == (1 if conflict == T.DROP_TRACK else 2)


@pytest.mark.parametrize("conflict", [T.DROP_TRACK, T.DROP_IMAGE])
def test_selection_and_length_limits(gpu_ctx, conflict):
    fm, K = T.scene_six()
    check(gpu_ctx, "six", fm, K, conflict=conflict)
    want, _ = check(gpu_ctx, "six", fm, K, conflict=conflict, select=([7, 3, 5], [2, 0, 1]))      # camera rows in non-ascending order
    assert set(want["obs_cam"].tolist()) == {0, 1, 2}
    check(gpu_ctx, "six", fm, K, conflict=conflict, min_length=3)
    check(gpu_ctx, "six", fm, K, conflict=conflict, max_length=4)
    check(gpu_ctx, "six", fm, K, conflict=conflict, min_length=3, max_length=4, select=([8, 4, 6, 3], [9, 1, 0, 4]))


def test_capacities(gpu_ctx):
    fm, K = T.scene_six()
    coords = T.coords_of(K)
    ref = ref_of("six", fm, K, coords, conflict=T.DROP_IMAGE)
    nt, no = (int(c) for c in ref["counts"])
    assert nt >= 3
    put(gpu_ctx, fm, K, coords)
    for caps in ((0, 0), (nt, no), (nt - 1, no), (nt, no - 1), (nt + 3, no + 7), (0, no), (nt, 0), (1, no)):
        want = assert_equals_contract(run(gpu_ctx, *caps, conflict=T.DROP_IMAGE), ref, *caps)
        assert want["written"] == {(nt, no): nt, (nt - 1, no): nt - 1, (nt, no - 1): nt - 1, (nt + 3, no + 7): nt, (1, no): 1}.get(caps, 0)


def test_host_entry_and_too_small_a_capacity(gpu_ctx):
    fm, K = T.scene_six()
    coords = T.coords_of(K)
    ref = ref_of("six", fm, K, coords, conflict=T.DROP_IMAGE)
    put(gpu_ctx, fm, K, coords)
    r = tracks.build(gpu_ctx, tracks.options(conflict=T.DROP_IMAGE))
    for k in ("counts", "trk_off", "obs_img", "obs_feat", "obs_xy", "feat_track", "stats"):
        assert np.array_equal(r[k], ref[k]), k
    assert r["obs_cam"] is None
    with pytest.raises(_lib.RcnError) as e:
        tracks.build(gpu_ctx, tracks.options(conflict=T.DROP_IMAGE), capacity=(int(ref["counts"][0]) - 1, int(ref["counts"][1])))
    assert e.value.code == -1 and "capacity" in str(e.value)


def test_feeds_the_triangulation_and_repeats_itself(gpu_ctx):
    import torch
    sc = synth_ba.make_scene(6, 300, obs_per_point=4, seed=9)
    cam, pt, uv = sc["obs_cam"].reshape(-1, 4), sc["obs_pt"].reshape(-1, 4), sc["obs_uv"].reshape(-1, 4, 2).astype(np.int32)
    feat, coords, fm = {}, {c: [] for c in range(6)}, {}
    for p in range(len(cam)):
        for k in range(4):
            feat[(p, k)] = len(coords[cam[p, k]])
            coords[cam[p, k]].append(uv[p, k])
        for k in range(3):
            fm.setdefault((int(cam[p, k]), int(cam[p, k + 1])), []).append((feat[(p, k)], feat[(p, k + 1)]))
    K = {c: len(v) for c, v in coords.items()}
    coords = {c: np.asarray(v, np.int32).reshape(-1, 2) for c, v in coords.items()}
    select = ([5, 4, 3, 2, 1, 0], [5, 4, 3, 2, 1, 0])
    ref = T.build(*T.lists_of(fm), K, coords=coords, select=select)
    nt, no = (int(c) for c in ref["counts"])
    assert nt == 300 and no == 1200
    put(gpu_ctx, fm, K, coords)
    P, I = synth_ba.poses_to_34(sc["poses_gt"]), sc["intr_gt"]
    want_xyz, want_status = tri.triangulate_tracks(gpu_ctx, P, I, ref["trk_off"], ref["obs_cam"], ref["obs_xy"])
    assert (want_status == 0).any()
    dev = torch.device("cuda", gpu_ctx.device)
    runs = []
    for _ in range(2):
        out = tracks.build_device(gpu_ctx, nt, no, select=select)
        Pd, Id = torch.from_numpy(P).to(dev), torch.from_numpy(np.ascontiguousarray(I)).to(dev)
        xyz = torch.zeros((nt, 3), dtype=torch.float64, device=dev)
        status = torch.zeros(nt, dtype=torch.uint8, device=dev)
        compact = torch.zeros((nt, 3), dtype=torch.float64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        pb = _lib.TriangulationProblem(6, nt, no, 0, Pd.data_ptr(), Id.data_ptr(), out["trk_off"].data_ptr(), out["obs_cam"].data_ptr(),
                                       out["obs_xy"].data_ptr())
        gpu_ctx.check(gpu_ctx.lib.rcn_triangulate_device(gpu_ctx.h, C.byref(pb), tri.MAX_PROJECTION_ERROR, tri.MIN_TRIANGULATION_ANGLE,
                                                         xyz.data_ptr(), status.data_ptr(), compact.data_ptr(), 0, cnt.data_ptr()))
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        assert xyz.cpu().numpy().tobytes() == want_xyz.tobytes() and np.array_equal(status.cpu().numpy(), want_status)
        runs.append({k: v.cpu().numpy().tobytes() for k, v in out.items() if v is not None})
    assert runs[0] == runs[1]                                 # two calls in a row: identical bytes


def test_argument_errors(gpu_ctx):
    ctx = gpu_ctx
    fm, K = T.scene_conflict()
    coords = T.coords_of(K)
    put(ctx, fm, K, coords)

    def fails(code, text, **kw):
        with pytest.raises(_lib.RcnError) as e:
            run(ctx, 4, 16, **kw)
        assert e.value.code == code and text in str(e.value), str(e.value)

    fails(-1, "min_length", min_length=1)
    fails(-1, "max_length", min_length=3, max_length=2)
    fails(-1, "max_length", max_length=-1)
    fails(-1, "policy", conflict=2)
    fails(-1, "twice", select=([10, 11, 10], [0, 1, 2]))
    fails(-1, "negative camera row", select=([10, 11], [0, -1]))
    fails(-5, "not among", select=([10, 13], [0, 1]))
    o = tracks.options()
    o.reserved = 1
    with pytest.raises(_lib.RcnError) as e:
        tracks.build(ctx, o)
    assert e.value.code == -1 and "reserved" in str(e.value)
    import torch
    buf = torch.zeros(64, dtype=torch.int32, device=torch.device("cuda", ctx.device))
    p = C.c_void_p(buf.data_ptr())
    assert ctx.lib.rcn_tracks_build_device(ctx.h, None, 0, None, None, 4, 16, p, p, p, p, p, None, None, None) == -1      # camera rows without a selection
    assert "obs_cam" in ctx.lib.rcn_last_error(ctx.h).decode()
    assert ctx.lib.rcn_tracks_build_device(ctx.h, None, 0, None, None, -1, 16, p, p, p, p, None, None, None, None) == -1
    assert ctx.lib.rcn_tracks_build_device(ctx.h, None, 0, None, None, 4, 16, None, p, p, p, None, None, None, None) == -1
    # coordinates changed since the upload of the lists
    a = np.ascontiguousarray(coords[10])
    ctx.check(ctx.lib.rcn_coords_upload(ctx.h, 10, a.ctypes.data, len(a)))
    fails(-1, "coordinates changed")
    with pytest.raises(_lib.RcnError):
        tracks.layout(ctx)
    # no resident lists
    nextview.clear_lists(ctx)
    fails(-1, "no match lists")
    ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
