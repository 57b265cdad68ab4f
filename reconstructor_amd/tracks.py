"""Host mirror of track building over librcn.so (no CPU fallback): the tracks that the resident match lists
(nextview.upload_lists) tie together across all their images, after the conflict rule, the selection and the length filter.

    options        rcn_tracks_default_options with overrides
    layout         rcn_tracks_layout: the list images ascending and the first node of each (the order of feat_track)
    build          rcn_tracks_build: numpy arrays, synchronous
    build_device   rcn_tracks_build_device: torch tensors in HBM (asynchronous on the ctx stream), the CSR rcn_triangulate_device takes
    phase_ms       rcn_tracks_last_phase_ms: device milliseconds of the last build's hook, flatten, conflicts, scans, scatter, sort

The lists (rcn_match_lists_upload) and the integer coordinates of their images (rcn_coords_upload*) must be resident.  Nothing here
computes a component for a caller; smoke() restates one planted answer to check the run it made.
"""
import ctypes as C

import numpy as np

from . import _lib

DROP_TRACK, DROP_IMAGE = 0, 1
STATS = ("components", "conflicts", "dropped_by_conflict", "dropped_by_length", "largest_component", "longest_track", "edges", "reserved")


def options(**kw):
    o = _lib.TracksOptions()
    _lib.load().rcn_tracks_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("tracks: no option " + k)
        setattr(o, k, v)
    return o


_options = options          # build / build_device take an argument of that name


def layout(ctx):
    """Returns (img_ids[n], node_off[n + 1] int64): node = node_off[i] + feature."""
    n = C.c_int32(0)
    ctx.check(ctx.lib.rcn_tracks_layout(ctx.h, None, None, C.byref(n)))
    ids, off = np.zeros(max(n.value, 1), np.int32), np.zeros(n.value + 1, np.int64)
    ctx.check(ctx.lib.rcn_tracks_layout(ctx.h, ids.ctypes.data, off.ctypes.data, C.byref(n)))
    return ids[:n.value], off


def _select(select):
    if select is None:
        return 0, None, None
    img = np.ascontiguousarray(select[0], np.int32).reshape(-1)
    cam = np.ascontiguousarray(select[1], np.int32).reshape(-1)
    if len(img) != len(cam) or len(img) == 0:
        raise ValueError("tracks: select is (images, camera rows) of one non-zero length")
    return len(img), img, cam


def build(ctx, options=None, select=None, capacity=None):
    """select: (images, camera rows) or None (every image, no camera rows).  capacity: (tracks, observations) or None (sized by a
    second call when the first guess is too small).  Returns a dict: counts[2], trk_off[n_tracks + 1], obs_img, obs_feat, obs_cam
    (None without a selection), obs_xy[n_obs, 2], feat_track[n_nodes], stats[8] int64."""
    opt = options if options is not None else _options()
    n_sel, img, cam = _select(select)
    n_nodes = int(layout(ctx)[1][-1])
    cap_t, cap_o = (int(capacity[0]), int(capacity[1])) if capacity is not None else (max(1, n_nodes // 2), max(1, n_nodes))
    counts, stats = np.zeros(2, np.int32), np.zeros(8, np.int64)
    ft = np.full(max(n_nodes, 1), -1, np.int32)
    for _ in range(2):
        off = np.zeros(cap_t + 1, np.int32)
        oi, of, oc = (np.zeros(max(cap_o, 1), np.int32) for _ in range(3))
        xy = np.zeros((max(cap_o, 1), 2), np.int32)
        rc = ctx.lib.rcn_tracks_build(ctx.h, C.byref(opt), n_sel, img.ctypes.data if n_sel else None, cam.ctypes.data if n_sel else None,
                                      cap_t, cap_o, counts.ctypes.data, off.ctypes.data, oi.ctypes.data, of.ctypes.data,
                                      oc.ctypes.data if n_sel else None, xy.ctypes.data, ft.ctypes.data, stats.ctypes.data)
        if rc != _lib.RCN_OK and capacity is None and (counts[0] > cap_t or counts[1] > cap_o):
            cap_t, cap_o = int(counts[0]), int(counts[1])
            continue
        ctx.check(rc)
        break
    nt, no = int(counts[0]), int(counts[1])
    return dict(counts=counts, trk_off=off[:nt + 1], obs_img=oi[:no], obs_feat=of[:no], obs_cam=oc[:no] if n_sel else None,
                obs_xy=xy[:no], feat_track=ft[:n_nodes], stats=stats)


def build_device(ctx, cap_tracks, cap_obs, options=None, select=None, want_xy=True, want_feat_track=True, want_stats=True, pad=0):
    """Returns a dict of CUDA tensors: counts[2], trk_off[cap_tracks + 1], obs_img / obs_feat / obs_cam[cap_obs] (obs_cam None
    without a selection), obs_xy[2 cap_obs], feat_track[n_nodes], stats[8] int64.  Asynchronous on the ctx stream.  pad > 0 appends
    that many words holding -7 behind every array (the library must leave them alone); every array starts out as -7."""
    import torch
    opt = options if options is not None else _options()
    n_sel, img, cam = _select(select)
    dev = torch.device("cuda", ctx.device)
    n_nodes = int(layout(ctx)[1][-1])
    ct, co = int(cap_tracks), int(cap_obs)
    mk = lambda n, dt=torch.int32: torch.full((n + pad,), -7, dtype=dt, device=dev)
    out = dict(counts=mk(2), trk_off=mk(ct + 1), obs_img=mk(co), obs_feat=mk(co), obs_cam=mk(co) if n_sel else None,
               obs_xy=mk(2 * co) if want_xy else None, feat_track=mk(n_nodes) if want_feat_track else None,
               stats=mk(8, torch.int64) if want_stats else None)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_tracks_build_device(ctx.h, C.byref(opt), n_sel, img.ctypes.data if n_sel else None, cam.ctypes.data if n_sel else None,
                                              ct, co, ptr(out["counts"]), ptr(out["trk_off"]), ptr(out["obs_img"]), ptr(out["obs_feat"]),
                                              ptr(out["obs_cam"]), ptr(out["obs_xy"]), ptr(out["feat_track"]), ptr(out["stats"])))
    return out


def phase_ms(ctx):
    ms = np.zeros(6, np.float64)
    ctx.check(ctx.lib.rcn_tracks_last_phase_ms(ctx.h, ms.ctypes.data))
    return ms


def smoke(ctx):
    """Five images of four keypoints, features 0 .. 3 chained f -> f through the pairs (i, i + 1) -- feature 3 only as far as image
    2 -- and one planted wrong match (0, 2): 2 -> 3, which ties the chains of features 2 and 3 together so that images 0, 1 and 2
    occur twice in that component.  DROP_TRACK keeps the chains of features 0 and 1; DROP_IMAGE also the rest of the conflicting
    component, (3, 2) and (4, 2).  Returns (tracks, observations, tracks under DROP_IMAGE)."""
    from . import nextview
    for i in range(5):
        xy = np.c_[10 * i + np.arange(4), 100 + np.arange(4)].astype(np.int32)
        ctx.check(ctx.lib.rcn_coords_upload(ctx.h, i, xy.ctypes.data, 4))
    fm = {(i, i + 1): [(f, f) for f in range(4 if i < 2 else 3)] for i in range(4)}
    fm[(0, 2)] = [(2, 3)]
    nextview.upload_feature_matches(ctx, fm)
    try:
        r = build(ctx)
        chain = lambda f, imgs: [(i, f) for i in imgs]
        want = [chain(0, range(5)), chain(1, range(5))]
        got = [list(zip(r["obs_img"][a:b].tolist(), r["obs_feat"][a:b].tolist())) for a, b in zip(r["trk_off"][:-1], r["trk_off"][1:])]
        assert got == want, "tracks: the two clean chains were not found"
        assert r["stats"].tolist() == [3, 1, 8, 0, 8, 5, 15, 0], "tracks: statistics of the planted scene"
        assert np.array_equal(r["obs_xy"], np.array([[10 * i + f, 100 + f] for t in want for i, f in t], np.int32)), "tracks: pixels"
        r1 = build(ctx, options(conflict=DROP_IMAGE))
        got1 = [list(zip(r1["obs_img"][a:b].tolist(), r1["obs_feat"][a:b].tolist())) for a, b in zip(r1["trk_off"][:-1], r1["trk_off"][1:])]
        assert got1 == want + [chain(2, (3, 4))], "tracks: DROP_IMAGE keeps the conflict-free rest of the component"
        return len(want), int(r["counts"][1]), len(got1)
    finally:
        nextview.clear_lists(ctx)
        ctx.check(ctx.lib.rcn_coords_clear(ctx.h))
