"""Host mirror of the reference's multi-view triangulation over librcn.so (no CPU fallback).

    SequentialReconstructor::triangulateMultiView        SequentialReconstructor.cpp:396-489
    SequentialReconstructor::triangulateInitialPair      SequentialReconstructor.cpp:377-394
    SequentialReconstructor::triangulateMatchedLandmarks SequentialReconstructor.cpp:492-556 (step 3)

`triangulate_tracks` is the flat form: one batched launch for any number of tracks.  The candidate builders are pure
index logic -- which (image, feature) lists the reference's loops would hand to triangulateMultiView, in the order the
caller's containers iterate -- so that a whole loop becomes one launch (DESIGN.md section 15 says why that is exact).
"""
import ctypes as C

import numpy as np

from . import _lib

MAX_PROJECTION_ERROR = 4.0      # SequentialReconstructor.h:256
MIN_TRIANGULATION_ANGLE = 1.0   # SequentialReconstructor.h:257

ACCEPTED, REJECT_SOLVE, REJECT_REPROJECTION, REJECT_ANGLE = 0, 1, 2, 3


def _problem(poses34, intrinsics, trk_off, obs_cam, obs_xy):
    poses34 = np.ascontiguousarray(poses34, np.float64).reshape(-1, 12)
    intrinsics = np.ascontiguousarray(intrinsics, np.float64).reshape(-1, 6)
    trk_off = np.ascontiguousarray(trk_off, np.int32)
    obs_cam = np.ascontiguousarray(obs_cam, np.int32)
    obs_xy = np.ascontiguousarray(obs_xy, np.int32).reshape(-1, 2)
    if len(poses34) != len(intrinsics):
        raise ValueError("one intrinsics row per pose")
    if len(trk_off) < 1 or len(obs_xy) != len(obs_cam):
        raise ValueError("trk_off needs n_tracks + 1 entries; obs_xy one row per observation")
    keep = (poses34, intrinsics, trk_off, obs_cam, obs_xy)
    pb = _lib.TriangulationProblem(len(poses34), len(trk_off) - 1, len(obs_cam), 0,
                                   poses34.ctypes.data, intrinsics.ctypes.data, trk_off.ctypes.data,
                                   obs_cam.ctypes.data, obs_xy.ctypes.data)
    return pb, keep


def triangulate_tracks(ctx, poses34, intrinsics, trk_off, obs_cam, obs_xy,
                       max_projection_error=MAX_PROJECTION_ERROR, min_triangulation_angle=MIN_TRIANGULATION_ANGLE):
    """triangulateMultiView for every track of a CSR batch (rcn_triangulate).  Returns (xyz[n_tracks, 3], status[n_tracks]
    uint8): xyz holds every track's X, accepted or not; status 0 accepted, 1 zero singular value / world z not > 0,
    2 reprojection, 3 angle."""
    pb, keep = _problem(poses34, intrinsics, trk_off, obs_cam, obs_xy)
    n = pb.n_tracks
    xyz = np.zeros((max(n, 1), 3))
    status = np.zeros(max(n, 1), np.uint8)
    cnt = C.c_int32(0)
    ctx.check(ctx.lib.rcn_triangulate(ctx.h, C.byref(pb), float(max_projection_error), float(min_triangulation_angle),
                                      xyz.ctypes.data, status.ctypes.data, C.addressof(cnt)))
    del keep
    return xyz[:n], status[:n]


def triangulate_tracks_device(ctx, poses34, intrinsics, trk_off, obs_cam, obs_xy, compact_first=0,
                              max_projection_error=MAX_PROJECTION_ERROR, min_triangulation_angle=MIN_TRIANGULATION_ANGLE):
    """rcn_triangulate_device on torch tensors in HBM.  Returns (xyz, status, compact, n_accepted) as device tensors:
    compact holds the accepted tracks' X at rows compact_first, compact_first + 1, ... (rows before that are zero)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).contiguous().to(dev)
    P = t(np.asarray(poses34, np.float64).reshape(-1, 12), torch.float64)
    K = t(np.asarray(intrinsics, np.float64).reshape(-1, 6), torch.float64)
    off = t(np.asarray(trk_off, np.int32), torch.int32)
    cam = t(np.asarray(obs_cam, np.int32), torch.int32)
    xy = t(np.asarray(obs_xy, np.int32).reshape(-1, 2), torch.int32)
    n = off.numel() - 1
    xyz = torch.zeros((max(n, 1), 3), dtype=torch.float64, device=dev)
    status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    compact = torch.zeros((compact_first + max(n, 1), 3), dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    pb = _lib.TriangulationProblem(P.shape[0], n, cam.numel(), 0, P.data_ptr(), K.data_ptr(), off.data_ptr(),
                                   cam.data_ptr(), xy.data_ptr())
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_triangulate_device(ctx.h, C.byref(pb), float(max_projection_error), float(min_triangulation_angle),
                                             xyz.data_ptr(), status.data_ptr(), compact.data_ptr(), int(compact_first), cnt.data_ptr()))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    return xyz[:n], status[:n], compact, cnt


# ---- candidate builders: which tracks the reference's loops hand to triangulateMultiView (no arithmetic) ----------------

def initial_pair_tracks(matches, img1=0, img2=1):
    """triangulateInitialPair (:377-394): one track [(img1, f1), (img2, f2)] per match, in the iteration order given
    (the caller's featureMatches[(img1, img2)]; a dict or any iterable of (f1, f2) pairs)."""
    items = matches.items() if hasattr(matches, "items") else matches
    return [[(img1, int(f1)), (img2, int(f2))] for f1, f2 in items]


def new_view_tracks(img, landmark_ids, registered, img_matches, feature_matches):
    """Step 3 of triangulateMatchedLandmarks (:514-553) for the new image `img`, after step 1.

    landmark_ids     {image: sequence of landmarkId per feature} (-1: not a landmark), as features[*][*]->landmarkId
    registered       [(image, status)] in the caller's registeredImages iteration order (never sorted here)
    img_matches      {image: images it was matched with} (imgMatches)
    feature_matches  {(img, other): {feature of img: feature of other}}
    Returns the tracks [(reg image, its feature), (img, feature)] in feature order: for every feature of img that is not
    a landmark, the first registered image matched with img whose pair map holds the feature and whose partner is not a
    landmark either (the break of :548 follows the call whether or not the track is accepted)."""
    out = []
    matched = set(img_matches[img])
    own = landmark_ids[img]
    for f in range(len(own)):
        if own[f] != -1:
            continue
        for reg, status in registered:
            if not status or reg not in matched:
                continue
            pm = feature_matches.get((img, reg))
            if pm is None or f not in pm:
                continue
            g = pm[f]
            if landmark_ids[reg][g] == -1:
                out.append([(reg, int(g)), (img, f)])
                break
    return out


def tracks_to_arrays(tracks, cam_index, coords):
    """Flatten tracks of (image, feature) into (trk_off, obs_cam, obs_xy): cam_index maps an image to its camera row,
    coords[image][feature] is the integer pixel (x, y)."""
    off = np.zeros(len(tracks) + 1, np.int32)
    cam, xy = [], []
    for j, t in enumerate(tracks):
        for img, f in t:
            cam.append(cam_index[img])
            xy.append((int(coords[img][f][0]), int(coords[img][f][1])))
        off[j + 1] = len(cam)
    return off, np.asarray(cam, np.int32), np.asarray(xy, np.int32).reshape(-1, 2)
