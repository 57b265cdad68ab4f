"""Step 3 of the reference's triangulateMatchedLandmarks on the device, over librcn.so (no CPU fallback).

    SequentialReconstructor::triangulateMatchedLandmarks   SequentialReconstructor.cpp:514-553 (step 3)

`LandmarkIds` is the device copy of features[*][*]->landmarkId; `new_view_tracks_device` finds the tracks the reference's loop
would hand to triangulateMultiView for a new image from the resident match lists (nextview.upload_lists), the resident
coordinates and that table; `new_view_triangulate_device` also triangulates them and commits the accepted tracks' landmark
indices to the table; ba.BaSession.grow_view does the same straight into a session.  triangulate.new_view_tracks is the host
walk they all reproduce, track for track.  DESIGN.md section 25.
"""
import ctypes as C

import numpy as np

from . import _lib
from .triangulate import MAX_PROJECTION_ERROR, MIN_TRIANGULATION_ANGLE


class LandmarkIds:
    """The landmark-id table resident in the ctx (rcn_landmark_ids_*): one int32 per keypoint of every image with resident
    coordinates, -1 = not a landmark.  A new upload of lists or coordinates invalidates it until the next reset()."""

    def __init__(self, ctx):
        self.ctx = ctx

    def reset(self):
        self.ctx.check(self.ctx.lib.rcn_landmark_ids_reset(self.ctx.h))

    def set(self, img, feat, ids):
        """Entries (image, feature) get the landmark id given; -1 frees an entry.  img may be one image for all entries."""
        feat = np.ascontiguousarray(feat, np.int32).reshape(-1)
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(ids, np.int32), feat.shape))
        img = np.ascontiguousarray(np.broadcast_to(np.asarray(img, np.int32), feat.shape))
        n = len(feat)
        self.ctx.check(self.ctx.lib.rcn_landmark_ids_set(self.ctx.h, n, img.ctypes.data if n else None,
                                                         feat.ctypes.data if n else None, ids.ctypes.data if n else None))

    def set_all(self, landmark_ids):
        """{image: landmarkId per feature}: every entry that is not -1 (after a reset the rest already is)."""
        img, feat, ids = [], [], []
        for i, row in landmark_ids.items():
            for f, l in enumerate(row):
                if l != -1:
                    img.append(i), feat.append(f), ids.append(l)
        self.set(img, feat, ids)

    def read(self, img, K):
        out = np.zeros(max(int(K), 1), np.int32)
        self.ctx.check(self.ctx.lib.rcn_landmark_ids_read(self.ctx.h, int(img), out.ctypes.data, int(K)))
        return out[:K]


def visited(img, registered, img_matches):
    """The registered images the loop of :521-551 looks at for the new image `img`, in the caller's registeredImages
    iteration order: status true and matched with img (the filter of triangulate.new_view_tracks)."""
    matched = set(img_matches[img])
    return [int(reg) for reg, status in registered if status and reg in matched]


def _reg_arrays(img, registered, img_matches, cam_index):
    reg = visited(img, registered, img_matches)
    return np.asarray(reg, np.int32), np.asarray([cam_index[r] for r in reg], np.int32)


def new_view_tracks_device(ctx, img, registered, img_matches, cam_index, capacity, pad=0):
    """rcn_new_view_tracks_device for the new image `img`.  registered / img_matches as triangulate.new_view_tracks takes them,
    cam_index {image: camera row}.  Returns device tensors (n_tracks[1], trk_off[capacity + 1], obs_cam[2 capacity],
    obs_xy[2 capacity, 2], trk_src[capacity, 3]); pad > 0 appends that many int32 words holding -7 behind every array (the
    library must leave them alone)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    reg, cam = _reg_arrays(img, registered, img_matches, cam_index)
    cap = int(capacity)
    mk = lambda n: torch.full((n + pad,), -7, dtype=torch.int32, device=dev)
    n_tracks, off, ocam, oxy, src = mk(1), mk(cap + 1), mk(2 * cap), mk(4 * cap), mk(3 * cap)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_new_view_tracks_device(ctx.h, int(img), len(reg), reg.ctypes.data if len(reg) else None, int(cam_index[img]),
                                                 cam.ctypes.data if len(reg) else None, cap, n_tracks.data_ptr(), off.data_ptr(),
                                                 ocam.data_ptr(), oxy.data_ptr(), src.data_ptr()))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    if pad:
        return n_tracks, off, ocam, oxy, src
    return n_tracks, off, ocam, oxy.reshape(-1, 2), src.reshape(-1, 3)


def new_view_triangulate_device(ctx, img, registered, img_matches, cam_index, poses34, intrinsics, first_landmark, capacity,
                                compact_first=0, max_projection_error=MAX_PROJECTION_ERROR,
                                min_triangulation_angle=MIN_TRIANGULATION_ANGLE):
    """rcn_new_view_triangulate_device: the candidates, their triangulation against poses34 / intrinsics (one row per camera;
    numpy or device tensors) and the commit of first_landmark + rank into the table.  Returns a dict of device tensors:
    n_tracks, trk_off, obs_cam, obs_xy, trk_src (new_view_tracks_device) and xyz[capacity, 3], status[capacity],
    compact[compact_first + capacity, 3], n_accepted[1] (triangulate.triangulate_tracks_device)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    reg, cam = _reg_arrays(img, registered, img_matches, cam_index)
    cap = int(capacity)
    t = lambda a, w: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, np.float64))).to(dev).reshape(-1, w).contiguous()
    P, K = t(poses34, 12), t(intrinsics, 6)
    if P.shape[0] != K.shape[0]:
        raise ValueError("one intrinsics row per pose")
    mk = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    out = dict(n_tracks=mk(1), trk_off=mk(cap + 1), obs_cam=mk(2 * cap), obs_xy=mk(4 * cap), trk_src=mk(3 * cap),
               xyz=torch.zeros((max(cap, 1), 3), dtype=torch.float64, device=dev),
               status=torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev),
               compact=torch.zeros((compact_first + max(cap, 1), 3), dtype=torch.float64, device=dev), n_accepted=mk(1))
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.rcn_new_view_triangulate_device(
        ctx.h, int(img), len(reg), reg.ctypes.data if len(reg) else None, int(cam_index[img]), cam.ctypes.data if len(reg) else None,
        P.shape[0], P.data_ptr(), K.data_ptr(), float(max_projection_error), float(min_triangulation_angle), int(first_landmark), cap,
        out["n_tracks"].data_ptr(), out["trk_off"].data_ptr(), out["obs_cam"].data_ptr(), out["obs_xy"].data_ptr(),
        out["trk_src"].data_ptr(), out["xyz"].data_ptr(), out["status"].data_ptr(), out["compact"].data_ptr(), int(compact_first),
        out["n_accepted"].data_ptr()))
    ctx.check(ctx.lib.rcn_synchronize(ctx.h))
    out["obs_xy"] = out["obs_xy"].reshape(-1, 2)
    out["trk_src"] = out["trk_src"].reshape(-1, 3)
    out["xyz"], out["status"] = out["xyz"][:cap], out["status"][:cap]
    return out
