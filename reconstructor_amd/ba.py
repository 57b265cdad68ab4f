"""Host-side mirror (Python) of the reference's BundleAdjuster over the C ABI.

  BundleAdjuster::adjust(features, landmarks, imgIdx2camPose, imgIdx2camIntrinsics, imgIdxOrder)
      BundleAdjuster.h:80-84 / BundleAdjuster.cpp:11-188
`solve_flat` is the flat form (what adjust packs, :17-97); `BundleAdjuster.adjust` packs and
unpacks exactly as the reference does, including its quirks (axis/(angle+1e-6) on unpack,
:161-170; integer feature coordinates, :83-84).  The C++ form of the same adapter is
reconstructor_amd/host/HipBundleAdjuster.h.  All arithmetic of the solve runs in librcn.so.
"""
import ctypes as C

import numpy as np

from . import _lib

TERMINATION = {1: "CONVERGENCE (function tolerance)", 2: "CONVERGENCE (gradient tolerance)",
               3: "CONVERGENCE (parameter tolerance)", 4: "CONVERGENCE (trust region radius)",
               5: "NO_CONVERGENCE (max iterations)", 6: "FAILURE"}


def default_options(ctx, n_cams):
    o = _lib.BaOptions()
    ctx.lib.rcn_ba_default_options(int(n_cams), C.byref(o))
    return o


def summary_dict(s):
    d = {k: getattr(s, k) for k, _ in s._fields_ if k != "cost_trace"}
    d["cost_trace"] = np.array(s.cost_trace[:min(160, s.iterations + 1)])
    return d


LOSS_KINDS = {"trivial": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}


def make_loss(loss):
    """None, an rcn_ba_loss, or (kind, scale) with kind a name of LOSS_KINDS or its number -> _lib.BaLoss or None"""
    if loss is None or isinstance(loss, _lib.BaLoss):
        return loss
    kind, scale = loss
    return _lib.BaLoss(LOSS_KINDS[kind] if isinstance(kind, str) else int(kind), 0, float(scale))


def loss_report_dict(r):
    return {k: getattr(r, k) for k, _ in r._fields_}


def solve_flat(ctx, poses, intrinsics, points, obs_uv, obs_cam, obs_pt, options=None, allow_failure=False, loss=None, report=False,
               constant=None, groups=None):
    """Returns (poses, intrinsics, points, summary); inputs are copied, not modified.
    groups: None or one int per camera (rcn_ba_solve_tied): -1 = the camera's own intrinsics, equal values >= 0 = one physical camera,
    whose fx, fy, k1, k2 are one set of unknowns in intrinsics mode 1; members enter and leave with bit-identical intrinsics.
    constant: None or a mask over the cameras (rcn_ba_solve_constant): a camera with a true entry has no free parameter and comes
    back unchanged bit for bit.
    allow_failure: a solve that ends in RCN_BA_FAILURE (RCN_ERR_NUMERIC; the summary is filled) returns instead of raising.
    loss: None (rcn_ba_solve) or what make_loss takes (rcn_ba_solve_robust: Huber, soft-L1 or Cauchy with a scale in pixels; the
    summary's costs are then robust costs).  report: the summary also carries "loss_report" (rcn_ba_loss_report as a dict) and
    "loss_weights" (rho'(s) per observation) at the final point."""
    poses = np.array(poses, np.float64, order="C")
    intr = np.array(intrinsics, np.float64, order="C")
    pts = np.array(points, np.float64, order="C").reshape(-1, 3)
    uv = np.ascontiguousarray(obs_uv, np.float64)
    cam = np.ascontiguousarray(obs_cam, np.int32)
    pt = np.ascontiguousarray(obs_pt, np.int32)
    pb = _lib.BaProblem(poses.shape[0], pts.shape[0], cam.shape[0], 0,
                        poses.ctypes.data, intr.ctypes.data, pts.ctypes.data if pts.size else None,
                        uv.ctypes.data if uv.size else None, cam.ctypes.data if cam.size else None,
                        pt.ctypes.data if pt.size else None)
    o = options if options is not None else default_options(ctx, poses.shape[0])
    s = _lib.BaSummary()
    mask = None
    if constant is not None:
        mask = np.ascontiguousarray(np.asarray(constant) != 0, np.uint8)
        if mask.shape != (poses.shape[0],):
            raise ValueError("solve_flat: constant must hold one entry per camera")
    if groups is not None:
        grp = np.ascontiguousarray(groups, np.int32)
        if grp.shape != (poses.shape[0],):
            raise ValueError("solve_flat: groups must hold one entry per camera")
        ls = make_loss(loss)
        rep = _lib.BaLossReport()
        w = np.zeros(max(cam.shape[0], 1))
        rc = ctx.lib.rcn_ba_solve_tied(ctx.h, C.byref(pb), C.byref(o), C.byref(ls) if ls is not None else None,
                                       mask.ctypes.data if mask is not None else None, grp.ctypes.data,
                                       C.byref(s), C.byref(rep) if report else None, w.ctypes.data if report else None)
    elif constant is not None:
        ls = make_loss(loss)
        rep = _lib.BaLossReport()
        w = np.zeros(max(cam.shape[0], 1))
        rc = ctx.lib.rcn_ba_solve_constant(ctx.h, C.byref(pb), C.byref(o), C.byref(ls) if ls is not None else None, mask.ctypes.data,
                                           C.byref(s), C.byref(rep) if report else None, w.ctypes.data if report else None)
    elif loss is None and not report:
        rc = ctx.lib.rcn_ba_solve(ctx.h, C.byref(pb), C.byref(o), C.byref(s))
    else:
        ls = make_loss(loss)
        rep = _lib.BaLossReport()
        w = np.zeros(max(cam.shape[0], 1))
        rc = ctx.lib.rcn_ba_solve_robust(ctx.h, C.byref(pb), C.byref(o), C.byref(ls) if ls is not None else None, C.byref(s),
                                         C.byref(rep) if report else None, w.ctypes.data if report else None)
    if not (allow_failure and rc == -6 and s.termination == 6):
        ctx.check(rc)
    d = summary_dict(s)
    if report:
        d["loss_report"], d["loss_weights"] = loss_report_dict(rep), w[:cam.shape[0]]
    return poses, intr, pts, d


def solve_scene(ctx, scene, options=None, allow_failure=False, loss=None, report=False, constant=None, groups=None):
    return solve_flat(ctx, scene["poses"], scene["intrinsics"], scene["points"], scene["obs_uv"],
                      scene["obs_cam"], scene["obs_pt"], options, allow_failure, loss, report, constant, groups)


def _rot_to_angle_axis(R):
    c = (np.trace(R) - 1.0) / 2.0
    th = np.arccos(np.clip(c, -1.0, 1.0))
    if th < 1e-12:
        return np.zeros(3)
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (2.0 * np.sin(th))
    return ax * th


def _angle_axis_to_rot(angle, axis):
    """Eigen::AngleAxisd(angle, axis).toRotationMatrix() for a possibly non-unit axis."""
    c, s = np.cos(angle), np.sin(angle)
    x, y, z = axis
    t = 1 - c
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


class BundleAdjuster:
    """Same call shape as the reference class (BundleAdjuster.h:76-85)."""

    def __init__(self, ctx=None, device=0, loss=None):
        """loss: None (the reference: no loss) or what make_loss takes, for every adjust()"""
        self.ctx = ctx if ctx is not None else _lib.Context(device)
        self.last_summary = None
        self.loss = make_loss(loss)

    def adjust(self, features, landmarks, img_idx2cam_pose, img_idx2cam_intrinsics, img_idx_order):
        """features[img][feat] -> (x, y) integer pixel coords (or objects with .featCoord.x/.y);
        landmarks: list of dicts/objects with x, y, z and triangulatedFeatures = [(imgIdx, featIdx)];
        img_idx2cam_pose: {img: 4x4 world->camera}; img_idx2cam_intrinsics: {img: [fx,fy,cx,cy,k1,k2]}.
        Updates landmarks, poses and intrinsics in place; returns {global img idx: local idx}."""
        order = list(img_idx_order)
        g2l = {g: l for l, g in enumerate(order)}                       # BundleAdjuster.cpp:34-63
        nc = len(order)
        poses = np.zeros((nc, 6)); intr = np.zeros((nc, 6))
        for l, g in enumerate(order):
            intr[l] = np.asarray(img_idx2cam_intrinsics[g], np.float64)[:6]
            T = np.asarray(img_idx2cam_pose[g], np.float64)
            poses[l, :3] = _rot_to_angle_axis(T[:3, :3])
            poses[l, 3:] = T[:3, 3]
        get = (lambda lm, k: lm[k]) if isinstance(landmarks[0], dict) else getattr
        pts = np.array([[get(lm, "x"), get(lm, "y"), get(lm, "z")] for lm in landmarks], np.float64)
        uv, cam, pt = [], [], []
        for j, lm in enumerate(landmarks):                              # :74-97, landmark-major
            for (img, feat) in get(lm, "triangulatedFeatures"):
                f = features[img][feat]
                xy = (f.featCoord.x, f.featCoord.y) if hasattr(f, "featCoord") else (f[0], f[1])
                uv.append((float(xy[0]), float(xy[1]))); cam.append(g2l[img]); pt.append(j)
        P, I, X, s = solve_flat(self.ctx, poses, intr, pts, np.array(uv).reshape(-1, 2),
                                np.array(cam, np.int32), np.array(pt, np.int32), loss=self.loss)
        self.last_summary = s
        for j, lm in enumerate(landmarks):                              # :150-155
            if isinstance(lm, dict):
                lm["x"], lm["y"], lm["z"] = X[j]
            else:
                lm.x, lm.y, lm.z = X[j]
        for l, g in enumerate(order):                                   # :157-185
            ang = float(np.sqrt((P[l, :3] ** 2).sum()))
            axis = P[l, :3] / (ang + 1e-6)                               # the reference's non-unit axis
            T = np.eye(4)
            T[:3, :3] = _angle_axis_to_rot(ang, axis)
            T[:3, 3] = P[l, 3:]
            img_idx2cam_pose[g] = T
            img_idx2cam_intrinsics[g] = I[l].copy()
        return g2l


def poses34_from_angle_axis(poses):
    """[R | t] rows as the reference's pipeline holds them after adjust(): the unpack of BundleAdjuster.cpp:157-185,
    non-unit axis w / (angle + 1e-6) included."""
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    out = np.zeros((len(poses), 12))
    for l, p in enumerate(poses):
        ang = float(np.sqrt((p[:3] ** 2).sum()))
        R = _angle_axis_to_rot(ang, p[:3] / (ang + 1e-6))
        out[l] = np.concatenate([R, p[3:, None]], 1).reshape(-1)
    return out


class BaSession:
    """rcn_ba_session: the incremental loop's problem resident in HBM across its N - 2 global solves
    (SequentialReconstructor.cpp:1040-1094).  Cameras / landmarks / observations are appended; solve(), validity()
    and remove_outliers() work on the device arrays."""

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.rcn_ba_session_create(ctx.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.rcn_ba_session_destroy(self.h)
            self.h = None

    def add_camera(self, pose6, intr6):
        p, k = np.ascontiguousarray(pose6, np.float64), np.ascontiguousarray(intr6, np.float64)
        idx = C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_add_camera(self.h, p.ctypes.data, k.ctypes.data, C.byref(idx)))
        return idx.value

    def add_points(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        first = C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_add_points(self.h, len(xyz), xyz.ctypes.data if len(xyz) else None, C.byref(first)))
        return first.value

    def add_observations(self, pt, cam, xy):
        pt, cam = np.ascontiguousarray(pt, np.int32), np.ascontiguousarray(cam, np.int32)
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        self.ctx.check(self.ctx.lib.rcn_ba_session_add_observations(self.h, len(pt), pt.ctypes.data if len(pt) else None,
                                                                    cam.ctypes.data if len(pt) else None, xy.ctypes.data if len(pt) else None))

    def counts(self):
        nc, npts, no = C.c_int32(), C.c_int32(), C.c_int64()
        self.ctx.check(self.ctx.lib.rcn_ba_session_counts(self.h, C.byref(nc), C.byref(npts), C.byref(no)))
        return nc.value, npts.value, no.value

    def cameras(self, poses=None, intr=None):
        """Returns (poses, intrinsics); arrays given are written into the session first."""
        nc = self.counts()[0]
        pi = None if poses is None else np.ascontiguousarray(poses, np.float64)
        ki = None if intr is None else np.ascontiguousarray(intr, np.float64)
        po, ko = np.zeros((nc, 6)), np.zeros((nc, 6))
        self.ctx.check(self.ctx.lib.rcn_ba_session_cameras(self.h, po.ctypes.data, ko.ctypes.data,
                                                           pi.ctypes.data if pi is not None else None, ki.ctypes.data if ki is not None else None))
        return po, ko

    def graph(self):
        no = self.counts()[2]
        pt, cam, xy = np.zeros(no, np.int32), np.zeros(no, np.int32), np.zeros((no, 2), np.int32)
        self.ctx.check(self.ctx.lib.rcn_ba_session_graph(self.h, pt.ctypes.data, cam.ctypes.data, xy.ctypes.data))
        return pt, cam, xy

    def points(self):
        x = np.zeros((self.counts()[1], 3))
        self.ctx.check(self.ctx.lib.rcn_ba_session_read_points(self.h, x.ctypes.data))
        return x

    def solve(self, options=None):
        s = _lib.BaSummary()
        self.ctx.check(self.ctx.lib.rcn_ba_session_solve(self.h, C.byref(options) if options is not None else None, C.byref(s)))
        return summary_dict(s)

    def solve_local(self, free_cams, options=None):
        """Local adjustment (rcn_ba_session_solve_local): the cameras free_cams and the landmarks they see move, every other camera that
        sees one of those landmarks is constant, everything else stays.  Returns (summary, info) with info = dict(n_cams, n_constant,
        n_points, n_obs) of the sub-problem."""
        fc = np.ascontiguousarray(free_cams, np.int32).reshape(-1)
        s = _lib.BaSummary()
        info = np.zeros(4, np.int32)
        self.ctx.check(self.ctx.lib.rcn_ba_session_solve_local(self.h, fc.ctypes.data if len(fc) else None, len(fc),
                                                               C.byref(options) if options is not None else None, C.byref(s), info.ctypes.data))
        return summary_dict(s), dict(zip(("n_cams", "n_constant", "n_points", "n_obs"), (int(v) for v in info)))

    def local_seconds(self):
        """(extraction, solve, scatter) host-clock seconds of the last solve_local"""
        t = np.zeros(3)
        self.ctx.check(self.ctx.lib.rcn_ba_session_local_seconds(self.h, t.ctypes.data))
        return tuple(float(v) for v in t)

    def covisible(self, cam, k):
        """(the k cameras that share the most landmarks with `cam`, count descending, ties to the lower index -- fewer when fewer
        share any; landmarks shared with `cam` per session camera, [cam] = its own landmark count)  (rcn_ba_session_covisible)"""
        nc = self.counts()[0]
        cams, counts, n = np.zeros(max(int(k), 1), np.int32), np.zeros(max(nc, 1), np.int32), C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_covisible(self.h, int(cam), int(k), cams.ctypes.data, C.byref(n), counts.ctypes.data))
        return cams[:n.value].copy(), counts[:nc]

    def set_loss(self, loss):
        """the loss of every later solve (rcn_ba_session_set_loss): None switches it off"""
        ls = make_loss(loss)
        self.ctx.check(self.ctx.lib.rcn_ba_session_set_loss(self.h, C.byref(ls) if ls is not None else None))

    def set_groups(self, groups):
        """the groups of every later solve and solve_local (rcn_ba_session_set_groups): one int per camera, -1 = its own intrinsics;
        None clears them.  Cameras added afterwards are -1 until set again."""
        if groups is None:
            self.ctx.check(self.ctx.lib.rcn_ba_session_set_groups(self.h, None, 0))
            return
        g = np.ascontiguousarray(groups, np.int32).reshape(-1)
        self.ctx.check(self.ctx.lib.rcn_ba_session_set_groups(self.h, g.ctypes.data if len(g) else None, len(g)))

    def loss_report(self):
        """(rcn_ba_loss_report as a dict, rho'(s) per observation) at the session's current state, under its loss"""
        rep = _lib.BaLossReport()
        w = np.zeros(max(self.counts()[2], 1))
        self.ctx.check(self.ctx.lib.rcn_ba_session_loss_report(self.h, C.byref(rep), w.ctypes.data))
        return loss_report_dict(rep), w[:self.counts()[2]]

    def validity(self, poses34=None, max_err=4.0, min_angle=1.0):
        """checkLandmarkValidity on the device arrays; returns (inlier flags, observations erased)."""
        if poses34 is None:
            poses34 = poses34_from_angle_axis(self.cameras()[0])
        p = np.ascontiguousarray(poses34, np.float64)
        inl = np.zeros(max(1, self.counts()[1]), np.uint8)
        n_in, n_er = C.c_int32(), C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_validity(self.h, p.ctypes.data, float(max_err), float(min_angle), inl.ctypes.data, C.byref(n_in), C.byref(n_er)))
        return inl[:self.counts()[1]].astype(bool), n_er.value

    def triangulate(self, trk_off, obs_cam, obs_xy, poses34=None, max_err=4.0, min_angle=1.0):
        """triangulateMultiView for a CSR batch of tracks (camera indices = session indices) straight into the session:
        accepted tracks become landmarks (in track order) with their observations.  Returns (status per track, index of
        the first new landmark, landmarks added)."""
        if poses34 is None:
            poses34 = poses34_from_angle_axis(self.cameras()[0])
        p = np.ascontiguousarray(poses34, np.float64)
        off = np.ascontiguousarray(trk_off, np.int32)
        cam = np.ascontiguousarray(obs_cam, np.int32)
        xy = np.ascontiguousarray(obs_xy, np.int32).reshape(-1, 2)
        n = len(off) - 1
        st = np.zeros(max(n, 1), np.uint8)
        first, added = C.c_int32(), C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_triangulate(self.h, p.ctypes.data, n, off.ctypes.data, cam.ctypes.data if len(cam) else None,
                                                               xy.ctypes.data if len(cam) else None, float(max_err), float(min_angle),
                                                               st.ctypes.data, C.byref(first), C.byref(added)))
        return st[:n], first.value, added.value

    def attach(self, cam, landmark, feat, xy, poses34=None, max_err=4.0):
        """Step 1 of triangulateMatchedLandmarks against the session's landmarks (rcn_ba_session_attach): entries (landmark,
        feature, xy) of camera `cam` in list order; attached ones are appended to their tracks.  Returns (status per entry:
        0 attached, 1 depth, 2 reprojection, 3 feature taken; number attached)."""
        if poses34 is None:
            poses34 = poses34_from_angle_axis(self.cameras()[0])
        p = np.ascontiguousarray(poses34, np.float64)
        lm, ft = np.ascontiguousarray(landmark, np.int32), np.ascontiguousarray(feat, np.int32)
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n = len(lm)
        st = np.zeros(max(n, 1), np.uint8)
        added = C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_attach(self.h, p.ctypes.data, int(cam), n, lm.ctypes.data if n else None,
                                                          ft.ctypes.data if n else None, xy.ctypes.data if n else None,
                                                          float(max_err), st.ctypes.data, C.byref(added)))
        return st[:n], added.value

    def grow_view(self, img, n_keypoints, registered, img_matches, cam_index, poses34=None, max_err=4.0, min_angle=1.0):
        """Step 3 of triangulateMatchedLandmarks for the new image `img` (n_keypoints features) on the device
        (rcn_ba_session_grow_view): the candidates from the resident lists and the landmark-id table (newview.LandmarkIds),
        triangulated straight into the session, the table committed with the new landmarks' indices.  registered /
        img_matches as triangulate.new_view_tracks takes them (filtered here), cam_index {image: session camera}.  Returns
        (trk_src[n_tracks, 3] = (reg image, its feature, feature of img), status per candidate, index of the first new
        landmark, landmarks added) -- what new_view_tracks -> tracks_to_arrays -> triangulate() gives on the same state."""
        from . import newview
        if poses34 is None:
            poses34 = poses34_from_angle_axis(self.cameras()[0])
        p = np.ascontiguousarray(poses34, np.float64)
        reg = np.asarray(newview.visited(img, registered, img_matches), np.int32)
        cam = np.asarray([cam_index[r] for r in reg], np.int32)
        K = int(n_keypoints)
        newview.LandmarkIds(self.ctx).read(img, K)          # raises unless img has exactly K keypoints: the arrays below have room
        src, st = np.zeros((max(K, 1), 3), np.int32), np.zeros(max(K, 1), np.uint8)
        n, first, added = C.c_int32(), C.c_int32(), C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_grow_view(self.h, p.ctypes.data, int(img), int(cam_index[img]), len(reg),
                                                             reg.ctypes.data if len(reg) else None, cam.ctypes.data if len(reg) else None,
                                                             float(max_err), float(min_angle), C.byref(n), src.ctypes.data, st.ctypes.data,
                                                             C.byref(first), C.byref(added)))
        return src[:n.value], st[:n.value], first.value, added.value

    def pnp(self, landmark, xy, intr6, options=None):
        """registerImagePnP of one view against the session's landmarks in HBM (rcn_ba_session_pnp): entries (landmark,
        integer pixel) in list order.  Returns (pose34[12], inlier mask, count); count < 0: no pose (pnp.pnp_ransac)."""
        lm = np.ascontiguousarray(landmark, np.int32)
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        K = np.ascontiguousarray(intr6, np.float64).reshape(6)
        n = len(lm)
        pose, mask, cnt = np.zeros(12), np.zeros(max(n, 1), np.uint8), C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_pnp(self.h, n, lm.ctypes.data if n else None, xy.ctypes.data if n else None,
                                                       K.ctypes.data, C.byref(options) if options is not None else None,
                                                       pose.ctypes.data, mask.ctypes.data, C.byref(cnt)))
        return pose, mask[:n], cnt.value

    def init_pair(self, xy1, xy2, intr6_1, intr6_2, options=None, max_err=4.0, min_angle=1.0):
        """chooseInitialPair + triangulateInitialPair into this (empty) session (rcn_ba_session_init_pair): the two-view search
        on the pair's entries (integer pixels in ascending query-feature order), cameras 0 (the identity) and 1 (the
        recovered pose), every entry triangulated as a two-observation track.  Returns twoview.two_view_init's dict for the
        one pair plus status (the triangulation's, per entry) and added; count[0] < 0: no pose, the session stays empty."""
        xy1 = np.ascontiguousarray(xy1, np.int32).reshape(-1, 2)
        xy2 = np.ascontiguousarray(xy2, np.int32).reshape(-1, 2)
        K1 = np.ascontiguousarray(intr6_1, np.float64).reshape(6)
        K2 = np.ascontiguousarray(intr6_2, np.float64).reshape(6)
        n = len(xy1)
        if len(xy2) != n:
            raise ValueError("init_pair: xy1 and xy2 differ in length")
        out = dict(E=np.zeros(9), pose34=np.zeros(12), mask=np.zeros(max(n, 1), np.uint8), cheir_mask=np.zeros(max(n, 1), np.uint8),
                   count=np.zeros(2, np.int32), iterations=np.zeros(1, np.int32), status=np.zeros(max(n, 1), np.uint8))
        added = C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_init_pair(self.h, n, xy1.ctypes.data if n else None, xy2.ctypes.data if n else None,
                                                             K1.ctypes.data, K2.ctypes.data, C.byref(options) if options is not None else None,
                                                             float(max_err), float(min_angle), out["E"].ctypes.data, out["pose34"].ctypes.data,
                                                             out["mask"].ctypes.data, out["cheir_mask"].ctypes.data, out["count"].ctypes.data,
                                                             out["iterations"].ctypes.data, out["status"].ctypes.data, C.byref(added)))
        for k in ("mask", "cheir_mask", "status"):
            out[k] = out[k][:n]
        out["added"] = added.value
        return out

    def remove_outliers(self):
        npts = self.counts()[1]
        new_idx = np.zeros(max(1, npts), np.int32)
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.rcn_ba_session_remove_outliers(self.h, new_idx.ctypes.data, C.byref(n)))
        return new_idx[:npts], n.value


def smoke(ctx):
    """Small solve on the GPU checked against nothing but itself converging (used by
    __graft_entry__.smoke together with the oracle comparison there)."""
    from . import synth_ba
    sc = synth_ba.make_scene(12, 300, seed=5)
    P, I, X, s = solve_scene(ctx, sc)
    assert s["final_rms_px"] < 1.0 < s["initial_rms_px"], s
    return sc, (P, I, X, s)


def smoke_local(ctx):
    """A local adjustment on the GPU: the last camera of a 12-camera session and the three that share the most landmarks with it are
    freed, the sub-problem is cut out on the device, solved with the other cameras constant and scattered back.  Checked against
    itself: the cost falls, the cameras outside the window and the landmarks the window does not see keep their bits."""
    from . import synth_ba
    sc = synth_ba.make_scene(12, 300, obs_per_point=4, seed=5)
    ses = BaSession(ctx)
    try:
        for p, k in zip(sc["poses"], sc["intrinsics"]):
            ses.add_camera(p, k)
        ses.add_points(sc["points"])
        ses.add_observations(sc["obs_pt"], sc["obs_cam"], sc["obs_uv"].astype(np.int32))
        near, counts = ses.covisible(11, 3)
        free = np.concatenate([[11], near])
        P0, X0 = ses.cameras()[0], ses.points()
        o = default_options(ctx, len(free))
        o.fix_cam0_pose = o.fix_cam1_translation = 0
        s, info = ses.solve_local(free, o)
        P1, X1 = ses.cameras()[0], ses.points()
        held = np.setdiff1d(np.arange(12), free)
        seen = np.zeros(300, bool)
        seen[sc["obs_pt"][np.isin(sc["obs_cam"], free)]] = True
        assert len(near) == 3 and counts[11] == (sc["obs_cam"] == 11).sum()
        assert s["final_cost"] < s["initial_cost"] and info["n_points"] == seen.sum() and info["n_constant"] == info["n_cams"] - 4, (s, info)
        assert P1[held].tobytes() == P0[held].tobytes() and X1[~seen].tobytes() == X0[~seen].tobytes() and (~seen).any()
        assert not np.array_equal(P1[free], P0[free]) and not np.array_equal(X1[seen], X0[seen])
        return info, s
    finally:
        ses.close()
