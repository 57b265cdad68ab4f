"""CPU restatements of batched multi-view triangulation (csrc/triangulate.hip), for the tests only.

canonical_*   the kernel's exact operation sequence in Python floats (IEEE doubles; math.sqrt is correctly rounded):
              Givens QR of A row by row, cyclic one-sided Jacobi on R, the three rules.  X agrees with the device bit for
              bit; a status may differ only where acos decides a track at exactly the angle threshold.
numpy_*       the reference's own steps (SequentialReconstructor.cpp:396-489) with numpy.linalg.svd(A) for the null
              vector: an independent check of the mathematics, equal to the canonical X to rounding.
sequential_*  triangulateInitialPair (:377-394) and triangulateMatchedLandmarks (:492-556) as the reference runs them --
              one triangulateMultiView call at a time, landmarkId updated between the calls -- over plain containers.
"""
import math

import numpy as np

SWEEPS = 20
JACOBI_TOL = 1e-15


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(a):
    return math.nan if a != a else math.sqrt(a)


def _acos(a):
    return math.nan if (a != a or a > 1.0 or a < -1.0) else math.acos(a)


# ---- the kernel's operation sequence ------------------------------------------------------------------------------

def cam_centre(P):
    """-R't (camgeom.h k_cam_centres)."""
    return [((-P[i]) * P[3] + (-P[4 + i]) * P[7]) + (-P[8 + i]) * P[11] for i in range(3)]


def reproj_l1(P, K, X, ox, oy):
    """camgeom.h reproj_l1: (L1 error, camera-frame depth)."""
    l = [((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3] for i in range(3)]
    x, y = _div(l[0], l[2]), _div(l[1], l[2])
    radius = x * x + y * y
    d = K[4] * radius + (K[5] * radius) * radius
    x += d
    y += d
    u, v = K[0] * x + K[2], K[1] * y + K[3]
    return abs(u - float(ox)) + abs(v - float(oy)), l[2]


def tri_angle(X, c1, c2):
    """camgeom.h tri_angle: 180 acos(r1.r2 / (|r1| |r2|)) / 3.1415."""
    r1 = [X[0] - c1[0], X[1] - c1[1], X[2] - c1[2]]
    r2 = [X[0] - c2[0], X[1] - c2[1], X[2] - c2[2]]
    n1 = _sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2])
    n2 = _sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2])
    dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2]
    return _div(180.0 * _acos(_div(dot, n1 * n2)), 3.1415)


def dlt_rows(P, K, ox, oy):
    x = _div(float(ox) - K[2], K[0])
    y = _div(float(oy) - K[3], K[1])
    radius = x * x + y * y
    d = K[4] * radius + (K[5] * radius) * radius
    x -= d
    y -= d
    return [x * P[8 + c] - P[c] for c in range(4)], [y * P[8 + c] - P[4 + c] for c in range(4)]


def givens_row(R, a):
    for k in range(4):
        if a[k] != 0.0:
            rho = _sqrt(R[k][k] * R[k][k] + a[k] * a[k])
            c, s = _div(R[k][k], rho), _div(a[k], rho)
            R[k][k] = rho
            for j in range(k + 1, 4):
                rk = R[k][j]
                R[k][j] = c * rk + s * a[j]
                a[j] = c * a[j] - s * rk
            a[k] = 0.0


def _col_dot(W, p, q):
    return ((W[0][p] * W[0][q] + W[1][p] * W[1][q]) + W[2][p] * W[2][q]) + W[3][p] * W[3][q]


def jacobi_min(W):
    """Returns (smallest column norm, the column of V that belongs to it)."""
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                alpha, beta, gamma = _col_dot(W, p, p), _col_dot(W, q, q), _col_dot(W, p, q)
                if not (abs(gamma) > JACOBI_TOL * _sqrt(alpha * beta)):
                    continue
                zeta = _div(beta - alpha, 2.0 * gamma)
                t = _div(1.0 if zeta >= 0.0 else -1.0, abs(zeta) + _sqrt(1.0 + zeta * zeta))
                c = _div(1.0, _sqrt(1.0 + t * t))
                s = c * t
                for i in range(4):
                    wp, wq = W[i][p], W[i][q]
                    W[i][p] = c * wp - s * wq
                    W[i][q] = s * wp + c * wq
                    vp, vq = V[i][p], V[i][q]
                    V[i][p] = c * vp - s * vq
                    V[i][q] = s * vp + c * vq
                rotated = True
        if not rotated:
            break
    smin, jm = _sqrt(_col_dot(W, 0, 0)), 0
    for j in range(1, 4):
        sj = _sqrt(_col_dot(W, j, j))
        if sj < smin:
            smin, jm = sj, j
    return smin, [V[i][jm] for i in range(4)]


def canonical_track(Ps, Ks, xys, centres, max_err=4.0, min_angle=1.0):
    """One track: Ps / Ks / centres per observation (lists of floats), xys integer pixels.  Returns (X, status)."""
    R = [[0.0] * 4 for _ in range(4)]
    for P, K, (ox, oy) in zip(Ps, Ks, xys):
        a, b = dlt_rows(P, K, ox, oy)
        givens_row(R, a)
        givens_row(R, b)
    sigma, v = jacobi_min(R)
    X = [_div(v[0], v[3]), _div(v[1], v[3]), _div(v[2], v[3])]
    k = len(xys)
    st = 0
    if k < 2 or not (sigma != 0.0 and X[2] > 0.0):
        st = 1
    if st == 0:
        for P, K, (ox, oy) in zip(Ps, Ks, xys):
            if reproj_l1(P, K, X, ox, oy)[0] > max_err:
                st = 2
                break
    if st == 0:
        for p in range(k):
            if any(tri_angle(X, centres[p], centres[q]) < min_angle for q in range(p + 1, k)):
                st = 3
                break
    return X, st


def canonical_tracks(poses34, intrinsics, trk_off, obs_cam, obs_xy, max_err=4.0, min_angle=1.0):
    """The whole CSR batch: (xyz[n, 3], status[n] uint8), as rcn_triangulate returns them."""
    P = [[float(v) for v in row] for row in np.asarray(poses34, np.float64).reshape(-1, 12)]
    K = [[float(v) for v in row] for row in np.asarray(intrinsics, np.float64).reshape(-1, 6)]
    C = [cam_centre(p) for p in P]
    off = np.asarray(trk_off, np.int64)
    cam = np.asarray(obs_cam).tolist()
    xy = np.asarray(obs_xy, np.int64).reshape(-1, 2).tolist()
    n = len(off) - 1
    xyz = np.zeros((n, 3))
    st = np.zeros(n, np.uint8)
    for j in range(n):
        o = range(int(off[j]), int(off[j + 1]))
        X, s = canonical_track([P[cam[i]] for i in o], [K[cam[i]] for i in o], [xy[i] for i in o], [C[cam[i]] for i in o],
                               max_err, min_angle)
        xyz[j] = X
        st[j] = s
    return xyz, st


# ---- the reference's steps with numpy's SVD -------------------------------------------------------------------------

def numpy_tracks(poses34, intrinsics, trk_off, obs_cam, obs_xy, max_err=4.0, min_angle=1.0):
    """SequentialReconstructor.cpp:396-489 with numpy.linalg.svd(A) (tracks of one length batched together)."""
    P = np.asarray(poses34, np.float64).reshape(-1, 3, 4)
    K = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    off = np.asarray(trk_off, np.int64)
    cam = np.asarray(obs_cam, np.int64)
    xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    n = len(off) - 1
    xyz = np.zeros((n, 3))
    st = np.zeros(n, np.uint8)
    lens = np.diff(off)
    centres = -np.einsum("cji,cj->ci", P[:, :, :3], P[:, :, 3])
    with np.errstate(all="ignore"):
        for L in np.unique(lens):
            tr = np.flatnonzero(lens == L)
            idx = off[tr][:, None] + np.arange(L)[None, :]                       # (m, L)
            c, Kc = cam[idx], K[cam[idx]]
            x = (xy[idx, 0] - Kc[..., 2]) / Kc[..., 0]
            y = (xy[idx, 1] - Kc[..., 3]) / Kc[..., 1]
            r = x * x + y * y
            d = Kc[..., 4] * r + Kc[..., 5] * r * r
            x, y = x - d, y - d
            Pc = P[c]                                                            # (m, L, 3, 4)
            A = np.empty((len(tr), 2 * L, 4))
            A[:, 0::2] = x[..., None] * Pc[:, :, 2] - Pc[:, :, 0]
            A[:, 1::2] = y[..., None] * Pc[:, :, 2] - Pc[:, :, 1]
            _, s, vt = np.linalg.svd(A)
            v = vt[:, -1]
            X = v[:, :3] / v[:, 3:4]
            s4 = s[:, 3]
            ok = (s4 != 0) & (X[:, 2] > 0)
            loc = np.einsum("mlij,mj->mli", Pc[..., :3], X) + Pc[..., 3]
            px, py = loc[..., 0] / loc[..., 2], loc[..., 1] / loc[..., 2]
            rr = px * px + py * py
            dd = Kc[..., 4] * rr + Kc[..., 5] * rr * rr
            u, w = Kc[..., 0] * (px + dd) + Kc[..., 2], Kc[..., 1] * (py + dd) + Kc[..., 3]
            bad_rep = (np.abs(u - xy[idx, 0]) + np.abs(w - xy[idx, 1]) > max_err).any(1)
            ray = X[:, None, :] - centres[c]                                     # (m, L, 3)
            nr = np.linalg.norm(ray, axis=2)
            cos = np.einsum("mpi,mqi->mpq", ray, ray) / (nr[:, :, None] * nr[:, None, :])
            ang = 180.0 * np.arccos(cos) / 3.1415
            off_diag = ~np.eye(L, dtype=bool)
            bad_ang = ((ang < min_angle) & off_diag[None]).any((1, 2))
            xyz[tr] = X
            st[tr] = np.where(~ok, 1, np.where(bad_rep, 2, np.where(bad_ang, 3, 0)))
    return xyz, st


# ---- the reference's loops, one triangulateMultiView at a time ----------------------------------------------------

def triangulate_multi_view(track, coords, landmark_ids, landmarks, poses34, intrinsics, max_err=4.0, min_angle=1.0):
    """:396-489 for one track [(img, feat), ...] over containers: coords[img][feat] = (x, y), landmark_ids[img][feat],
    poses34[img] (12), intrinsics[img] (6); appends {"xyz", "track"} to landmarks and sets the landmarkIds if accepted."""
    Ps = [[float(v) for v in poses34[i]] for i, _ in track]
    Ks = [[float(v) for v in intrinsics[i]] for i, _ in track]
    X, st = canonical_track(Ps, Ks, [coords[i][f] for i, f in track], [cam_centre(p) for p in Ps], max_err, min_angle)
    if st == 0:
        for i, f in track:
            landmark_ids[i][f] = len(landmarks)
        landmarks.append({"xyz": X, "track": list(track)})
    return st


def sequential_initial_pair(img1, img2, feature_matches, coords, landmark_ids, landmarks, poses34, intrinsics, **kw):
    """:377-394: every match of featureMatches[(img1, img2)], in its iteration order."""
    for f1, f2 in feature_matches[(img1, img2)].items():
        triangulate_multi_view([(img1, f1), (img2, f2)], coords, landmark_ids, landmarks, poses34, intrinsics, **kw)


def sequential_matched_landmarks(img, feature_ids, landmark_idxs, registered, img_matches, feature_matches, coords,
                                 landmark_ids, landmarks, poses34, intrinsics, max_err=4.0, min_angle=1.0):
    """:492-556, literally.  registered: [(image, status)] in registeredImages' iteration order."""
    P, K = poses34[img], intrinsics[img]
    for f, lid in zip(feature_ids, landmark_idxs):                                  # step 1, :497-512 (note the <)
        X = landmarks[lid]["xyz"]
        err, depth = reproj_l1([float(v) for v in P], [float(v) for v in K], X, *coords[img][f])
        if depth > 0 and err < max_err and landmark_ids[img][f] == -1:
            landmarks[lid]["track"].append((img, f))
            landmark_ids[img][f] = lid
    for f in range(len(landmark_ids[img])):                                         # step 3, :518-553
        if landmark_ids[img][f] != -1:
            continue
        for reg, status in registered:
            if status and reg in img_matches[img]:
                pm = feature_matches.get((img, reg), {})
                if f in pm:
                    g = pm[f]
                    if landmark_ids[reg][g] == -1:
                        triangulate_multi_view([(reg, g), (img, f)], coords, landmark_ids, landmarks, poses34, intrinsics,
                                               max_err, min_angle)
                        break


# ---- seeded inputs (synth_ba scenes, camera 0 at the identity as the reference sets it, :1018) -----------------------

def _reframe(poses6, points):
    """World frame of camera 0: poses34 with camera 0 = [I | 0], points mapped along (observations do not change)."""
    from reconstructor_amd import synth_ba
    P = synth_ba.poses_to_34(poses6).reshape(-1, 3, 4)
    R0, t0 = P[0, :, :3].copy(), P[0, :, 3].copy()
    out = np.empty_like(P)
    out[:, :, :3] = P[:, :, :3] @ R0.T
    out[:, :, 3] = P[:, :, 3] - out[:, :, :3] @ t0
    out[0] = np.eye(3, 4)
    return out.reshape(-1, 12), points @ R0.T + t0


def make_tracks(n_cams, n_tracks, min_len=2, max_len=2, seed=0, defect_rate=0.0, distortion=False):
    """A CSR batch of tracks of min_len .. max_len observations (in random camera order) of a synth_ba scene, integer
    pixels with 0.5 px noise.  defect_rate > 0: some observations displaced by up to 5 px, some points far out along
    their rays (narrow angles) or mirrored through the scene centre (world z <= 0 for some)."""
    from reconstructor_amd import synth_ba
    k = min(max_len, n_cams)
    sc = synth_ba.make_scene(n_cams, n_tracks, obs_per_point=k, seed=seed)
    rng = np.random.default_rng(seed + 77)
    pts, intr = sc["points_gt"].copy(), sc["intr_gt"].copy()
    if distortion:
        intr[rng.random(n_cams) < 0.3, 4:] = rng.normal(0, 1e-3, 2)
    cam = rng.permuted(sc["obs_cam"].reshape(n_tracks, k), axis=1)
    if defect_rate:
        far = rng.random(n_tracks) < defect_rate / 2
        pts[far] *= rng.choice([30.0, 300.0, -4.0], (far.sum(), 1))
    uv, _ = synth_ba.project(sc["poses_gt"][cam.reshape(-1)], intr[cam.reshape(-1)], np.repeat(pts, k, axis=0))
    uv = uv + 0.5 * rng.standard_normal(uv.shape)
    if defect_rate:
        bump = rng.random(len(uv)) < defect_rate / 2
        uv[bump] += rng.uniform(-5, 5, (bump.sum(), 2))
    xy = np.trunc(np.nan_to_num(uv, nan=0.0, posinf=1e6, neginf=-1e6)).clip(-1e6, 1e6).astype(np.int32)
    length = rng.integers(min_len, k + 1, n_tracks) if min_len < k else np.full(n_tracks, k)
    sel = (np.arange(k)[None, :] < length[:, None]).reshape(-1)
    poses34, pts = _reframe(sc["poses_gt"], pts)
    return {"poses34": poses34, "intrinsics": intr, "trk_off": np.concatenate([[0], np.cumsum(length)]).astype(np.int32),
            "obs_cam": np.ascontiguousarray(cam.reshape(-1)[sel].astype(np.int32)), "obs_xy": np.ascontiguousarray(xy[sel]),
            "points_gt": pts}


def loop_containers(n_images, n_points, obs_per_point=6, seed=0, wrong_rate=0.03):
    """The reference's containers for a synth_ba scene: coords[img][feat], landmark_ids[img][feat] (all -1),
    poses34[img] / intrinsics[img] (camera 0 at the identity), feature_matches[(i, j)] = {feat of i: feat of j} for
    every pair that shares points (the inverse map under (j, i), injective; a few partners swapped so that some tracks
    fail the reprojection rule), img_matches[i] = every other image.  Also point_of[img][feat] (scene point) and poses6
    (angle-axis, translation per image: the same poses as rcn_ba_problem wants them)."""
    from reconstructor_amd import synth_ba
    sc = synth_ba.make_scene(n_images, n_points, obs_per_point=obs_per_point, seed=seed)
    rng = np.random.default_rng(seed + 5)
    poses34, _ = _reframe(sc["poses_gt"], sc["points_gt"])
    poses6 = np.array([np.concatenate([synth_ba.rot_to_angle_axis(p.reshape(3, 4)[:, :3]), p.reshape(3, 4)[:, 3]]) for p in poses34])
    xy = sc["obs_uv"].astype(np.int64)
    coords, point_of = {}, {}
    for i in range(n_images):
        o = np.flatnonzero(sc["obs_cam"] == i)
        o = o[rng.permutation(len(o))]
        coords[i] = [(int(xy[q, 0]), int(xy[q, 1])) for q in o]
        point_of[i] = [int(sc["obs_pt"][q]) for q in o]
    feat_of = [{p: f for f, p in enumerate(point_of[i])} for i in range(n_images)]
    feature_matches = {}
    for i in range(n_images):
        for j in range(i + 1, n_images):
            common = [p for p in point_of[i] if p in feat_of[j]]
            if not common:
                continue
            q = [feat_of[i][p] for p in common]
            t = [feat_of[j][p] for p in common]
            for a in range(len(t) - 1):
                if rng.random() < wrong_rate:
                    t[a], t[a + 1] = t[a + 1], t[a]
            order = rng.permutation(len(q))
            feature_matches[(i, j)] = {q[a]: t[a] for a in order}
            feature_matches[(j, i)] = {t[a]: q[a] for a in order}
    return {"coords": coords, "point_of": point_of, "landmark_ids": {i: [-1] * len(coords[i]) for i in range(n_images)},
            "poses34": {i: poses34[i] for i in range(n_images)}, "poses6": poses6, "intrinsics": {i: sc["intr_gt"][i] for i in range(n_images)},
            "feature_matches": feature_matches, "img_matches": {i: [j for j in range(n_images) if j != i] for i in range(n_images)}}


def calc_2d3d_matches(img, img_matches, feature_matches, landmark_ids, landmarks):
    """calc2d3dMatches (:654-679) for one candidate image: (featureIds, landmarkIds), a feature possibly twice."""
    fids, lids = [], []
    for lid, lm in enumerate(landmarks):
        for i, f in lm["track"]:
            if i in img_matches[img]:
                pm = feature_matches.get((i, img), {})
                if f in pm and landmark_ids[img][pm[f]] == -1:
                    fids.append(pm[f])
                    lids.append(lid)
    return fids, lids
