"""Ray-cast scenes for the plane sweep: pinhole views of one textured plane, rendered on the host.

    cameras       n cameras along a baseline, camera 0 at the origin looking down +z, the others shifted and slightly rotated
    render        the bytes every camera sees of the plane n . X = d, textured with a sum of twelve sinusoids over its world (x, y)
    wall_depths   the true camera-frame depth of every pixel of a view
    wall_scene    cameras + images + RGB planes in one call

Host code only (numpy); the tests, the smoke run and tools/mvs_timing.py share it.
"""
import numpy as np


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def cameras(n, rows, cols, f=100.0, baseline=0.35, seed=0, k1=0.0, k2=0.0):
    """(poses34 [n][12] rows of [R | t] world -> camera, intrinsics [n][6] = fx fy cx cy k1 k2).  Camera 0 is the identity; camera
    i sits about i * baseline away along x (alternating sides, a little y and z) with a few hundredths of a radian of rotation."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 12))
    for i in range(n):
        if i == 0:
            R, C = np.eye(3), np.zeros(3)
        else:
            side = 1.0 if i % 2 else -1.0
            C = np.array([side * baseline * ((i + 1) // 2), 0.1 * baseline * rng.standard_normal(), 0.05 * baseline * rng.standard_normal()])
            R = _rot(*(0.03 * rng.standard_normal(3)))
        poses[i] = np.c_[R, -R @ C].reshape(12)
    intr = np.tile(np.array([f, f, (cols - 1) / 2.0, (rows - 1) / 2.0, k1, k2]), (n, 1))
    return poses, intr


_TEX = None


def _texture(x, y):
    global _TEX
    if _TEX is None:
        rng = np.random.default_rng(12)
        _TEX = (rng.uniform(2.0, 14.0, 12), rng.uniform(0, 2 * np.pi, 12), rng.uniform(0, 2 * np.pi, 12), rng.uniform(0.5, 1.0, 12))
    freq, ang, ph, amp = _TEX
    t = np.zeros_like(x)
    for f, a, p, m in zip(freq, ang, ph, amp):
        t += m * np.sin(f * (np.cos(a) * x + np.sin(a) * y) + p)
    return t / amp.sum()


def _hits(pose, intr, rows, cols, normal, d):
    """World points and camera-frame depths where the pixel rays of one pinhole camera meet the plane normal . X = d."""
    R, t = pose.reshape(3, 4)[:, :3], pose.reshape(3, 4)[:, 3]
    C = -R.T @ t
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    dirs = np.stack([(xs - intr[2]) / intr[0], (ys - intr[3]) / intr[1], np.ones_like(xs)], -1)        # camera frame, z = 1
    wd = dirs @ R                                                                                        # R^T dir
    s = (d - normal @ C) / (wd @ normal)                                                                 # the camera-frame depth
    return C + wd * s[..., None], s


def render(poses, intr, rows, cols, normal=(0.0, 0.0, 1.0), d=5.0, channels=1):
    """uint8 [n][rows][cols] (or [n][rows][cols][3]: three differently scaled copies of the texture) of the plane normal . X = d."""
    normal = np.asarray(normal, np.float64)
    out = []
    for P, K in zip(poses, intr):
        X, s = _hits(P, K, rows, cols, normal, d)
        t = _texture(X[..., 0], X[..., 1])
        g = np.where(s > 0, np.clip(np.floor(127.5 + 127.5 * t + 0.5), 0, 255), 0).astype(np.uint8)
        if channels == 1:
            out.append(g)
        else:
            out.append(np.stack([g, 255 - g, (g.astype(np.int32) * 3 // 4 + 20).astype(np.uint8)], -1))
    return np.stack(out)


def wall_depths(pose, intr, rows, cols, normal=(0.0, 0.0, 1.0), d=5.0):
    return _hits(pose, intr, rows, cols, np.asarray(normal, np.float64), d)[1]


def wall_scene(n=4, rows=72, cols=96, f=100.0, normal=(0.0, 0.0, 1.0), d=5.0, seed=0, baseline=0.35):
    """dict(poses34, intrinsics, gray [n][rows][cols], rgb [n][rows][cols][3], normal, d)."""
    poses, intr = cameras(n, rows, cols, f, baseline, seed)
    rgb = render(poses, intr, rows, cols, normal, d, channels=3)
    return dict(poses34=poses, intrinsics=intr, gray=np.ascontiguousarray(rgb[..., 0]), rgb=rgb, normal=np.asarray(normal, np.float64), d=float(d))
