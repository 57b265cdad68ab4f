"""Writes tests/golden/keypoints_small.npz: network logits for 3 images of 120 x 160 and the keypoints the reference's
own arithmetic gives for them -- heat map (a) of tests/kp_ref.py (extractHeatMap as written, torch fp32) followed by (c)
(threshold 0.015, greedy nmsFast radius 4 in the canonical order, border 4), no cap.

The heat stage of the GPU path is not bit-exact, so the input is chosen with a guard band, asserted on the float64
restatement (b): no heat value within relative 2^-18 of the threshold, and no two candidates inside one NMS window whose
confidences differ by less than relative 2^-18 without being bit-equal in (a).  The first seed for which this holds is
used: a condition on the input, not on any code under test."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kp_ref  # noqa: E402

N, H, W = 3, 120, 160
THRESH, RADIUS, BORDER = 0.015, 4, 4
BAND = 2.0 ** -18


def guard_band(a, b):
    """(threshold gap, window gap): the smallest relative distances that the band bounds; inf when nothing is near."""
    thr_gap = np.min(np.abs(b - THRESH) / THRESH)
    cand = b >= THRESH
    win_gap = np.inf
    bits = a.view(np.uint32)
    r = RADIUS
    for dy in range(0, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx <= 0:
                continue
            y0, y1 = 0, H - dy
            x0, x1 = max(0, -dx), W - max(0, dx)
            s0 = (slice(y0, y1), slice(x0, x1))
            s1 = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            both = cand[s0] & cand[s1] & (bits[s0] != bits[s1])
            if both.any():
                rel = np.abs(b[s0] - b[s1]) / np.maximum(b[s0], b[s1])
                win_gap = min(win_gap, rel[both].min())
    return thr_gap, win_gap


def make(seed):
    rng = np.random.default_rng(seed)
    logits = (1.2 * rng.standard_normal((N, 65, H // 8, W // 8))).astype(np.float32)
    logits[1] *= np.float32(0.8)               # the three images differ in how many candidates they have
    logits[2, :64, 5:9] += np.float32(0.8)
    out, gaps = [], []
    for i in range(N):
        a, b = kp_ref.heat_as_written(logits[i]), kp_ref.heat_reference_f64(logits[i])
        gaps.append(guard_band(a, b))
        out.append(kp_ref.nms_greedy(a, THRESH, RADIUS, BORDER))
    return logits, out, gaps


if __name__ == "__main__":
    for seed in range(1, 100):
        logits, out, gaps = make(seed)
        if all(t >= BAND and w >= BAND for t, w in gaps):
            break
    else:
        raise SystemExit("no seed satisfies the guard band")
    assert all(t >= BAND and w >= BAND for t, w in gaps)
    counts = np.array([c for _, _, c in out], np.int32)
    K = int(counts.max())
    xy = np.full((N, K, 2), -1, np.int32)
    conf = np.zeros((N, K), np.float32)
    for i, (x, c, n) in enumerate(out):
        xy[i, :n], conf[i, :n] = x, c
    np.savez_compressed(os.path.join(HERE, "keypoints_small.npz"), logits=logits, xy=xy, conf=conf, counts=counts, seed=np.int32(seed),
                        conf_thresh=np.float64(THRESH), nms_radius=np.int32(RADIUS), border=np.int32(BORDER))
    print("seed %d: counts %s, nearest heat value %.2e relative from the threshold, nearest unequal pair in a window %.2e"
          % (seed, counts.tolist(), min(t for t, _ in gaps), min(w for _, w in gaps)))
