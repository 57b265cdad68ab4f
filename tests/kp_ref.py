"""CPU reference of the keypoint stage, written from its description and independent of the HIP
code: (a) extractHeatMap as the reference writes it, in torch fp32; (b) its float64 restatement (and the softmax mode's);
(c) threshold, greedy nmsFast in the canonical order, border filter and the cap.  Shared by the CPU and GPU keypoint tests."""
import numpy as np

R31 = (1 << 31) - 1


def depth_to_space(h64):
    """[64][Hc][Wc] -> [8 Hc][8 Wc]: heat[8 yc + c // 8][8 xc + c % 8] = h[c][yc][xc]."""
    _, Hc, Wc = h64.shape
    return np.ascontiguousarray(h64.reshape(8, 8, Hc, Wc).transpose(2, 0, 3, 1).reshape(8 * Hc, 8 * Wc))


def heat_as_written(logits):
    """(a) extractHeatMap (FeatureSuperPoint.cpp:95-140) statement by statement, torch fp32: every row of every plane is
    divided by the sum of the WHOLE plane as modified so far, + 1e-5."""
    import torch
    dense = torch.exp(torch.from_numpy(np.ascontiguousarray(logits, np.float32)))
    for d in range(dense.shape[0]):
        for r in range(dense.shape[1]):
            s = torch.sum(dense[d]) + 1e-5
            dense[d][r] /= s
    return depth_to_space(dense[:64].numpy())


def heat_reference_f64(logits):
    """(b) the same without the data dependence, in float64 throughout: S_r = sum_{k<r} R_k / S_k + sum_{k>=r} R_k + 1e-5."""
    e = np.exp(np.asarray(logits, np.float64))[:64]
    R = e.sum(axis=2)                                   # [64][Hc]
    Hc = R.shape[1]
    suf = np.cumsum(R[:, ::-1], axis=1)[:, ::-1]
    S = np.zeros_like(R)
    pre = np.zeros(64)
    for r in range(Hc):
        S[:, r] = pre + suf[:, r] + 1e-5
        pre = pre + R[:, r] / S[:, r]
    return depth_to_space(e / S[:, :, None])


def heat_softmax_f64(logits):
    """(b) for the softmax mode: softmax over the 65 channels of a cell, channel 64 dropped."""
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=0, keepdims=True))
    return depth_to_space((e / e.sum(axis=0, keepdims=True))[:64])


def keys_of(heat, conf_thresh):
    """Candidates of a heat map: (raster indices ascending, their 64-bit keys).  Candidate iff (double)heat >= thresh (a NaN
    never is); key = (fp32 bits << 32) | (2^31 - 1 - raster), a larger key comes earlier."""
    heat = np.ascontiguousarray(heat, np.float32)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(heat.astype(np.float64).ravel() >= conf_thresh)
    bits = heat.ravel().view(np.uint32)[cand].astype(np.uint64)
    return cand, (bits << np.uint64(32)) | (np.uint64(R31) - cand.astype(np.uint64))


def nms_greedy(heat, conf_thresh=0.015, nms_radius=4, border=4, K=None):
    """(c) processKeypoints behind the heat map: nmsFast walked in the canonical order (an alive candidate kills every other
    candidate within Chebyshev distance nms_radius, a killed one kills nothing), removeBorderKeypoints, then the cap: the K
    largest keys.  Returns (xy[K][2] int32, conf[K] float32, count): raster order, padding (-1, -1) / 0, count uncapped.
    K None: no cap, arrays as long as the count."""
    heat = np.ascontiguousarray(heat, np.float32)
    H, W = heat.shape
    cand, key = keys_of(heat, conf_thresh)
    alive = np.zeros((H, W), bool)
    alive.ravel()[cand] = True
    r = nms_radius
    for q in cand[np.argsort(key)[::-1]]:
        y, x = divmod(int(q), W)
        if alive[y, x]:
            alive[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = False
            alive[y, x] = True
    ys, xs = np.nonzero(alive)
    ok = ~((xs < border) | (xs >= W - border) | (ys < border) | (ys >= H - border))
    ys, xs = ys[ok], xs[ok]
    count = len(ys)
    if K is None:
        K = count
    if count > K:
        q = ys.astype(np.int64) * W + xs
        k = (heat[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(R31) - q.astype(np.uint64))
        top = np.sort(np.argsort(k)[::-1][:K])
        ys, xs = ys[top], xs[top]
    xy = np.full((K, 2), -1, np.int32)
    conf = np.zeros(K, np.float32)
    m = len(ys)
    xy[:m, 0], xy[:m, 1] = xs, ys
    conf[:m] = heat[ys, xs]
    return xy, conf, count


def nms_fixed_point(heat, conf_thresh=0.015, nms_radius=4):
    """The parallel form of nmsFast, transcribed on its own: a candidate is kept once every larger key in its window is
    suppressed, suppressed once any of them is kept; all candidates decide together from the state of the last round.
    Returns (kept[H][W] bool, rounds)."""
    heat = np.ascontiguousarray(heat, np.float32)
    H, W = heat.shape
    cand, key = keys_of(heat, conf_thresh)
    r = nms_radius
    keyp = np.zeros((H + 2 * r, W + 2 * r), np.uint64)                # key 0: no candidate (a real key is > 0 while raster < 2^31 - 1)
    und = np.zeros((H + 2 * r, W + 2 * r), bool)
    kept = np.zeros_like(und)
    inner = (slice(r, r + H), slice(r, r + W))
    kk = np.zeros(H * W, np.uint64)
    kk[cand] = key
    keyp[inner] = kk.reshape(H, W)
    uu = np.zeros(H * W, bool)
    uu[cand] = True
    und[inner] = uu.reshape(H, W)
    rounds = 0
    while und.any():
        larger_kept = np.zeros((H, W), bool)
        larger_und = np.zeros((H, W), bool)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                if dy == r and dx == r:
                    continue
                sl = (slice(dy, dy + H), slice(dx, dx + W))
                larger = keyp[sl] > keyp[inner]
                larger_kept |= larger & kept[sl]
                larger_und |= larger & und[sl]
        u = und[inner]
        new_kept = u & ~larger_kept & ~larger_und
        decided = u & (larger_kept | new_kept)
        kept[inner] |= new_kept
        und[inner] &= ~decided
        rounds += 1
    return kept[inner].copy(), rounds


def named_maps():
    """The four maps of the issue's table: name -> (heat[H][W] float32, conf_thresh)."""
    rng = np.random.default_rng(7)
    lg = (1.2 * rng.standard_normal((65, 15, 20))).astype(np.float32)
    out = {"random": (heat_as_written(lg), 0.015)}
    out["dense"] = (rng.random((64, 96), dtype=np.float32) + np.float32(0.5), 0.015)
    out["ties"] = ((rng.integers(0, 6, (64, 96)) / 8.0 + 0.125).astype(np.float32), 0.015)
    out["ramp"] = ((np.arange(64 * 96, dtype=np.float32).reshape(64, 96) + 1) / np.float32(64 * 96), 0.0)
    return out
