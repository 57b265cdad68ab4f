"""The contract of track building (rcn_tracks_*) in plain Python / numpy: what the GPU must equal bit for bit.

    nodes      one per (image, feature): the images of the lists ascending by id, feature 0 .. K[image] - 1; node = node_off + feature
    edges      every entry (f, g) of every list (a, b) joins (a, f) and (b, g); `mirror` is accepted and changes nothing
    rule 4     a component in which an image occurs with two or more features: DROP_TRACK drops it, DROP_IMAGE the observations of
               such images in it
    rule 5     select = (images, camera rows): observations of other images are dropped, after rule 4
    rule 6     a track is kept when min_length <= n and (max_length == 0 or n <= max_length), n the surviving observations
    order      observations ascend by node, tracks by their first surviving observation

build() returns the full result; truncate() what a call with capacities writes.  stats: components of at least 2 nodes, components
with a conflict, observations dropped by rule 4 (DROP_TRACK: every node of a conflicting component), components of at least 2 nodes
that rule 4 did not drop whole and rule 6 dropped, the largest component's nodes, the longest kept track, the edges, 0.
"""
import numpy as np

DROP_TRACK, DROP_IMAGE = 0, 1


def layout(pairs, K):
    """pairs [n, 2]; K {image: keypoints}.  Returns (img_ids ascending, node_off[n + 1] int64)."""
    ids = np.unique(np.asarray(pairs, np.int64).reshape(-1, 2)).astype(np.int32)
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum([int(K[int(i)]) for i in ids])
    return ids, off


def edge_nodes(pairs, offsets, qt, ids, node_off):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    qt = np.asarray(qt, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    if len(pairs) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    per = np.diff(offsets)
    sa = np.searchsorted(ids, pairs[:, 0])
    sb = np.searchsorted(ids, pairs[:, 1])
    return np.repeat(node_off[sa], per) + qt[:, 0], np.repeat(node_off[sb], per) + qt[:, 1]


def components(n, u, v):
    """root[x] = the smallest node of x's component (sequential union-find, the larger root under the smaller)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    return np.array([find(x) for x in range(n)], np.int64).reshape(n)


def build(pairs, offsets, qt, K, min_length=2, max_length=0, conflict=DROP_TRACK, select=None, coords=None, mirror=False):
    """Returns a dict: img_ids, node_off, counts[2], trk_off, obs_img, obs_feat, obs_cam (None without select), obs_xy (None without
    coords {image: [K, 2]}), feat_track[n_nodes], stats[8], tracks (a list of lists of (image, feature))."""
    if min_length < 2 or max_length < 0 or (0 < max_length < min_length) or conflict not in (DROP_TRACK, DROP_IMAGE):
        raise ValueError("bad options")
    del mirror
    ids, node_off = layout(pairs, K)
    ns, n = len(ids), int(node_off[-1])
    u, v = edge_nodes(pairs, offsets, qt, ids, node_off)
    root = components(n, u, v)
    slot = np.repeat(np.arange(ns, dtype=np.int64), np.diff(node_off))
    size = np.bincount(root, minlength=max(n, 1))[:max(n, 1)]
    comp2 = size[root] >= 2 if n else np.zeros(0, bool)
    _, inv, cnt = np.unique(root * max(ns, 1) + slot, return_inverse=True, return_counts=True)
    twice = cnt[inv.reshape(-1)] >= 2 if n else np.zeros(0, bool)
    cflag = np.zeros(max(n, 1), bool)
    cflag[root[twice]] = True
    dropped4 = comp2 & (cflag[root] if conflict == DROP_TRACK else twice)
    cam_of_slot = np.zeros(ns, np.int64)
    if select is not None:
        s_img, s_cam = np.asarray(select[0], np.int64).reshape(-1), np.asarray(select[1], np.int64).reshape(-1)
        if len(np.unique(s_img)) != len(s_img) or (s_cam < 0).any() or not np.isin(s_img, ids).all():
            raise ValueError("bad selection")
        cam_of_slot[:] = -1
        cam_of_slot[np.searchsorted(ids, s_img)] = s_cam
    alive = comp2 & ~dropped4 & (cam_of_slot[slot] >= 0)
    nsurv = np.bincount(root[alive], minlength=max(n, 1))[:max(n, 1)]
    len_ok = (nsurv >= min_length) & ((max_length == 0) | (nsurv <= max_length))
    nodes = np.nonzero(alive & len_ok[root])[0]
    first = np.full(max(n, 1), n, np.int64)
    np.minimum.at(first, root[nodes], nodes)
    nodes = nodes[np.lexsort((nodes, first[root[nodes]]))]
    heads = np.nonzero(first[root[nodes]] == nodes)[0]              # positions of the tracks' first observations
    trk_off = np.append(heads, len(nodes)).astype(np.int32)
    feat_track = np.full(n, -1, np.int32)
    feat_track[nodes] = np.repeat(np.arange(len(heads)), np.diff(trk_off))
    obs_img, obs_feat = ids[slot[nodes]].astype(np.int32), (nodes - node_off[slot[nodes]]).astype(np.int32)
    is_root = root == np.arange(n)
    r2 = is_root & (size[:n] >= 2)
    whole = r2 & cflag[:n] & (conflict == DROP_TRACK)
    kept = r2 & ~whole & len_ok[:n]
    stats = np.array([r2.sum(), (r2 & cflag[:n]).sum(), dropped4.sum(), (r2 & ~whole & ~len_ok[:n]).sum(), size[:n].max() if n else 0,
                      nsurv[:n][kept].max() if kept.any() else 0, len(u), 0], np.int64)
    out = dict(img_ids=ids, node_off=node_off, counts=np.array([len(heads), len(nodes)], np.int32), trk_off=trk_off, obs_img=obs_img,
               obs_feat=obs_feat, obs_cam=cam_of_slot[slot[nodes]].astype(np.int32) if select is not None else None, obs_xy=None,
               feat_track=feat_track, stats=stats)
    if coords is not None:
        out["obs_xy"] = np.array([coords[int(i)][int(f)] for i, f in zip(obs_img, obs_feat)], np.int32).reshape(-1, 2)
    out["tracks"] = [list(zip(obs_img[a:b].tolist(), obs_feat[a:b].tolist())) for a, b in zip(trk_off[:-1], trk_off[1:])]
    return out


def truncate(res, cap_tracks, cap_obs):
    """What a call with these capacities writes: track j iff tracks 0 .. j fit both; trk_off has cap_tracks + 1 entries, the ones past
    the last written track repeat its end; feat_track names written tracks only.  counts stay those of the full result."""
    off = res["trk_off"]
    w = 0
    while w < min(len(off) - 1, cap_tracks) and off[w + 1] <= cap_obs:
        w += 1
    end = int(off[w])
    out = dict(res)
    out["written"] = w
    out["trk_off"] = np.concatenate([off[:w + 1], np.full(cap_tracks - w, end, np.int32)]).astype(np.int32)
    for k in ("obs_img", "obs_feat", "obs_cam", "obs_xy"):
        out[k] = res[k][:end] if res[k] is not None else None
    ft = res["feat_track"].copy()
    ft[ft >= w] = -1
    out["feat_track"] = ft
    out["tracks"] = res["tracks"][:w]
    return out


# ---- scenes shared by the CPU checks of the scenes (tests/test_tracks_ref.py) and the GPU tests (tests/test_tracks_gpu.py) ----------

def lists_of(fm):
    """{(a, b): [(f, g), ...]} -> (pairs, offsets, qt) in the dict's order."""
    pairs, offs, qt = [], [0], []
    for (a, b), m in fm.items():
        pairs.append((int(a), int(b)))
        qt.extend((int(f), int(g)) for f, g in m)
        offs.append(len(qt))
    return np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.asarray(qt, np.int32).reshape(-1, 2)


def coords_of(K, seed=0):
    rng = np.random.default_rng(seed)
    return {int(i): rng.integers(0, 4000, (int(k), 2)).astype(np.int32) for i, k in K.items()}


def shuffled(fm, seed):
    """The same lists with the pairs and the entries of every pair in another order."""
    rng = np.random.default_rng(seed)
    keys = list(fm)
    return {keys[k]: [fm[keys[k]][e] for e in rng.permutation(len(fm[keys[k]]))] for k in rng.permutation(len(keys))}


def scene_chain(L, K=2):
    """L images of K keypoints, f -> f between consecutive images: K tracks of exactly L observations."""
    return {(i, i + 1): [(f, f) for f in range(K)] for i in range(L - 1)}, {i: K for i in range(L)}


def scene_star(n=64):
    """Feature 0 of image 0 matched into n other images (feature 1 of each): one track of n + 1, every union on one root."""
    return {(0, i): [(0, 1)] for i in range(1, n + 1)}, {i: 3 for i in range(n + 1)}


def scene_grid(n=12, K=600):
    """n images of K keypoints, f -> f across all n (n - 1) / 2 pairs: K cliques of n."""
    return {(a, b): [(f, f) for f in range(K)] for a in range(n) for b in range(a + 1, n)}, {i: K for i in range(n)}


def scene_giant(n=12, K=600):
    """f -> f + 1 between consecutive images and f -> f elsewhere: the shifts chain every feature to the next, one component far above
    the image count."""
    fm = {}
    for a in range(n):
        for b in range(a + 1, n):
            fm[(a, b)] = [(f, f + 1) for f in range(K - 1)] if b == a + 1 else [(f, f) for f in range(K)]
    return fm, {i: K for i in range(n)}


def scene_conflict():
    """Images 10, 11, 12, 14 (ids with gaps) of 3 keypoints: the component {(10, 0), (11, 0), (12, 0), (14, 0), (11, 2)} holds image 11
    twice (the planted wrong match (12, 0) -> (11, 2)); features 1 chain cleanly through all four images."""
    fm = {(10, 11): [(0, 0), (1, 1)], (11, 12): [(0, 0), (1, 1)], (12, 14): [(0, 0), (1, 1)], (12, 11): [(0, 2)]}
    return fm, {10: 3, 11: 3, 12: 3, 14: 3}


def scene_six(seed=2):
    """Six images (ids 3 .. 8) of 40 keypoints with random injective lists on 10 of the 15 pairs: tracks of many lengths, some conflicts,
    keypoints matched nowhere; used with a selection of 3 images, min_length 3 and max_length 4."""
    rng = np.random.default_rng(seed)
    ids = list(range(3, 9))
    fm = {}
    for a in range(6):
        for b in range(a + 1, 6):
            if rng.random() < 0.6:
                m = int(rng.integers(5, 30))
                f = rng.permutation(40)[:m]
                g = np.where(rng.random(m) < 0.85, f, rng.permutation(40)[:m])       # mostly the same landmark, some wrong matches
                _, keep = np.unique(g, return_index=True)
                fm[(ids[a], ids[b])] = [(int(f[k]), int(g[k])) for k in sorted(keep)]
    return fm, {i: 40 for i in ids}


def scene_degenerate():
    """Images with K = 0, an empty list, a feature matched nowhere (image 2, feature 3) and one real match."""
    return {(0, 1): [], (1, 2): [(0, 1)], (2, 5): [], (5, 7): []}, {0: 0, 1: 2, 2: 4, 5: 0, 7: 1}
