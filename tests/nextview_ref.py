"""CPU restatements of the next-view search (csrc/corr2d3d.hip), for the tests only.

literal_*     the reference's loops as it writes them (SequentialReconstructor.cpp:643-759, :497-512) over plain containers:
              calc2d3dMatches, rankNextImages in both modes with their map quirks, step 1 of triangulateMatchedLandmarks
vector_*      the restatement the kernels implement: obs_of[(image, feature)] = flattened observation index, a walk over
              the directed match lists (mirror resolved as rcn_match_lists_upload does), the hits of a candidate ordered
              by observation index; the density cells and the out-of-frame count per candidate
make_case     seeded containers for both (a synth_ba scene half registered), built in numpy
"""
import numpy as np

import tri_ref

CELL = 32


def cell_of(x, y, rows, cols):
    """rankNextImages (:726-731): (int)(cellSize * x / (double)cols) with C's truncation; None outside 0 .. 31."""
    cx, cy = int((CELL * int(x)) / float(cols)), int((CELL * int(y)) / float(rows))
    return (cy, cx) if 0 <= cx < CELL and 0 <= cy < CELL else None


# ---- the reference's loops ----------------------------------------------------------------------------------------------

def literal_calc_2d3d_matches(candidates, img_matches, feature_matches, landmark_ids, tracks):
    """calc2d3dMatches (:643-695): ({c: landmarkIds}, {c: featureIds}) for the std::set of candidates (ascending)."""
    lids, fids = {}, {}
    for c in sorted(set(candidates)):
        cm = img_matches[c]
        L, F = [], []
        for lid, track in enumerate(tracks):
            for i, f in track:
                if i in cm:
                    pm = feature_matches.get((i, c), {})        # operator[]: an absent pair is an empty map
                    if f in pm and landmark_ids[c][pm[f]] == -1:
                        L.append(lid)
                        F.append(pm[f])
        lids[c], fids[c] = L, F
    return lids, fids


def literal_density(feats, coords, shape):
    """:723-736: projDensity set per entry (out-of-frame cells set nothing here; the reference writes out of bounds)."""
    rows, cols = shape
    cells = set()
    for g in feats:
        c = cell_of(coords[g][0], coords[g][1], rows, cols)
        if c is not None:
            cells.add(c)
    return len(cells)


def literal_rank(lids, fids, mode, coords, shapes, min_matches=30, order=None):
    """rankNextImages (:697-759).  order: the unordered_map's iteration order over the candidates (default: dict order).
    MatchTotal: std::map<imgId, n, greater>: image ids descending.  MatchDensity: std::map<score, imgId, greater> assigned
    in iteration order (the last image of a score wins), scores > min_matches."""
    order = list(lids) if order is None else list(order)
    if mode == "total":
        m = {c: len(lids[c]) for c in order}
        return sorted(m, reverse=True)
    score2img = {}
    for c in order:
        score2img[literal_density(fids[c], coords[c], shapes[c])] = c
    return [score2img[s] for s in sorted(score2img, reverse=True) if s > min_matches]


def literal_attach(P, K, points, entries, max_err=4.0, taken=None):
    """Step 1 (:497-512) over entries [(landmark, feature, (x, y))]: status per entry (0 attached, 1 depth, 2 reprojection,
    3 feature already has a landmark) -- the first failing rule in that order."""
    taken = set() if taken is None else taken
    P = [float(v) for v in np.asarray(P).reshape(12)]
    K = [float(v) for v in np.asarray(K).reshape(6)]
    out = []
    for l, f, (x, y) in entries:
        X = [float(v) for v in points[l]]
        err, depth = tri_ref.reproj_l1(P, K, X, x, y)
        if not depth > 0:
            out.append(1)
        elif not err < max_err:
            out.append(2)
        elif f in taken:
            out.append(3)
        else:
            taken.add(f)
            out.append(0)
    return out


# ---- the kernels' restatement ---------------------------------------------------------------------------------------------

def resolve_lists(pairs, offsets, qt, mirror):
    """{(i, c): {f: g}} as the device reads it: a directed pair as given, else (mirror) its reverse read backwards."""
    direct = {}
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        direct[(a, b)] = {int(f): int(g) for f, g in np.asarray(qt).reshape(-1, 2)[offsets[p]:offsets[p + 1]].tolist()}
    out = dict(direct)
    if mirror:
        for (a, b), m in direct.items():
            if (b, a) not in direct:
                out[(b, a)] = {g: f for f, g in m.items()}
    return out


def vector_corr(pt_off, obs_img, obs_feat, pairs, offsets, qt, mirror, candidates, shapes, coords):
    """obs_of + list walk + order by observation index.  Returns (cand_off, landmark, feature, cells, outside) as
    rcn_corr_2d3d does."""
    pt_off, obs_img, obs_feat = np.asarray(pt_off), np.asarray(obs_img), np.asarray(obs_feat)
    obs_pt = np.repeat(np.arange(len(pt_off) - 1), np.diff(pt_off))
    obs_of = {}
    for o, (i, f) in enumerate(zip(obs_img.tolist(), obs_feat.tolist())):
        obs_of.setdefault((i, f), o)
    graph_imgs = set(obs_img.tolist())
    lists = resolve_lists(pairs, offsets, qt, mirror)
    off, L, F, cells, outside = [0], [], [], [], []
    for c, (rows, cols) in zip(list(candidates), np.asarray(shapes).reshape(-1, 2).tolist()):
        hits = {}
        for (i, cc), m in lists.items():
            if cc != c or i == c or i not in graph_imgs:
                continue
            for f, g in m.items():
                o = obs_of.get((i, f))
                if o is not None:
                    hits[o] = g
        occ, out = set(), 0
        for o in sorted(hits):
            L.append(int(obs_pt[o]))
            F.append(hits[o])
            cl = cell_of(coords[c][hits[o]][0], coords[c][hits[o]][1], rows, cols)
            if cl is None:
                out += 1
            else:
                occ.add(cl)
        off.append(len(L))
        cells.append(len(occ))
        outside.append(out)
    return (np.asarray(off, np.int64), np.asarray(L, np.int32), np.asarray(F, np.int32), np.asarray(cells, np.int32),
            np.asarray(outside, np.int32))


# ---- seeded containers ------------------------------------------------------------------------------------------------------

SHAPE = (336, 512)       # rows, cols of the synth_ba images (K0: cx 256, cy 168)


def make_case(n_images, n_points, seed=0, obs_per_point=6, n_registered=None, extra_rate=0.02):
    """A synth_ba scene through tri_ref.loop_containers, its first n_registered images registered: one landmark per scene
    point seen by >= 2 of them (track = those observations, in random order).  Some landmarks are split in two (the same
    feature then matches two landmarks' observations, so a candidate feature repeats) and a few random extra matches are
    added to the lists (both directions, kept injective).  Returns the containers of loop_containers plus tracks,
    candidates, shapes."""
    L = tri_ref.loop_containers(n_images, n_points, obs_per_point=obs_per_point, seed=seed, wrong_rate=0.0)
    rng = np.random.default_rng(seed + 101)
    nr = n_images // 2 if n_registered is None else n_registered
    reg = list(range(nr))
    seen = {}
    for i in reg:
        for f, p in enumerate(L["point_of"][i]):
            seen.setdefault(p, []).append((i, f))
    tracks = []
    for p in sorted(seen):
        t = seen[p]
        if len(t) < 2:
            continue
        t = [t[k] for k in rng.permutation(len(t))]
        if len(t) >= 4 and rng.random() < 0.1:
            tracks.append(t[:2])
            tracks.append(t[2:])
        else:
            tracks.append(t)
    tracks = [tracks[k] for k in rng.permutation(len(tracks))]
    fm = L["feature_matches"]
    for (i, j) in [k for k in fm if k[0] < k[1]]:
        if rng.random() < extra_rate * 10:
            m, r = fm[(i, j)], fm[(j, i)]
            fi = rng.integers(0, len(L["coords"][i]))
            gj = rng.integers(0, len(L["coords"][j]))
            if fi not in m and gj not in r:
                m[int(fi)] = int(gj)
                r[int(gj)] = int(fi)
    L["tracks"] = tracks
    L["candidates"] = list(range(nr, n_images))
    L["shapes"] = {i: SHAPE for i in range(n_images)}
    return L


def canonical_lists(fm):
    """The i < j half of a two-way featureMatches (what mirror = 1 expects)."""
    return {k: v for k, v in fm.items() if k[0] < k[1]}


def vector_attach(P, K, points, entries, max_err=4.0):
    """The attach kernels' rule: per entry the two geometric rules, then the smallest index among the PASSING entries of a
    feature wins; the other passing entries of that feature get status 3."""
    P = [float(v) for v in np.asarray(P).reshape(12)]
    K = [float(v) for v in np.asarray(K).reshape(6)]
    st, win = [], {}
    for e, (l, f, (x, y)) in enumerate(entries):
        err, depth = tri_ref.reproj_l1(P, K, [float(v) for v in points[l]], x, y)
        s = 1 if not depth > 0 else 2 if not err < max_err else 0
        st.append(s)
        if s == 0:
            win[f] = min(win.get(f, e), e)
    return [3 if s == 0 and win[f] != e else s for e, (s, (_, f, _)) in enumerate(zip(st, entries))]
