"""Step 3 of triangulateMatchedLandmarks (SequentialReconstructor.cpp:514-553) turned round, as csrc/corr2d3d.hip computes
it: instead of walking the registered images for every feature, walk every list (new image, reg[k]) once, keep per feature
the minimum of (k, g) over the entries whose two ends are free, and read the result out in feature order.  The literal loop
is reconstructor_amd.triangulate.new_view_tracks; tests/test_new_view_tracks_ref.py holds the two against each other.
Also the seeded scenes of those tests and a classification of the new image's features by what the literal loop does."""
import numpy as np

import tri_ref


def turned_round(img, landmark_ids, registered, img_matches, feature_matches):
    """The tracks [(reg image, g), (img, f)] in ascending f: min over the lists of (position in the visited order, g)."""
    matched = set(img_matches[img])
    reg = [r for r, status in registered if status and r in matched]
    own = landmark_ids[img]
    best = {}
    for k, r in enumerate(reg):
        pm = feature_matches.get((img, r))
        if pm is None:
            continue
        for f, g in pm.items():
            if own[f] != -1 or landmark_ids[r][g] != -1:
                continue
            if f not in best or (k, g) < best[f]:
                best[f] = (k, g)
    return [[(reg[k], int(g)), (img, int(f))] for f, (k, g) in sorted(best.items())]


TAKEN, FIRST, FALL_THROUGH, NO_TRACK = "taken", "first", "fall-through", "no-track"


def classify(img, landmark_ids, registered, img_matches, feature_matches):
    """What the literal loop does with every feature of img: TAKEN (a landmark already), FIRST (its track comes from the first
    visited list that holds it), FALL_THROUGH (an earlier list held it with a taken partner), NO_TRACK (free, no track)."""
    matched = set(img_matches[img])
    out = []
    for f, l in enumerate(landmark_ids[img]):
        if l != -1:
            out.append(TAKEN)
            continue
        skipped, kind = 0, NO_TRACK
        for reg, status in registered:
            if not status or reg not in matched:
                continue
            pm = feature_matches.get((img, reg))
            if pm is None or f not in pm:
                continue
            if landmark_ids[reg][pm[f]] == -1:
                kind = FALL_THROUGH if skipped else FIRST
                break
            skipped += 1
        out.append(kind)
    return out


def take_ids(landmark_ids, frac=0.35, seed=0):
    """A copy of the id containers with `frac` of all entries set to random non-negative values."""
    rng = np.random.default_rng(seed)
    out = {}
    for i, row in landmark_ids.items():
        hit = rng.random(len(row)) < frac
        val = rng.integers(0, 1 << 20, len(row))
        out[i] = [int(val[f]) if hit[f] else -1 for f in range(len(row))]
    return out


def scene(n_images, n_points, obs_per_point, seed, frac=0.35):
    """tri_ref.loop_containers with `frac` of the ids taken, the last image as the new one and the others registered in a
    seeded permutation with one entry's status false."""
    L = tri_ref.loop_containers(n_images, n_points, obs_per_point=obs_per_point, seed=seed)
    L["landmark_ids"] = take_ids(L["landmark_ids"], frac, seed + 11)
    rng = np.random.default_rng(seed + 12)
    v = n_images - 1
    order = [int(i) for i in rng.permutation(n_images - 1)]
    off = order[int(rng.integers(0, len(order)))]
    L["v"] = v
    L["registered"] = [(i, i != off) for i in order]
    L["cam_index"] = {i: i for i in range(n_images)}
    return L
