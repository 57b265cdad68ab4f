"""Writes tests/golden/tracks_small.npz: small list sets with the contract's answer (tests/tracks_ref.py), so that a change of the
contract shows up as a diff.  Run from the repository root:  python tests/golden/make_tracks_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tracks_ref as T  # noqa: E402


def main():
    cases = {
        "conflict_track": (T.scene_conflict(), dict()),
        "conflict_image": (T.scene_conflict(), dict(conflict=T.DROP_IMAGE)),
        "six_select": (T.scene_six(), dict(select=([7, 3, 5], [2, 0, 1]), conflict=T.DROP_IMAGE)),
        "six_lengths": (T.scene_six(), dict(min_length=3, max_length=4)),
        "chain_65": (T.scene_chain(65), dict()),
        "degenerate": (T.scene_degenerate(), dict()),
    }
    out = {}
    for name, ((fm, K), kw) in cases.items():
        pairs, offsets, qt = T.lists_of(fm)
        r = T.build(pairs, offsets, qt, K, **kw)
        sel = kw.get("select", ([], []))
        out.update({name + ".pairs": pairs, name + ".offsets": offsets, name + ".qt": qt,
                    name + ".K_img": np.array(sorted(K), np.int32), name + ".K": np.array([K[i] for i in sorted(K)], np.int32),
                    name + ".options": np.array([kw.get("min_length", 2), kw.get("max_length", 0), kw.get("conflict", 0)], np.int32),
                    name + ".sel_img": np.array(sel[0], np.int32), name + ".sel_cam": np.array(sel[1], np.int32)})
        for k in ("counts", "trk_off", "obs_img", "obs_feat", "feat_track", "stats"):
            out[name + "." + k] = r[k]
    np.savez_compressed(os.path.join(HERE, "tracks_small.npz"), **out)


if __name__ == "__main__":
    main()
