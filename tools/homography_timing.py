"""Times of the homography search and of the two-view geometry call next to the E search on the same
pairs: HIP events on a stream of its own around each host entry (its copies in and out are inside the interval; the
kernels k_hg_pair and k_tv_pair are the only launches of rcn_homography_ransac and rcn_twoview_init), 3 warm-up calls,
median of --reps, the clock state noted; beside them the time of the numpy restatement (tests/homography_ref.py, one run)
on the first pair.  Writes profiles/homography_timing.json, stamped with the source hash.

    python tools/homography_timing.py [--reps 20] [--no-ref]

Batches of 1, 32 and 300 pairs at 300 and 2500 entries per pair, shares of wrong matches 0.3 and 0.6
(tests/twoview_ref.scene_pair: general scenes, the case in which the homography search runs to its iteration cap)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _clocks():
    try:
        return subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30).stdout[-1500:]
    except Exception as e:                                   # noqa: BLE001  (the note is optional)
        return "unavailable: %s" % e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement")
    a = ap.parse_args()
    import torch
    import bench
    import homography_ref as hr
    import twoview_ref as tv
    from reconstructor_amd import _lib, homography, twoview
    ctx = _lib.Context(0)
    out = {"tool": "homography_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "clocks_before": _clocks(), "unit": "ms, median of reps, host entry (copies inside)", "cases": []}
    st = torch.cuda.Stream()
    base = {}
    for n in (300, 2500):
        for w in (0.3, 0.6):
            base[(n, w)] = [tv.scene_pair(7000 + 10 * k + int(10 * w), w, n=n) for k in range(8)]
    for npairs in (1, 32, 300):
        for n in (300, 2500):
            for w in (0.3, 0.6):
                sc = [base[(n, w)][p % 8] for p in range(npairs)]
                off = np.arange(npairs + 1, dtype=np.int64) * n
                xy1, xy2 = np.concatenate([s["xy1"] for s in sc]), np.concatenate([s["xy2"] for s in sc])
                K1, K2 = np.stack([s["K1"] for s in sc]), np.stack([s["K2"] for s in sc])
                calls = {"homography": lambda: homography.find(ctx, off, xy1, xy2),
                         "twoview": lambda: twoview.two_view_init(ctx, off, xy1, xy2, K1, K2),
                         "geometry": lambda: twoview.geometry(ctx, off, xy1, xy2, K1, K2)}
                c = {"pairs": npairs, "entries_per_pair": n, "wrong_share": w}
                torch.cuda.synchronize()
                ctx.check(ctx.lib.rcn_set_stream(ctx.h, st.cuda_stream))
                for name, fn in calls.items():
                    for _ in range(3):
                        r = fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ms = []
                    for _ in range(a.reps):
                        e0.record(st)
                        r = fn()
                        e1.record(st)
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    c[name + "_ms"] = round(float(np.median(ms)), 4)
                    if name == "homography":
                        c["h_iterations_first"] = int(r["iterations"][0])
                    if name == "twoview":
                        c["e_iterations_first"] = int(r["iterations"][0])
                ctx.check(ctx.lib.rcn_set_stream(ctx.h, None))
                c["homography_over_twoview"] = round(c["homography_ms"] / c["twoview_ms"], 3)
                c["geometry_over_twoview"] = round(c["geometry_ms"] / c["twoview_ms"], 3)
                if not a.no_ref and npairs == 1:
                    t0 = time.perf_counter()
                    hr.find(sc[0]["xy1"], sc[0]["xy2"])
                    c["numpy_restatement_ms_one_pair"] = round(1e3 * (time.perf_counter() - t0), 1)
                out["cases"].append(c)
    out["clocks_after"] = _clocks()
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "homography_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not k.startswith("clocks")}))


if __name__ == "__main__":
    main()
