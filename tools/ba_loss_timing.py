"""Cost of a robust loss in the bundle adjustment at cfg 4 and cfg 5 size (synth_ba.make_scene, 200 cameras /
200k observations and 1000 cameras / 1M observations, 8 % of the observations displaced by 20 to 120 px): LM iterations per second and
the time of the residual + Jacobian kernel per launch (summary.jacobian_seconds / jacobian_evals) without a loss and under Huber,
soft-L1 and Cauchy at 2 px.  Solves with different losses take different paths (other iteration counts), so the kernel's time per
launch and the iteration rate are the comparable figures, not the solve time.

With --parent-lib PATH (a librcn.so built from the parent commit) the no-loss figures are also taken with THAT library, parent and
new alternating, --rounds each (default 3): the no-loss path passes when the new library's median lies within the spread (min .. max)
of the parent's own rounds.  Nothing tighter is claimed.

Every measurement is a process of its own (--worker; one library per process), which solves once to warm up (allocations, pair
lists, clocks) and then times --solves solves: wall time between two stream synchronisations (rcn_ba_summary.solve_seconds is taken
inside the library that way) and HIP events around the kernel.  Fails without a GPU.  One JSON line stamped with the source hash.

    python tools/ba_loss_timing.py [--parent-lib PATH] [--rounds 3] [--solves 2] [--cfgs 4,5]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CFG = {4: (200, 20000), 5: (1000, 100000)}
LOSSES = {"none": None, "huber": (1, 2.0), "soft_l1": (2, 2.0), "cauchy": (3, 2.0)}


def worker(a):
    """one library, one configuration, one loss: prints a JSON line"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ba_loss_timing: no GPU")
    import ba_loss_ref as R
    from reconstructor_amd import synth_ba
    from reconstructor_amd._lib import BaLoss, BaOptions, BaProblem, BaSummary      # the struct layouts of include/rcn.h (unchanged since the parent)
    L = C.CDLL(a.lib)
    vp = C.c_void_p
    L.rcn_create.argtypes, L.rcn_destroy.argtypes = [C.c_int, C.POINTER(vp)], [vp]
    L.rcn_last_error.restype, L.rcn_last_error.argtypes = C.c_char_p, [vp]
    L.rcn_ba_default_options.argtypes = [C.c_int32, C.POINTER(BaOptions)]
    L.rcn_ba_solve.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaSummary)]
    nc, npts = CFG[a.cfg]
    base = synth_ba.make_scene(nc, npts, obs_per_point=10, seed=2024)
    sc, _ = R.plant_outliers(base, len(base["obs_cam"]) * 8 // 100, 2024)
    loss = LOSSES[a.loss]
    h = vp()
    assert L.rcn_create(0, C.byref(h)) == 0, "rcn_create"
    o = BaOptions()
    L.rcn_ba_default_options(nc, C.byref(o))
    uv, cam, pt = (np.ascontiguousarray(sc[k], t) for k, t in (("obs_uv", np.float64), ("obs_cam", np.int32), ("obs_pt", np.int32)))
    runs = []
    for i in range(a.solves + 1):
        poses, intr, pts = (np.array(sc[k], np.float64, order="C") for k in ("poses", "intrinsics", "points"))
        pb = BaProblem(nc, npts, len(cam), 0, poses.ctypes.data, intr.ctypes.data, pts.ctypes.data, uv.ctypes.data, cam.ctypes.data, pt.ctypes.data)
        s = BaSummary()
        if loss is None:
            rc = L.rcn_ba_solve(h, C.byref(pb), C.byref(o), C.byref(s))
        else:
            L.rcn_ba_solve_robust.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaLoss), C.POINTER(BaSummary), vp, vp]
            rc = L.rcn_ba_solve_robust(h, C.byref(pb), C.byref(o), C.byref(BaLoss(loss[0], 0, loss[1])), C.byref(s), None, None)
        assert rc == 0, L.rcn_last_error(h).decode()
        if i:          # (the first solve is the warm-up)
            runs.append(dict(iterations=s.iterations, solve_seconds=s.solve_seconds, jacobian_seconds=s.jacobian_seconds, jacobian_evals=s.jacobian_evals,
                             final_rms_px=s.final_rms_px, termination=s.termination))
    L.rcn_destroy(h)
    it = sum(r["iterations"] for r in runs)
    print(json.dumps(dict(cfg=a.cfg, loss=a.loss, n_obs=len(cam), iterations=runs[0]["iterations"], termination=runs[0]["termination"], final_rms_px=runs[0]["final_rms_px"],
                          lm_iterations_per_s=it / sum(r["solve_seconds"] for r in runs),
                          jacobian_us_per_eval=1e6 * sum(r["jacobian_seconds"] for r in runs) / max(1, sum(r["jacobian_evals"] for r in runs)))))


def measure(lib, cfg, loss, solves):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--cfg", str(cfg), "--loss", loss, "--solves", str(solves)],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("worker failed (%s, cfg %d, %s):\n%s%s" % (lib, cfg, loss, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "reconstructor_amd", "librcn.so"))
    ap.add_argument("--cfg", type=int, default=4)
    ap.add_argument("--loss", default="none")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solves", type=int, default=2)
    ap.add_argument("--cfgs", default="4,5")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ba_loss_timing: no GPU")
    import bench
    out = {"tool": "ba_loss_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "solves_per_round": a.solves,
           "loss_scale_px": 2.0, "outliers": "8 % of the observations displaced by 20 to 120 px per axis", "cases": {}}
    for cfg in (int(v) for v in a.cfgs.split(",")):
        case = out["cases"]["cfg%d" % cfg] = {}
        rounds = {"new": [], "parent": []}
        for _ in range(a.rounds):          # parent and new alternate
            if a.parent_lib:
                rounds["parent"].append(measure(a.parent_lib, cfg, "none", a.solves))
            rounds["new"].append(measure(a.lib, cfg, "none", a.solves))
        case["n_obs"] = rounds["new"][0]["n_obs"]
        for who, rs in rounds.items():
            if rs:
                case["no_loss_" + who] = {k: [round(r[k], 3) for r in rs] for k in ("lm_iterations_per_s", "jacobian_us_per_eval")}
                case["no_loss_" + who]["iterations"] = rs[0]["iterations"]
        if a.parent_lib:
            verdict = {}
            for k in ("lm_iterations_per_s", "jacobian_us_per_eval"):
                p, n = [r[k] for r in rounds["parent"]], float(np.median([r[k] for r in rounds["new"]]))
                verdict[k] = {"parent_min": round(min(p), 3), "parent_max": round(max(p), 3), "new_median": round(n, 3), "within_parent_spread": bool(min(p) <= n <= max(p))}
            case["no_loss_ab"] = verdict
        for name in ("huber", "soft_l1", "cauchy"):
            r = measure(a.lib, cfg, name, a.solves)
            case[name] = {k: (round(r[k], 3) if isinstance(r[k], float) else r[k]) for k in ("iterations", "termination", "final_rms_px", "lm_iterations_per_s", "jacobian_us_per_eval")}
            case[name]["jacobian_bytes_per_obs"] = 224
            case[name]["jacobian_tb_per_s"] = round(224 * r["n_obs"] / (r["jacobian_us_per_eval"] * 1e-6) / 1e12, 3)
        n0 = float(np.median([r["jacobian_us_per_eval"] for r in rounds["new"]]))
        case["no_loss_jacobian_tb_per_s"] = round(224 * case["n_obs"] / (n0 * 1e-6) / 1e12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
