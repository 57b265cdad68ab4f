"""What shared intrinsics cost and save on the large solves, at cfg 4 and cfg 5 size (synth_ba.make_scene, 200
cameras / 200k observations and 1000 cameras / 1M observations; every camera of the scene shares its true intrinsics).

One group of all cameras against no groups, per case:
  lm_iterations_per_s, iterations, termination, final rms
  per LM iteration: the factorisation (rcn_ba_summary.cholesky_seconds), the Schur phase (schur_seconds: HIP events around the Schur build
  and, tied, the fold behind it) and the rest of the loop
  fold_s_per_iteration   the tied Schur phase minus the untied one, per iteration: the same Schur build on the same scene, so the
                         difference of the two event-timed phases is the fold (its three kernels, the padding and the right-hand-side row)
  fold_bytes, fold_gb_per_s, hbm_roof_fraction   the lower triangle of S read once plus S' written, over that time, against 8 TB/s
  expected_factor_ratio  (n' / n)^3, beside the measured ratio of the factorisation's time
With --parent-lib PATH (a librcn.so built from the parent commit) the untied solve is also timed with THAT library, parent and new
alternating, --rounds each: the new library passes when the median of its LM iterations per second lies within the spread (min .. max)
of the parent's own rounds, as tools/ba_loss_timing.py and tools/ba_local_timing.py judged.  Nothing tighter is claimed.

Every measurement is a process of its own (one library per process).  The scenes are made once and handed to the workers in a
temporary file.  Fails without a GPU.  Writes --out (default profiles/ba_tied_timing.json), stamped with the source hash.

    python tools/ba_tied_timing.py [--parent-lib PATH] [--rounds 3] [--solves 2] [--cfgs 4,5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {4: (200, 20000), 5: (1000, 100000)}
HBM_ROOF = 8.0e12      # bytes / s


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ba_tied_timing: no GPU")
    return torch


def worker(a):
    """rcn_ba_solve (untied; an entry both the parent and this tree have) or rcn_ba_solve_tied with one group, through one library's C ABI"""
    _need_gpu()
    from reconstructor_amd._lib import BaOptions, BaProblem, BaSummary      # struct layouts of include/rcn.h (unchanged since the parent)
    sc = dict(np.load(a.scene))
    L = C.CDLL(a.lib)
    vp = C.c_void_p
    L.rcn_create.argtypes, L.rcn_destroy.argtypes = [C.c_int, C.POINTER(vp)], [vp]
    L.rcn_last_error.restype, L.rcn_last_error.argtypes = C.c_char_p, [vp]
    L.rcn_ba_default_options.argtypes = [C.c_int32, C.POINTER(BaOptions)]
    L.rcn_ba_solve.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), C.POINTER(BaSummary)]
    h = vp()
    assert L.rcn_create(0, C.byref(h)) == 0, "rcn_create"
    uv, cam, pt = np.ascontiguousarray(sc["obs_uv"], np.float64), np.ascontiguousarray(sc["obs_cam"], np.int32), np.ascontiguousarray(sc["obs_pt"], np.int32)
    nc = len(sc["poses"])
    grp = np.zeros(nc, np.int32)
    o = BaOptions()
    L.rcn_ba_default_options(nc, C.byref(o))
    runs = []
    for i in range(a.solves + 1):
        P, K, X = (np.array(sc[k], np.float64, order="C") for k in ("poses", "intrinsics", "points"))
        pb = BaProblem(nc, len(X), len(cam), 0, P.ctypes.data, K.ctypes.data, X.ctypes.data, uv.ctypes.data, cam.ctypes.data, pt.ctypes.data)
        sm = BaSummary()
        if a.worker == "tied":
            L.rcn_ba_solve_tied.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOptions), vp, vp, vp, C.POINTER(BaSummary), vp, vp]
            rc = L.rcn_ba_solve_tied(h, C.byref(pb), C.byref(o), None, None, grp.ctypes.data, C.byref(sm), None, None)
        else:
            rc = L.rcn_ba_solve(h, C.byref(pb), C.byref(o), C.byref(sm))
        assert rc == 0, L.rcn_last_error(h).decode()
        if i:          # (the first solve is the warm-up)
            runs.append({k: getattr(sm, k) for k in ("iterations", "termination", "reduced_dim", "solve_seconds", "schur_seconds", "cholesky_seconds", "trisolve_seconds",
                                                     "final_rms_px")})
    L.rcn_destroy(h)
    it = sum(r["iterations"] for r in runs)
    tot = {k: sum(r[k] for r in runs) for k in ("solve_seconds", "schur_seconds", "cholesky_seconds", "trisolve_seconds")}
    print(json.dumps(dict(n_obs=len(pt), iterations=runs[0]["iterations"], termination=runs[0]["termination"], reduced_dim=runs[0]["reduced_dim"],
                          final_rms_px=runs[0]["final_rms_px"], lm_iterations_per_s=it / tot["solve_seconds"], iteration_s=tot["solve_seconds"] / it,
                          cholesky_s_per_iteration=tot["cholesky_seconds"] / it, schur_s_per_iteration=tot["schur_seconds"] / it,
                          rest_s_per_iteration=(tot["solve_seconds"] - tot["cholesky_seconds"] - tot["schur_seconds"]) / it)))


def measure(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit("worker failed (%s):\n%s%s" % (" ".join(args), r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def _round(v):
    if isinstance(v, float):
        return float("%.4g" % v)
    if isinstance(v, dict):
        return {k: _round(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_round(x) for x in v]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["untied", "tied"], default=None)
    ap.add_argument("--lib", default=os.path.join(ROOT, "reconstructor_amd", "librcn.so"))
    ap.add_argument("--scene", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solves", type=int, default=2)
    ap.add_argument("--cfgs", default="4,5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_tied_timing.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    torch = _need_gpu()
    import bench
    from reconstructor_amd import synth_ba
    out = {"tool": "ba_tied_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "solves_per_round": a.solves,
           "hbm_roof_bytes_per_s": HBM_ROOF, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for cfg in (int(v) for v in a.cfgs.split(",")):
            nc, npts = CFG[cfg]
            sc = synth_ba.make_scene(nc, npts, obs_per_point=10, seed=2024)
            path = os.path.join(tmp, "cfg%d.npz" % cfg)
            np.savez(path, **{k: sc[k] for k in ("poses", "intrinsics", "points", "obs_uv", "obs_cam", "obs_pt")})
            case = out["cases"]["cfg%d" % cfg] = {}
            rounds = {"new": [], "parent": [], "tied": []}
            for _ in range(a.rounds):          # parent, new and tied alternate
                if a.parent_lib:
                    rounds["parent"].append(measure(["--worker", "untied", "--lib", a.parent_lib, "--scene", path, "--solves", str(a.solves)]))
                rounds["new"].append(measure(["--worker", "untied", "--lib", a.lib, "--scene", path, "--solves", str(a.solves)]))
                rounds["tied"].append(measure(["--worker", "tied", "--lib", a.lib, "--scene", path, "--solves", str(a.solves)]))
            med = lambda rs, k: float(np.median([r[k] for r in rs]))
            for who, key in (("new", "no_groups"), ("tied", "one_group")):
                rs = rounds[who]
                case[key] = _round(dict(reduced_dim=rs[0]["reduced_dim"], iterations=rs[0]["iterations"], termination=rs[0]["termination"], final_rms_px=rs[0]["final_rms_px"],
                                        lm_iterations_per_s=[r["lm_iterations_per_s"] for r in rs],
                                        **{k: med(rs, k) for k in ("iteration_s", "cholesky_s_per_iteration", "schur_s_per_iteration", "rest_s_per_iteration")}))
            n, nt = case["no_groups"]["reduced_dim"], case["one_group"]["reduced_dim"]
            pad = lambda v: max(128, (v + 127) // 128 * 128)
            fold_s = med(rounds["tied"], "schur_s_per_iteration") - med(rounds["new"], "schur_s_per_iteration")
            fold_bytes = 8.0 * (n * (n + 1) / 2 + nt * (nt + 1) / 2 + (pad(nt) - nt) * pad(nt))
            saved = med(rounds["new"], "cholesky_s_per_iteration") - med(rounds["tied"], "cholesky_s_per_iteration")
            case["fold"] = _round(dict(fold_s_per_iteration=fold_s, fold_bytes=fold_bytes, fold_gb_per_s=fold_bytes / fold_s / 1e9 if fold_s > 0 else None,
                                       hbm_roof_fraction=fold_bytes / fold_s / HBM_ROOF if fold_s > 0 else None,
                                       expected_factor_ratio=(nt / n) ** 3,
                                       measured_factor_ratio=med(rounds["tied"], "cholesky_s_per_iteration") / med(rounds["new"], "cholesky_s_per_iteration"),
                                       factorisation_saved_s_per_iteration=saved, fold_over_saved=fold_s / saved if saved > 0 else None))
            if a.parent_lib:
                p, nw = [r["lm_iterations_per_s"] for r in rounds["parent"]], float(np.median([r["lm_iterations_per_s"] for r in rounds["new"]]))
                case["no_groups_parent"] = _round({"lm_iterations_per_s": p, "iterations": rounds["parent"][0]["iterations"], "final_rms_px": rounds["parent"][0]["final_rms_px"]})
                case["no_groups_ab"] = _round({"parent_min": min(p), "parent_max": max(p), "new_median": nw, "within_parent_spread": bool(min(p) <= nw <= max(p)),
                                               "same_result": bool(rounds["parent"][0]["final_rms_px"] == rounds["new"][0]["final_rms_px"] and
                                                                   rounds["parent"][0]["iterations"] == rounds["new"][0]["iterations"])})
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
