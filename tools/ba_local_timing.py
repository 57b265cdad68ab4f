"""What a local bundle adjustment costs on a large session, beside the global solve it replaces, at cfg 4 and
cfg 5 size (synth_ba.make_scene, 200 cameras / 200k observations and 1000 cameras / 1M observations) held in an rcn_ba_session.

For windows of 1 + {5, 10, 20} cameras -- the last camera and the ones that share the most landmarks with it -- it records
  covisible_s     rcn_ba_session_covisible (counts on the device, the choice on the host), the observation arrays already resident;
                  flatten_s beside it: the first call on a fresh session, which also flattens the tracks on the host and uploads them
  extract_s       the extraction on the device and the copy back of the sub-problem's structure
  solve_call_s    rcn_int_ba_solve on the sub-problem: its host-side structure pass and workspace set-up, and inside it
  lm_loop_s       the Levenberg-Marquardt loop (rcn_ba_summary.solve_seconds), with its iterations
  scatter_s       the solved points back into the session's array
  the sub-problem's sizes (cameras, of them constant, landmarks, observations)
and, for the same session, the global rcn_ba_session_solve (wall, LM loop, iterations).  A window is timed on a fresh session, after the
same call on another fresh session has warmed the allocations up.  Host clock around calls that end synchronised.

With --parent-lib PATH (a librcn.so built from the parent commit) the global, no-mask session solve is also timed with THAT library,
parent and new alternating, --rounds each: the new library passes when the median of its LM iterations per second lies within the
spread (min .. max) of the parent's own rounds, as tools/ba_loss_timing.py judged the robust losses.  Nothing tighter is claimed.

Every measurement is a process of its own (one library per process).  The scenes are made once and handed to the workers in a
temporary file.  Fails without a GPU.  Writes --out (default profiles/ba_local_timing.json), stamped with the source hash.

    python tools/ba_local_timing.py [--parent-lib PATH] [--rounds 3] [--solves 2] [--cfgs 4,5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = {4: (200, 20000), 5: (1000, 100000)}
WINDOWS = (5, 10, 20)


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ba_local_timing: no GPU")
    return torch


def worker_global(a):
    """the global session solve through one library's C ABI (entries both the parent and this tree have): one JSON line"""
    _need_gpu()
    from reconstructor_amd._lib import BaOptions, BaSummary      # struct layouts of include/rcn.h (unchanged since the parent)
    sc = dict(np.load(a.scene))
    L = C.CDLL(a.lib)
    vp, i32 = C.c_void_p, C.c_int32
    L.rcn_create.argtypes, L.rcn_destroy.argtypes = [C.c_int, C.POINTER(vp)], [vp]
    L.rcn_last_error.restype, L.rcn_last_error.argtypes = C.c_char_p, [vp]
    L.rcn_ba_session_create.argtypes, L.rcn_ba_session_destroy.argtypes = [vp, C.POINTER(vp)], [vp]
    L.rcn_ba_session_add_camera.argtypes = [vp, vp, vp, vp]
    L.rcn_ba_session_add_points.argtypes = [vp, i32, vp, vp]
    L.rcn_ba_session_add_observations.argtypes = [vp, i32, vp, vp, vp]
    L.rcn_ba_session_solve.argtypes = [vp, vp, C.POINTER(BaSummary)]
    h = vp()
    assert L.rcn_create(0, C.byref(h)) == 0, "rcn_create"
    P, K, X = (np.ascontiguousarray(sc[k], np.float64) for k in ("poses", "intrinsics", "points"))
    pt, cam, xy = np.ascontiguousarray(sc["obs_pt"], np.int32), np.ascontiguousarray(sc["obs_cam"], np.int32), np.ascontiguousarray(sc["obs_uv"].astype(np.int32))
    runs = []
    for i in range(a.solves + 1):
        s = vp()
        assert L.rcn_ba_session_create(h, C.byref(s)) == 0
        for c in range(len(P)):
            assert L.rcn_ba_session_add_camera(s, P[c].ctypes.data, K[c].ctypes.data, None) == 0
        assert L.rcn_ba_session_add_points(s, len(X), X.ctypes.data, None) == 0
        assert L.rcn_ba_session_add_observations(s, len(pt), pt.ctypes.data, cam.ctypes.data, xy.ctypes.data) == 0
        sm = BaSummary()
        t0 = time.perf_counter()
        rc = L.rcn_ba_session_solve(s, None, C.byref(sm))
        wall = time.perf_counter() - t0
        assert rc == 0, L.rcn_last_error(h).decode()
        if i:          # (the first session is the warm-up)
            runs.append(dict(iterations=sm.iterations, solve_seconds=sm.solve_seconds, wall_seconds=wall, final_rms_px=sm.final_rms_px, termination=sm.termination))
        L.rcn_ba_session_destroy(s)
    L.rcn_destroy(h)
    print(json.dumps(dict(n_obs=len(pt), iterations=runs[0]["iterations"], termination=runs[0]["termination"], final_rms_px=runs[0]["final_rms_px"],
                          lm_iterations_per_s=sum(r["iterations"] for r in runs) / sum(r["solve_seconds"] for r in runs),
                          lm_loop_s=float(np.median([r["solve_seconds"] for r in runs])), wall_s=float(np.median([r["wall_seconds"] for r in runs])))))


def worker_local(a):
    """the windows on this tree's library: one JSON line"""
    _need_gpu()
    from reconstructor_amd import _lib, ba
    sc = dict(np.load(a.scene))
    ctx = _lib.Context(0)
    nc = len(sc["poses"])
    xy = sc["obs_uv"].astype(np.int32)

    def session():
        ses = ba.BaSession(ctx)
        for p, k in zip(sc["poses"], sc["intrinsics"]):
            ses.add_camera(p, k)
        ses.add_points(sc["points"])
        ses.add_observations(sc["obs_pt"], sc["obs_cam"], xy)
        return ses

    def clock(f):
        t0 = time.perf_counter()
        r = f()
        return r, time.perf_counter() - t0

    out = {}
    for k in WINDOWS:
        rec = None
        for timed in (False, True):
            ses = session()
            (near, counts), t_first = clock(lambda: ses.covisible(nc - 1, k))
            (near, counts), t_cov = clock(lambda: ses.covisible(nc - 1, k))
            free = np.concatenate([[nc - 1], near])
            o = ba.default_options(ctx, len(free))
            o.fix_cam0_pose = o.fix_cam1_translation = 0
            (s, info), t_call = clock(lambda: ses.solve_local(free, o))
            t_ext, t_solve, t_sc = ses.local_seconds()
            rec = dict(window=1 + len(near), shared_landmarks=[int(counts[c]) for c in near[:3]], flatten_s=t_first - t_cov, covisible_s=t_cov, extract_s=t_ext,
                       solve_call_s=t_solve, lm_loop_s=s["solve_seconds"], scatter_s=t_sc, call_s=t_call, iterations=s["iterations"], termination=s["termination"],
                       reduced_dim=s["reduced_dim"], rms_px=[s["initial_rms_px"], s["final_rms_px"]], **info)
            ses.close()
        out["window_%d" % (1 + k)] = rec
    for timed in (False, True):
        ses = session()
        s, wall = clock(lambda: ses.solve())
        out["global"] = dict(wall_s=wall, lm_loop_s=s["solve_seconds"], iterations=s["iterations"], termination=s["termination"], reduced_dim=s["reduced_dim"],
                             rms_px=[s["initial_rms_px"], s["final_rms_px"]], n_cams=nc, n_points=len(sc["points"]), n_obs=len(sc["obs_pt"]))
        ses.close()
    ctx.close()
    print(json.dumps(out))


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
    ap.add_argument("--worker", choices=["global", "local"], default=None)
    ap.add_argument("--lib", default=os.path.join(ROOT, "reconstructor_amd", "librcn.so"))
    ap.add_argument("--scene", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solves", type=int, default=2)
    ap.add_argument("--cfgs", default="4,5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_local_timing.json"))
    a = ap.parse_args()
    if a.worker:
        return worker_global(a) if a.worker == "global" else worker_local(a)
    torch = _need_gpu()
    import bench
    from reconstructor_amd import synth_ba
    out = {"tool": "ba_local_timing", "source_hash": bench.source_hash(), "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "solves_per_round": a.solves,
           "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for cfg in (int(v) for v in a.cfgs.split(",")):
            nc, npts = CFG[cfg]
            sc = synth_ba.make_scene(nc, npts, obs_per_point=10, seed=2024)
            path = os.path.join(tmp, "cfg%d.npz" % cfg)
            np.savez(path, **{k: sc[k] for k in ("poses", "intrinsics", "points", "obs_uv", "obs_cam", "obs_pt")})
            case = out["cases"]["cfg%d" % cfg] = {}
            rounds = {"new": [], "parent": []}
            for _ in range(a.rounds):          # parent and new alternate
                if a.parent_lib:
                    rounds["parent"].append(measure(["--worker", "global", "--lib", a.parent_lib, "--scene", path, "--solves", str(a.solves)]))
                rounds["new"].append(measure(["--worker", "global", "--lib", a.lib, "--scene", path, "--solves", str(a.solves)]))
            for who, rs in rounds.items():
                if rs:
                    case["global_no_mask_" + who] = _round({"lm_iterations_per_s": [r["lm_iterations_per_s"] for r in rs], "iterations": rs[0]["iterations"],
                                                            "final_rms_px": rs[0]["final_rms_px"]})
            if a.parent_lib:
                p, n = [r["lm_iterations_per_s"] for r in rounds["parent"]], float(np.median([r["lm_iterations_per_s"] for r in rounds["new"]]))
                case["global_no_mask_ab"] = _round({"parent_min": min(p), "parent_max": max(p), "new_median": n, "within_parent_spread": bool(min(p) <= n <= max(p)),
                                                    "same_result": bool(rounds["parent"][0]["final_rms_px"] == rounds["new"][0]["final_rms_px"] and
                                                                        rounds["parent"][0]["iterations"] == rounds["new"][0]["iterations"])})
            case.update(_round(measure(["--worker", "local", "--scene", path])))
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
