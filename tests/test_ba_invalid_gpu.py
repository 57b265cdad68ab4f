"""Invalid LM steps on every path that builds the reduced system (csrc/ba.hip, rcn_int_ba_solve) against the CPU oracle, which is the
specification: a step is invalid when a landmark's damped 3 x 3 block is singular, when the factorisation of the reduced camera system
breaks down, when the step is not finite or when the model cost change is not positive.

The scenes (tests/ba_invalid.py; tests/test_ba_invalid_ref.py shows on the CPU that they do what is said here) have ONE cause each,
exact in any floating-point arithmetic: "lone" a landmark block that is exactly zero beside a healthy camera system, "dead_first" /
"dead_last" a camera block of S that is exactly zero -- in the first or the last block column -- beside healthy landmark blocks.  The
sizes: n = 384 = npad (the flag words cleared by the host, the rows behind S written by kernels of their own: the unfused finish),
n = 132 (padded to 256) and n = 27 (one block), both finished by the Schur diagonal launch; n = 27 again in the diagnostic build with
the forward substitution as a launch of its own and with the atomic Schur build, which are unfused at any size.

Everything compared is an integer, a bit pattern or, with the default floor, the final RMS within the 1e-5 px of tests/test_ba_gpu.py;
the step-level tests use tests/test_ba_step_gpu.py's function-type bound as it stands."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_invalid as V
import ba_ref as B
import test_ba_step_gpu as S
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu
RMS_TOL_PX = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, n) for k in V.KINDS for n in V.SIZES]


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# whole solves
@pytest.mark.parametrize("limit", [1, 5])
@pytest.mark.parametrize("kind,n", CASES)
def test_every_step_is_invalid_and_the_solve_fails_where_the_oracle_fails(gpu_ctx, kind, n, limit):
    from reconstructor_amd import ba
    sc = V.scene(kind, n)
    o = V.set_options(ba.default_options(gpu_ctx, V.SIZES[n][0]), n, 0.0, limit)
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, o, allow_failure=True)
    _, _, _, s0 = V.oracle(kind, n, 0.0, limit)
    print(kind, n, limit, "gpu", [s[k] for k in V.INTEGERS], "oracle", [s0[k] for k in V.INTEGERS], "cost", s["initial_cost"], s["final_cost"])
    assert s["reduced_dim"] == n and n % 128 == {384: 0, 132: 4, 27: 27}[n]
    assert [s[k] for k in V.INTEGERS] == [s0[k] for k in V.INTEGERS] == [6, limit, limit, 0, 0, n]
    assert same_bits(P, sc["poses"]) and same_bits(I, sc["intrinsics"]) and same_bits(X, sc["points"])
    assert s["final_cost"] == s["initial_cost"]


@pytest.mark.parametrize("kind,n", CASES)
def test_with_the_default_floor_the_same_scenes_are_solved_as_the_oracle_solves_them(gpu_ctx, kind, n):
    from reconstructor_amd import ba
    sc = V.scene(kind, n)
    o = V.set_options(ba.default_options(gpu_ctx, V.SIZES[n][0]), n)
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, o)
    _, _, _, s0 = V.oracle(kind, n)
    print(kind, n, "gpu", [s[k] for k in V.INTEGERS], s["final_rms_px"], "oracle", [s0[k] for k in V.INTEGERS], s0["final_rms_px"])
    assert s["reduced_dim"] == n and n % 128 == {384: 0, 132: 4, 27: 27}[n]
    assert [s[k] for k in V.INTEGERS] == [s0[k] for k in V.INTEGERS]
    assert abs(s["final_rms_px"] - s0["final_rms_px"]) <= RMS_TOL_PX


_CHILD = r"""
import sys, json
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import ba_invalid as V
from reconstructor_amd import _lib, ba
assert b"DIAGNOSTIC" in _lib.load().rcn_version()
ctx = _lib.Context(0)
out = {}
for kind in V.KINDS:
    sc = V.scene(kind, 27)
    o = V.set_options(ba.default_options(ctx, V.SIZES[27][0]), 27, 0.0, 5)
    P, I, X, s = ba.solve_scene(ctx, sc, o, allow_failure=True)
    out[kind] = dict({k: int(s[k]) for k in V.INTEGERS}, initial_cost=s["initial_cost"], final_cost=s["final_cost"],
                     untouched=bool(P.tobytes() == np.asarray(sc["poses"], np.float64).tobytes() and I.tobytes() == np.asarray(sc["intrinsics"], np.float64).tobytes()
                                    and X.tobytes() == np.asarray(sc["points"], np.float64).tobytes()))
ctx.close()
print(json.dumps(out))
"""


@pytest.mark.parametrize("env", ["RCN_BA_TRSV_FWD", "RCN_BA_SCHUR_ATOMICS"])
def test_the_alternative_device_paths_fail_where_the_oracle_fails(env):
    """n = 27 with the right-hand side solved for by a launch of its own, and with the atomic Schur build: neither finishes the system in
    the Schur diagonal launch.  The switches exist in the diagnostic build only (tools/librcn_diag.so): one child process per switch."""
    diag = os.path.join(ROOT, "tools", "librcn_diag.so")
    assert os.path.exists(diag), "tools/librcn_diag.so missing: run __graft_entry__.build()"
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=dict(os.environ, RCN_LIB=diag, **{env: "1"}),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    print(env, got)
    for kind in V.KINDS:
        _, _, _, s0 = V.oracle(kind, 27, 0.0, 5)
        g = got[kind]
        assert [g[k] for k in V.INTEGERS] == [s0[k] for k in V.INTEGERS] == [6, 5, 5, 0, 0, 27], (env, kind, g)
        assert g["untouched"] and g["final_cost"] == g["initial_cost"], (env, kind, g)


@pytest.mark.parametrize("structure", ["n384", "defaults"])
def test_no_flag_word_outlives_a_failed_solve(structure):
    """one context: the lone-landmark scene at n = 384 to FAILURE, then an ordinary scene of the same size -- with the same options
    (n = 384 again: the unfused finish) and with the defaults (the bounded-intrinsics branch, the fused finish); outputs and summary
    equal, bit for bit, those of the same solve on a context that has never seen a failure"""
    import torch  # noqa: F401  (first: one shared HIP runtime)
    from reconstructor_amd import _lib, ba
    sc = synth_ba.make_scene(65, 650, obs_per_point=4)

    def ordinary(ctx):
        o = ba.default_options(ctx, 65)
        if structure == "n384":
            V.set_options(o, 384)
        return ba.solve_scene(ctx, sc, o)

    used = _lib.Context(0)
    try:
        bad = V.scene("lone", 384)
        _, _, _, sf = ba.solve_scene(used, bad, V.set_options(ba.default_options(used, 65), 384, 0.0, 5), allow_failure=True)
        assert sf["termination"] == 6 and sf["invalid_steps"] == 5 and sf["reduced_dim"] == 384
        P1, I1, X1, s1 = ordinary(used)
    finally:
        used.close()
    fresh = _lib.Context(0)
    try:
        P2, I2, X2, s2 = ordinary(fresh)
    finally:
        fresh.close()
    print(structure, {k: s1[k] for k in V.INTEGERS}, s1["final_cost"], s2["final_cost"])
    assert s1["reduced_dim"] == (384 if structure == "n384" else 641) and s1["invalid_steps"] == 0 and s1["successful_steps"] >= 2
    assert same_bits(P1, P2) and same_bits(I1, I2) and same_bits(X1, X2)
    for k in s2:
        if k == "cost_trace":
            assert same_bits(s1[k], s2[k])
        elif not k.endswith("_seconds"):
            assert s1[k] == s2[k], (k, s1[k], s2[k])


# ---------------------------------------------------------------------------------------------------------------------
# one step: the decision charged to the kernel that made it (tools/ba_step_check, as in tests/test_ba_step_gpu.py)
def invalid_case(name, scene, n, iteration):
    c = S.case(name, scene, iteration=iteration, mode=0, fix0=1, fix1=V.SIZES[n][1])
    c["lm"] = (0.0, S.HI)          # no floor under the LM diagonal; the ceiling as rcn_ba_default_options gives it
    return c


def common_checks(rep, sc, c, cap, n, skip=()):
    """what every invalid step must leave, whatever made it invalid; the landmark blocks listed in `skip` are judged by the caller"""
    npts = len(sc["points"])
    rep.exact("n / npad", (cap["n"], cap["npad"]) == (n, B.padded(n)))
    rep.exact("finish: fused_finish %d rhs_row %d fin %d" % (cap["fused_finish"], cap["rhs_row"], cap["fin"]),
              (cap["fused_finish"], cap["rhs_row"], cap["fin"] >= 0) == ((1, 1, True) if n % 128 else (0, 0, False)))
    rep.exact("captures (A %d, B %d)" % (cap["got_a"], cap["got_b"]), cap["got_a"] == 1 and cap["got_b"] == 2)
    rep.exact("flag words at A other than [0]", not cap["flag"][1:].any())
    rep.exact("flag words at B (reduction tickets [8:12], the landmark kernels' word [1])", not cap["flag_b"][8:12].any() and cap["flag_b"][1] == 0)
    rep.exact("ticket words", not cap["tickets"].any() and not cap["tickets_b"].any())
    dv = cap["Vraw"].reshape(-1, 9)[:, ::4].reshape(-1)
    rep.add("dgp without a floor", S.fn_ratio(cap["dgp"], B.lm_diagonal(dv, cap["sp"], 0.0, S.HI), B.lm_diagonal(dv, cap["sp"], 0.0, S.HI, np.float64)))
    # every other landmark's damped inverse: test_ba_step_gpu.judge's function-type rule, per block
    keep = np.setdiff1d(np.arange(npts), np.asarray(skip, np.int64))
    pick = lambda a, w: np.asarray(cap[a]).reshape(npts, w)[keep].reshape(-1)
    ir = 1.0 / cap["radius"]
    Vi, det, _ = B.point_solve(pick("Vraw", 9), pick("sp", 3), pick("dgp", 3), pick("gpraw", 3), ir)
    Vi64, _, _ = B.point_solve(pick("Vraw", 9), pick("sp", 3), pick("dgp", 3), pick("gpraw", 3), ir, np.float64)
    assert (det > 0).all()
    over = []
    rv = S.fn_ratio(pick("Vinv", 9).reshape(-1, 9), Vi.reshape(-1, 9), Vi64.reshape(-1, 9), axis=1, over=over)
    rep.add("Vinv (%d of %d blocks over)" % (over[0], len(keep)), rv)


@pytest.mark.parametrize("n", [384, 132])
def test_a_singular_landmark_block_is_flagged_by_the_launch_that_solves_it(tmp_path, n):
    """the lone-landmark scene without a floor: at iteration 1 the block is solved in k_ba_gradmax's launch, at iteration 2 -- behind an
    invalid step -- by k_ba_point_solve; either way flag[0] stands when the reduced system is complete (capture A), the step leaves
    through the invalid-step exit, and the block's inverse is nine zeros"""
    sc = V.scene("lone", n)
    lone = len(sc["points"]) - 1
    cases = [invalid_case("lone%d_it%d" % (n, it), "lone", n, it) for it in (1, 2)]
    caps = S.run_tool(tmp_path, {"lone": sc}, cases)
    for c in cases:
        cap = caps[c["name"]]
        rep = S.Report(c["name"])
        common_checks(rep, sc, c, cap, n, skip=[lone])
        rep.exact("flag[0] at A = %d" % cap["flag"][0], cap["flag"][0] == 1)
        rep.exact("the flag word read with the step's scalars = %r" % cap["scal"][13], cap["scal"][13] == 1.0)
        rep.exact("the lone block: Vraw and dgp zero, Vinv nine zeros",
                  not cap["Vraw"].reshape(-1, 9)[lone].any() and not cap["dgp"].reshape(-1, 3)[lone].any() and
                  np.array_equal(cap["Vinv"].reshape(-1, 9)[lone].view(np.uint64), np.zeros(9, np.uint64)))
        if c["iteration"] == 2:
            log = cap["log"].reshape(-1, 15)
            rep.exact("iteration 1 was invalid (its flag word %r, the radius now %r)" % (log[0, 13], cap["radius"]), log[0, 13] == 1.0 and cap["radius"] == 1e4 / 2)
        else:
            rep.exact("radius", cap["radius"] == 1e4)
        rep.done()


@pytest.mark.parametrize("kind", ["dead_first", "dead_last"])
def test_a_zero_camera_block_is_flagged_by_the_factorisation(tmp_path, kind):
    """the dead-camera scene at n = 384 without a floor: every landmark block is fine, so no flag word is up when the reduced system is
    complete; the camera's diagonal block of S is exactly zero, the factorisation raises its breakdown value, and that is what comes
    home with the step's scalars"""
    n = 384
    sc = V.scene(kind, n)
    nc = len(sc["poses"])
    dead = 1 if kind == "dead_first" else nc - 1
    c = invalid_case(kind, "dead", n, 1)
    cap = S.run_tool(tmp_path, {"dead": sc}, [c])[c["name"]]
    rep = S.Report(c["name"])
    common_checks(rep, sc, c, cap, n)
    rep.exact("flag[0] at A = %d" % cap["flag"][0], cap["flag"][0] == 0)
    _, dim, off = B.structure(nc, 0, 1, V.SIZES[n][1])
    blk = cap["S"].reshape(n, n)[off[dead]:off[dead + 1], off[dead]:off[dead + 1]]
    rep.exact("the dead camera's block of S is zero", (off[dead], off[dead + 1]) == ((0, 6) if dead == 1 else (n - 6, n)) and not np.tril(blk).any())
    rep.exact("the flag word read with the step's scalars = %r: the factorisation's breakdown" % cap["scal"][13], cap["scal"][13] == 1.0 and cap["flag_b"][0] == 1)
    rep.done()
