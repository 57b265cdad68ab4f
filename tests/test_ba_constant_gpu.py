"""GPU suite: constant cameras in the bundle adjuster (rcn_ba_solve_constant; csrc/ba.hip builds cam_dim = 0 for them).

Held against: rcn_ba_solve itself (no mask: bit for bit), the CPU oracle with the one constant camera moved to index 0, and the
independent judge of tests/ba_local_ref.py (two or more constant cameras: the gauge is fixed, parameters are comparable; its results
are read from tests/golden/ba_local_judge.npz, which tests/test_ba_local_ref.py holds against a fresh run of the judge)."""
import ctypes as C

import numpy as np
import pytest

import ba_graphs
import ba_local_ref as L
from oracle import orc_ba
from reconstructor_amd import synth_ba

pytestmark = pytest.mark.gpu

COUNTERS = ("iterations", "successful_steps", "unsuccessful_steps", "invalid_steps", "termination", "line_search_backtracks",
            "bound_projections", "reduced_dim", "initial_cost", "final_cost")


def _options(ctx, nc, mode=0, fix=(0, 0), max_iterations=None, **tol):
    from reconstructor_amd import ba
    o = ba.default_options(ctx, nc)
    o.intrinsics_mode, o.fix_cam0_pose, o.fix_cam1_translation = mode, fix[0], fix[1]
    if max_iterations:
        o.max_iterations = max_iterations
    for k, v in tol.items():
        setattr(o, k, v)
    return o


def _through_constant_entry(ctx, sc, o, mask):
    """rcn_ba_solve_constant called directly: mask None is a NULL pointer (ba.solve_flat would take rcn_ba_solve then)."""
    from reconstructor_amd import _lib, ba
    P, I, X = (np.array(sc[k], np.float64, order="C") for k in ("poses", "intrinsics", "points"))
    uv, cam, pt = np.ascontiguousarray(sc["obs_uv"], np.float64), np.ascontiguousarray(sc["obs_cam"], np.int32), np.ascontiguousarray(sc["obs_pt"], np.int32)
    pb = _lib.BaProblem(len(P), len(X), len(cam), 0, P.ctypes.data, I.ctypes.data, X.ctypes.data, uv.ctypes.data, cam.ctypes.data, pt.ctypes.data)
    s = _lib.BaSummary()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ctx.check(ctx.lib.rcn_ba_solve_constant(ctx.h, C.byref(pb), C.byref(o), None, m.ctypes.data if m is not None else None, C.byref(s), None, None))
    return P, I, X, ba.summary_dict(s)


def _same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and all(a[3][k] == b[3][k] for k in COUNTERS) and \
        np.array_equal(a[3]["cost_trace"], b[3]["cost_trace"])


@pytest.mark.parametrize("case", ["mode0_7", "mode1_12"])
def test_no_mask_is_rcn_ba_solve_bit_for_bit(gpu_ctx, case):
    from reconstructor_amd import ba
    if case == "mode0_7":
        sc = ba_graphs.graph_scene(7, 150, 11, lengths=[2, 3, 4, 7])
        o = ba.default_options(gpu_ctx, 7)
    else:
        sc = ba_graphs.graph_scene(12, 250, 12, lengths=[2, 3, 4, 12])
        o = ba.default_options(gpu_ctx, 12)
        o.focal_upper_bound = 700.0
        sc["intrinsics"][5, 0] = 706.0                        # starts above the bound: projected at iteration zero
        assert o.intrinsics_mode == 1
    ref = ba.solve_scene(gpu_ctx, sc, o)
    assert ref[3]["bound_projections"] == (1 if case == "mode1_12" else 0) and ref[3]["final_cost"] < ref[3]["initial_cost"]
    assert _same_bits(_through_constant_entry(gpu_ctx, sc, o, None), ref)
    assert _same_bits(_through_constant_entry(gpu_ctx, sc, o, np.zeros(len(sc["poses"]), np.uint8)), ref)
    assert _same_bits(ba.solve_scene(gpu_ctx, sc, o, constant=np.zeros(len(sc["poses"]), bool)), ref)


@pytest.mark.parametrize("nc,npts,seed,const", L.ONE_CONSTANT)
def test_one_constant_camera_is_the_oracle_with_it_at_index_0(gpu_ctx, nc, npts, seed, const):
    """index 0 (12 cameras), the middle (6) and the last (8).  The scale is free: only the RMS is compared."""
    from reconstructor_amd import ba
    sc = L.scene(nc, npts, seed)
    c = const[0]
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, nc), constant=L.mask(nc, const))
    perm, _ = L.permuted_to_front(sc, c)
    o = orc_ba.default_options(nc)
    o.intrinsics_mode, o.fix_cam0_pose, o.fix_cam1_translation = 0, 1, 0
    _, _, _, s0 = orc_ba.solve(perm, o, threads=4)
    print("constant camera %d of %d: %d iterations (oracle %d), termination %d (%d), rms %.9f px (oracle %.9f, difference %.2e)" %
          (c, nc, s["iterations"], s0["iterations"], s["termination"], s0["termination"], s["final_rms_px"], s0["final_rms_px"], abs(s["final_rms_px"] - s0["final_rms_px"])))
    assert s["reduced_dim"] == 6 * (nc - 1)
    assert s["iterations"] == s0["iterations"] and s["termination"] == s0["termination"]
    assert abs(s["final_rms_px"] - s0["final_rms_px"]) <= 1e-5
    assert P[c].tobytes() == sc["poses"][c].tobytes() and I[c].tobytes() == sc["intrinsics"][c].tobytes()
    assert I.tobytes() == sc["intrinsics"].tobytes()             # mode 0: no intrinsics move


@pytest.mark.parametrize("nc,npts,seed,const", L.MANY_CONSTANT)
def test_constant_sets_against_the_judge(gpu_ctx, nc, npts, seed, const):
    """Margins: 100 x what the judge's two minimisers (trf, dogbox) differ by on the same scene, floor 1e-9 -- the spread is what two
    correct minimisers differ by, a factor of 100 covers a third."""
    from reconstructor_amd import ba
    sc = L.scene(nc, npts, seed)
    m = L.mask(nc, const)
    Pj, Xj, rj, (s_rms, s_pose, s_pts) = L.recorded(nc, npts, seed, const)
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, nc, max_iterations=150, **L.TO_THE_END), constant=m)
    seen = np.zeros(npts, bool)
    seen[sc["obs_pt"]] = True
    d_rms, d_pose, d_pts = abs(s["final_rms_px"] - rj), np.abs(P - Pj).max(), np.abs(X - Xj)[seen].max()
    print("constant %s of %d: %d iterations, termination %d; against the judge: rms %.2e px, poses %.2e (margin %.2e), points %.2e (margin %.2e)" %
          (const, nc, s["iterations"], s["termination"], d_rms, d_pose, max(100 * s_pose, 1e-9), d_pts, max(100 * s_pts, 1e-9)))
    assert s["reduced_dim"] == 6 * (nc - len(const))
    assert P[m].tobytes() == sc["poses"][m].tobytes() and I.tobytes() == sc["intrinsics"].tobytes()
    assert X[~seen].tobytes() == sc["points"][~seen].tobytes()
    assert d_rms <= 1e-5
    assert d_pose <= max(100 * s_pose, 1e-9) and d_pts <= max(100 * s_pts, 1e-9)


def test_mode_1_leaves_a_constant_camera_s_focal_above_the_bound(gpu_ctx):
    from reconstructor_amd import ba
    sc = ba_graphs.graph_scene(12, 250, 12, lengths=[2, 3, 4, 12])
    o = ba.default_options(gpu_ctx, 12)                           # mode 1, camera 0's pose and camera 1's translation held
    o.focal_upper_bound = 700.0
    sc["intrinsics"][2, 0] = sc["intrinsics"][2, 1] = 706.0         # constant camera: both focal lengths above the bound
    sc["intrinsics"][5, 0] = 707.0                                # free camera: one
    m = L.mask(12, (2, 7))
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, o, constant=m)
    assert s["reduced_dim"] == 10 * 12 - 6 - 3 - 2 * 10
    assert I[m].tobytes() == sc["intrinsics"][m].tobytes() and P[m].tobytes() == sc["poses"][m].tobytes()
    assert I[2, 0] == 706.0 and I[5, 0] <= 700.0 and s["bound_projections"] == 1
    assert (np.delete(I, [2], axis=0)[:, :2] <= 700.0).all()
    assert s["final_cost"] < s["initial_cost"]
    free = ~m
    assert not np.array_equal(I[free][:, [0, 1, 4, 5]], sc["intrinsics"][free][:, [0, 1, 4, 5]])      # the free cameras' intrinsics did move
    assert np.array_equal(I[:, 2:4], sc["intrinsics"][:, 2:4])    # the principal point never does


def _reversed_cameras(sc):
    nc = len(sc["poses"])
    out = ba_graphs.copy_scene(sc)
    for k in ("poses", "intrinsics"):
        out[k] = np.ascontiguousarray(sc[k][::-1])
    out["obs_cam"] = np.ascontiguousarray((nc - 1 - sc["obs_cam"]).astype(np.int32))
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("const", [(0, 1, 2), (4, 5, 6), (9, 10, 11)], ids=["front", "middle", "end"])
def test_runs_of_constant_cameras_wherever_they_stand(gpu_ctx, const, mode):
    """The kernels find the camera of a reduced coordinate by a search over cam_off that steps over cam_dim == 0.  The same problem with
    the camera order reversed puts the run at the other end (front <-> end, the middle moved by one): both orders must find the same
    minimum -- three constant cameras fix the gauge, so the parameters are comparable, to the project's 1e-5 px in the RMS."""
    from reconstructor_amd import ba
    sc = L.scene(12, 300, 3)
    m = L.mask(12, const)
    o = _options(gpu_ctx, 12, mode=mode, max_iterations=150, **L.TIGHT)
    Pa, Ia, Xa, sa = ba.solve_scene(gpu_ctx, sc, o, constant=m)
    Pb, Ib, Xb, sb = ba.solve_scene(gpu_ctx, _reversed_cameras(sc), o, constant=m[::-1])
    assert sa["reduced_dim"] == sb["reduced_dim"] == (6 if mode == 0 else 10) * 9
    assert Pa[m].tobytes() == sc["poses"][m].tobytes() and Ia[m].tobytes() == sc["intrinsics"][m].tobytes()
    assert sa["final_cost"] < 0.1 * sa["initial_cost"]
    print("constant %s mode %d: rms %.9f / %.9f px, poses differ by %.2e, points by %.2e" %
          (const, mode, sa["final_rms_px"], sb["final_rms_px"], np.abs(Pa - Pb[::-1]).max(), np.abs(Xa - Xb).max()))
    assert abs(sa["final_rms_px"] - sb["final_rms_px"]) <= 1e-5
    if mode == 0:      # (mode 1: k1 / k2 and the focal lengths of cameras with few landmarks are loose directions; the RMS is the criterion there)
        assert np.abs(Pa - Pb[::-1]).max() <= 1e-5


def test_a_single_free_camera(gpu_ctx):
    from reconstructor_amd import ba
    sc = L.scene(6, 120, 1)
    for free, fix, n in ((3, (0, 0), 6), (1, (1, 1), 3), (0, (0, 0), 6)):
        m = ~L.mask(6, (free,))
        P, I, X, s = ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, 6, fix=fix), constant=m)
        assert s["reduced_dim"] == n and s["final_cost"] < s["initial_cost"]
        assert P[m].tobytes() == sc["poses"][m].tobytes() and P[free].tobytes() != sc["poses"][free].tobytes()
        if n == 3:
            assert P[1, 3:].tobytes() == sc["poses"][1, 3:].tobytes()      # camera 1's translation stays held by the option


def test_reduced_dimension_a_multiple_of_128(gpu_ctx):
    """64 free cameras x 6 columns = 384 = three blocks of the factorisation exactly (no padded row), beside two constant ones."""
    from reconstructor_amd import ba
    sc = ba_graphs.graph_scene(66, 660, 5, lengths=[2, 3, 4])
    assert 25 <= np.bincount(sc["obs_cam"], minlength=66).mean() <= 35
    m = L.mask(66, (10, 40))
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, 66), constant=m)
    assert s["reduced_dim"] == 384 and s["invalid_steps"] == 0
    assert s["final_cost"] < 0.1 * s["initial_cost"] and s["final_rms_px"] < 1.0
    assert P[m].tobytes() == sc["poses"][m].tobytes() and not np.array_equal(P[~m], sc["poses"][~m])


def test_all_cameras_constant_is_an_argument_error(gpu_ctx):
    from reconstructor_amd import _lib, ba
    sc = L.scene(6, 120, 1)
    with pytest.raises(_lib.RcnError) as e:
        ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, 6), constant=np.ones(6, bool))
    assert e.value.code == -1 and "no free parameter" in str(e.value)
    with pytest.raises(_lib.RcnError) as e:                       # cameras 1 .. 5 constant, camera 0 held by the option
        ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, 6, fix=(1, 1)), constant=~L.mask(6, (0,)))
    assert e.value.code == -1
    assert ba.solve_scene(gpu_ctx, sc)[3]["final_rms_px"] < 1.0   # the ctx is usable afterwards


def test_two_masked_solves_give_equal_bits(gpu_ctx):
    from reconstructor_amd import ba
    sc = L.scene(12, 300, 3)
    o, m = _options(gpu_ctx, 12, mode=1), L.mask(12, (0, 4, 11))
    a, b = ba.solve_scene(gpu_ctx, sc, o, constant=m), ba.solve_scene(gpu_ctx, sc, o, constant=m)
    assert _same_bits(a, b)
    c = ba.solve_scene(gpu_ctx, sc, o, constant=L.mask(12, (0, 4)))       # same graph, another mask: the pair lists are not reused
    assert c[3]["pair_lists_reused"] == 0 and c[3]["reduced_dim"] == 100 and c[0][11].tobytes() != sc["poses"][11].tobytes()


def test_a_robust_loss_with_a_mask(gpu_ctx):
    from reconstructor_amd import ba
    sc = L.scene(8, 200, 2)
    sc["obs_uv"] = sc["obs_uv"].copy()
    sc["obs_uv"][::17] += 25.0                                    # outliers for the loss to hold down
    m = L.mask(8, (2, 5))
    P, I, X, s = ba.solve_scene(gpu_ctx, sc, _options(gpu_ctx, 8), loss=("huber", 2.0), report=True, constant=m)
    assert s["final_cost"] < s["initial_cost"] and s["loss_report"]["n_beyond_scale"] > 0
    assert P[m].tobytes() == sc["poses"][m].tobytes()
