"""CPU only: the scenes of tests/ba_invalid.py do what tests/test_ba_invalid_gpu.py uses them for.  The oracle (oracle/ba_oracle.c, the
specification of an invalid LM step) ends every one of them in FAILURE after exactly `limit` steps without a floor under the LM
diagonal and solves it with the default floor; each scene has ONE cause of failure -- shown on the Jacobians, which are exactly zero
where the scene says so, and by taking the cause away."""
import numpy as np
import pytest

import ba_invalid as V
import ba_ref as B
from oracle import orc_ba
from reconstructor_amd import synth_ba

CASES = [(k, n) for k in V.KINDS for n in V.SIZES]
FREE = [0, 1, 2, 3, 4, 5, 12, 13, 14]          # pose and point columns of the oracle's 2 x 15 Jacobian


def jacobians(sc):
    """[N, 2, 15] = [pose 6 | intrinsics 6 | point 3] per observation, by the oracle's own residual function"""
    return np.stack([orc_ba.residual_jacobian(sc["poses"][c], sc["intrinsics"][c], sc["points"][j], sc["obs_uv"][o])[1]
                     for o, (c, j) in enumerate(zip(sc["obs_cam"], sc["obs_pt"]))])


def landmark_blocks(sc, J):
    Jp = J[:, :, 12:]
    Vb = np.zeros((len(sc["points"]), 3, 3))
    np.add.at(Vb, sc["obs_pt"], np.einsum("oia,oib->oab", Jp, Jp))
    return Vb


@pytest.mark.parametrize("n", list(V.SIZES))
def test_sizes_take_the_paths_they_are_here_for(n):
    nc, fix1 = V.SIZES[n]
    _, dim, off = B.structure(nc, 0, 1, fix1)
    assert int(off[-1]) == n and dim[0] == 0 and (dim[1:] > 0).all()
    assert {384: (0, 384), 132: (4, 256), 27: (27, 128)}[n] == (n % 128, B.padded(n))
    for kind in V.KINDS:
        sc = V.scene(kind, n)
        assert len(sc["poses"]) == nc <= 65 and len(sc["obs_cam"]) <= 2700 and (np.diff(sc["obs_pt"]) >= 0).all()


@pytest.mark.parametrize("n", list(V.SIZES))
def test_lone_landmark_scene_has_a_zero_landmark_block_and_healthy_cameras(n):
    sc = V.scene("lone", n)
    J = jacobians(sc)
    lone = len(sc["points"]) - 1
    assert list(sc["obs_cam"][sc["obs_pt"] == lone]) == [0, 0]
    # (the intrinsics' columns 6 .. 11 are no columns of the problem in mode 0)
    assert not J[sc["obs_cam"] == 0][:, :, FREE].any(), "camera 0's observations must have Jacobians that are exactly zero"
    Vb = landmark_blocks(sc, J)
    assert not Vb[lone].any() and (np.linalg.det(Vb[:lone]) > 0).all()
    live = np.bincount(sc["obs_pt"][sc["obs_cam"] != 0], minlength=lone + 1)
    assert live[lone] == 0 and (live[:lone] >= 3).all()
    # the lone landmark touches camera 0 only, which has no column: without it the same reduced system is solved with no floor at all
    keep = sc["obs_pt"] != lone
    rest = dict(sc, points=sc["points"][:lone], obs_pt=sc["obs_pt"][keep], obs_cam=sc["obs_cam"][keep], obs_uv=np.ascontiguousarray(sc["obs_uv"][keep]))
    o = V.set_options(orc_ba.default_options(len(sc["poses"])), n, floor=0.0)
    _, _, _, s = orc_ba.solve(rest, options=o, threads=4)
    assert s["invalid_steps"] == 0 and s["termination"] == 1 and s["reduced_dim"] == n


@pytest.mark.parametrize("kind,n", [(k, n) for k in V.KINDS[1:] for n in V.SIZES])
def test_dead_camera_scene_has_a_zero_camera_block_and_healthy_landmarks(kind, n):
    sc = V.scene(kind, n)
    nc = len(sc["poses"])
    dead = 1 if kind == "dead_first" else nc - 1
    assert sc["intrinsics"][dead, 0] == 0 == sc["intrinsics"][dead, 1] and (np.delete(sc["intrinsics"][:, :2], dead, 0) > 0).all()
    J = jacobians(sc)
    mine = sc["obs_cam"] == dead
    assert mine.sum() > 0 and not J[mine][:, :, FREE].any(), "the dead camera's observations must have Jacobians that are exactly zero"
    # every other free camera has a block of full rank in the columns it owns
    cols, dim, _ = B.structure(nc, 0, 1, V.SIZES[n][1])
    for c in range(1, nc):
        if c != dead:
            Jc = J[sc["obs_cam"] == c][:, :, cols[c, :dim[c]]].reshape(-1, dim[c])
            assert np.linalg.matrix_rank(Jc) == dim[c]
    assert (np.linalg.det(landmark_blocks(sc, J)) > 0).all()
    assert (np.bincount(sc["obs_pt"][~mine], minlength=len(sc["points"])) >= 3).all()


def test_case_lines_carry_the_lm_diagonal_bounds_only_where_a_case_sets_them(tmp_path):
    """tools/ba_step_check's cases.txt: nine columns as before for a case that leaves the bounds alone, two more -- exact -- otherwise"""
    base = dict(scene="s", iteration=2, mode=0, fix0=1, fix1=0, jacobi=1, ub=1000.0, radius=1e4)
    B.write_cases(str(tmp_path), [dict(base, name="plain"), dict(base, name="none", lm=None), dict(base, name="floorless", lm=(0.0, 1e32))])
    lines = [l.split() for l in open(tmp_path / "cases.txt") if not l.startswith("#")]
    assert [len(l) for l in lines] == [9, 9, 11] and lines[0][1:] == lines[1][1:] == lines[2][1:9]
    assert lines[0] == ["plain", "s", "2", "0", "1", "0", "1", "1000", "10000"]
    assert (float(lines[2][9]), float(lines[2][10])) == (0.0, 1e32)


@pytest.mark.parametrize("limit", [1, 5])
@pytest.mark.parametrize("kind,n", CASES)
def test_without_a_floor_the_oracle_fails_after_exactly_the_limit(kind, n, limit):
    sc = V.scene(kind, n)
    P, I, X, s = V.oracle(kind, n, 0.0, limit)
    assert [s[k] for k in V.INTEGERS] == [6, limit, limit, 0, 0, n], s
    assert P.tobytes() == np.asarray(sc["poses"]).tobytes() and I.tobytes() == np.asarray(sc["intrinsics"]).tobytes() and X.tobytes() == np.asarray(sc["points"]).tobytes()
    assert s["final_cost"] == s["initial_cost"]


@pytest.mark.parametrize("kind,n", CASES)
def test_with_the_default_floor_the_oracle_solves_the_scene(kind, n):
    sc = V.scene(kind, n)
    P, I, X, s = V.oracle(kind, n)
    assert [s[k] for k in V.INTEGERS] == [1, 3, 0, 2, 0, n], s
    assert not np.array_equal(P, sc["poses"]) and not np.array_equal(X, sc["points"]) and s["final_cost"] < s["initial_cost"]
