"""CPU suite: the judge of shared intrinsics (tests/ba_tied_ref.py) checked itself, and its record for the GPU suite
(tests/golden/ba_tied_judge.npz) held against a fresh run.

  (a) without groups and with the intrinsics held it ends where tests/ba_local_ref.py's judge ends; trust-region reflective and
      dogbox end at the same tied minimum;
  (b) without groups its step is tests/ba_ref.py's full step;
  the scenes' reason to exist: with one true camera and 0.5 px noise, the tied minimum's focal length is nearer the truth than the
  mean of the focal lengths the cameras find each on its own (over four weakly observed scenes; the test says why not on one)."""
import numpy as np

import ba_graphs
import ba_local_ref as L
import ba_ref as B
import ba_tied_ref as T


def test_without_groups_the_minimiser_is_ba_local_refs():
    nc, npts, seed, const = L.MANY_CONSTANT[0]
    sc, m = L.scene(nc, npts, seed), L.mask(nc, const)
    Pj, Xj, rj = L.judged(nc, npts, seed, const)
    P, I, X, r = T.judge(sc, None, m, fix=(0, 0), mode=0)
    seen = np.zeros(npts, bool)
    seen[sc["obs_pt"]] = True
    print("rms %.3e, poses %.3e, points %.3e" % (abs(r - rj), np.abs(P - Pj).max(), np.abs(X - Xj)[seen].max()))
    assert I.tobytes() == sc["intrinsics"].tobytes()
    assert abs(r - rj) <= 1e-12 and np.abs(P - Pj).max() <= 1e-9 and np.abs(X - Xj)[seen].max() <= 1e-8


def test_trf_against_dogbox_and_the_record():
    name = "one_group_12"
    sc, kw = T.case(name)
    a, b, rec = T.judged(name, "trf"), T.judged(name, "dogbox"), T.recorded(name)
    seen = np.zeros(len(a[2]), bool)
    seen[sc["obs_pt"]] = True
    d = (abs(a[3] - b[3]), np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2])[seen].max())
    print("trf - dogbox: rms %.2e, poses %.2e, intrinsics %.2e, points %.2e; recorded spread %s" % (d + (rec["spread"],)))
    assert d[0] <= 1e-10 and d[1] <= 1e-7 and d[2] <= 1e-4 and d[3] <= 1e-6
    assert (a[1] == a[1][0]).all()      # one group of all cameras: one set of intrinsics
    # the record is this run (same code, same inputs: up to the libraries' own rounding)
    assert abs(a[3] - float(rec["rms"])) <= 1e-10
    assert np.abs(a[0] - rec["P"]).max() <= 1e-7 and np.abs(a[1] - rec["I"]).max() <= 1e-4 and np.abs(a[2] - rec["X"])[seen].max() <= 1e-6
    st = T.stepped(name)
    for k in ("P", "I", "X"):
        assert np.abs(np.asarray(st["d" + k], np.float64) - rec["d" + k]).max() <= 1e-12 * max(1.0, np.abs(rec["d" + k]).max())
    assert rec["I0"].tobytes() == np.asarray(st["intr0"], np.float64).tobytes()


def test_every_case_is_recorded_with_its_layout():
    want = {"one_group_12": 67, "one_group_20": 115, "exactly_128": 128, "n_138": 138, "two_groups_66": 395}
    for name, c in T.CASES.items():
        sc, kw = T.case(name)
        rec = T.recorded(name)
        st = T.structure(c["nc"], kw["groups"], kw["constant"], 1, kw["fix"])
        assert st["n_tied"] == want.get(name, st["n_tied"]), name
        assert rec["P"].shape == (c["nc"], 6) and rec["dX"].shape == (c["npts"], 3) and rec["spread"].shape == (4,), name
        g = np.asarray(kw["groups"])
        assert all((sc["intrinsics"][g == k] == sc["intrinsics"][g == k][0]).all() for k in np.unique(g[g >= 0])), name
    sc, kw = T.case("one_group_20")
    assert T.structure(20, None)["n"] == 191 and B.padded(191) == 256 and B.padded(115) == 128


def test_without_groups_the_step_is_ba_refs():
    sc, kw = T.case("mixed_12")
    for real, tol in ((T.LD, 1e-15), (np.float64, 1e-9)):
        a = T.tied_step(sc, None, real=real)
        f = B.full_step(sc, dict(mode=1, fix0=1, fix1=1, jacobi=1, ub=1000.0, lo=1e-6, hi=1e32), 1e4, real)
        st = T.structure(12, None)
        assert st["n"] == st["n_tied"] == len(f["dlc"]) and (st["map"] == np.arange(st["n"])).all()
        d = np.concatenate([[a["dP"][c, col] if col < 6 else a["dI"][c, col - 6] for col in st["cols"][c, :st["dim"][c]]] for c in range(12)])
        e = float(max(np.abs(d - f["dlc"]).max() / np.abs(f["dlc"]).max(), np.abs(a["dX"].reshape(-1) - f["dlp"]).max() / np.abs(f["dlp"]).max()))
        print(real.__name__, "relative difference %.2e" % e)
        assert e <= tol


def test_a_tied_focal_length_is_nearer_the_truth():
    """Scenes with one true camera and 0.5 px noise, about 15 observations per camera (where a camera's own focal length is weakly held, which
    is what sharing is for): the tied minimum's focal length against the mean of the focal lengths the cameras find each on its own.  On ONE
    scene neither has to win -- to first order the mean of twelve unbiased estimates is as good as the pooled one (on the well-observed
    12-camera case of the GPU suite: tied off by 0.403, the untied mean by 0.058, the single cameras by 2.6 on average) -- so the comparison
    is over four scenes, root mean square; a single camera of its own is further off on every one of them."""
    truth = 1.2 * 512      # synth_ba.make_scene's focal length, every camera's
    tied, own_mean = [], []
    for seed in (41, 42, 43, 44):
        sc = ba_graphs.graph_scene(12, 70, seed, lengths=[2, 3])
        t, o = T.judge(sc, np.zeros(12, np.int32))[1], T.judge(sc, None)[1]
        assert (t == t[0]).all()
        tied.append(t[0, 0] - truth)
        own_mean.append(o[:, 0].mean() - truth)
        print("seed %d, %.1f observations per camera, true fx %.3f: tied %.3f (off by %.3f), untied mean %.3f (off by %.3f), single cameras off by %.3f on average" %
              (seed, len(sc["obs_cam"]) / 12, truth, t[0, 0], abs(tied[-1]), o[:, 0].mean(), abs(own_mean[-1]), np.abs(o[:, 0] - truth).mean()))
        assert abs(tied[-1]) < np.abs(o[:, 0] - truth).mean()
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print("over the four scenes: tied off by %.3f rms, the untied mean by %.3f rms" % (rms(tied), rms(own_mean)))
    assert rms(tied) < rms(own_mean)
