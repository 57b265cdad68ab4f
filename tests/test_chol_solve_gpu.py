"""The dense Cholesky (csrc/chol.hip, K7) as a unit on the GPU: S x = b through chol.h alone (tools/chol_solve_check, built by
__graft_entry__.build(), is only the driver) against an extended-precision reference (tests/chol_ref.py), at the block counts where the
plan changes regime, with the thresholds shrunk so that every kernel runs at its smallest shape, at the padding edges, over eight
orders of conditioning, for bit-equality between schedules, for the factor itself, and for breakdown.

Tolerances (none of them a number taken from the GPU):
  forward   fwd(x_gpu) <= 16 max(fwd(x_lap), u), x_lap LAPACK's solution of the same system: both are blocked FP64 Cholesky and differ in
            summation order and in applying diagonal blocks through explicit inverses -- a small factor; an indexing or padding bug
            costs ten orders.  A case with kappa >= 1e8 that exceeds it may assert 4 n kappa_2 u instead (solving through explicit block
            inverses); the cases that did are listed in DESIGN.md section 7.2.
  backward  bwd(x_gpu) <= n u for kappa <= 1e4, and the same bound for |S - F F'|_F / |S|_F.
Every test prints its figures before it asserts (pytest -s shows them)."""
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import chol_ref as R

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "chol_solve_check")
DIAG, TRSM_Q, UPD_Q, TRSM_PIPE, UPD_PIPE, SINV, PGEMM, PUBLISH = range(8)


def run_tool(tmp_path, systems, cases, timeout=180):
    """systems: {name: (S, b)}.  One process for the whole list; exit code 0 or the test fails."""
    assert os.path.exists(EXE), "tools/chol_solve_check missing: run __graft_entry__.build()"
    d = str(tmp_path)
    for name, (S, b) in systems.items():
        R.write_system(d, name, S, b)
    R.write_cases(d, cases)
    t0 = time.time()
    r = subprocess.run([EXE, d], capture_output=True, text=True, timeout=timeout)
    print("%d cases in %.2f s" % (len(cases), time.time() - t0))
    print(r.stdout[-6000:])
    assert r.returncode == 0, "chol_solve_check exit code %d\n" % r.returncode + r.stdout[-2000:] + r.stderr[-2000:]
    return {c.name: R.read_result(d, c) for c in cases}


class System:
    """a system with its reference, computed once"""

    def __init__(self, S, b, kappa):
        self.S, self.b, self.n, self.kappa = S, b, S.shape[0], kappa      # kappa: the 2-norm condition number where it is known, else None
        self.x_lap, self.x_ref = R.ref_solve(S, b)
        self.s_norm = R.norm_inf_ld(S)
        self.fwd_lap = R.fwd(self.x_lap, self.x_ref)


def _make(kind, n, arg, seed):
    if kind == "spectrum":
        return System(R.spd_spectrum(n, arg, seed), R.rhs(n, seed), arg)
    if kind == "wishart":        # arg: a scale factor; G G' / n + 0.1 I has its spectrum in [0.1, 0.1 + (1 + 1)^2] up to fluctuations: kappa < 1e2
        return System(R.spd_wishart(n, seed) * arg, R.rhs(n, seed), 1e2)
    if kind == "graded":
        return System(R.graded(R.spd_wishart(n, seed), 1.0 / arg, arg), R.rhs(n, seed), None)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _small(kind, n, arg, seed):
    return _make(kind, n, arg, seed)


def system(kind, n, arg, seed):
    return _small(kind, n, arg, seed) if n <= 1024 else _make(kind, n, arg, seed)      # (the large ones are used once, and are large)


def judge(sysm, res, label, check_bwd=True):
    """the tolerances of the module docstring for one solved case; returns an error string or None, prints the figures"""
    f = R.fwd(res["x"], sysm.x_ref) if np.isfinite(res["x"]).all() else np.inf
    bw = R.bwd(sysm.S, sysm.b, res["x"], sysm.s_norm) if np.isfinite(res["x"]).all() else np.inf
    bound = 16.0 * max(sysm.fwd_lap, R.U)
    escape = ""
    if f > bound and sysm.kappa is not None and sysm.kappa >= 1e8:
        bound = 4.0 * sysm.n * sysm.kappa * R.U
        escape = "  KAPPA ESCAPE (4 n kappa u = %.2e)" % bound
    print("%-34s n %5d  fwd gpu %.2e  lapack %.2e  ratio %8.2f  bwd %.2e (n u = %.1e)  flag %d  schedule %d  %8.3f ms%s"
          % (label, sysm.n, f, sysm.fwd_lap, f / max(sysm.fwd_lap, R.U), bw, sysm.n * R.U, res["flag"], res["schedule"], res["wall_ms"], escape))
    if res["flag"] != 0:
        return "%s: flag %d" % (label, res["flag"])
    if res["schedule"] != 0:
        return "%s: a hand-off timed out, the factorisation was repeated on one stream" % label
    if not f <= bound:
        return "%s: forward error %.3e above %.3e" % (label, f, bound)
    if check_bwd and sysm.kappa is not None and sysm.kappa <= 1e4 and not bw <= sysm.n * R.U:
        return "%s: backward error %.3e above n u = %.3e" % (label, bw, sysm.n * R.U)
    return None


def plan_of(nblk, prm):
    import test_chol_plan as P
    return P.get_plan(nblk, R.plan_array(prm))


def kinds(ops, kind, **kw):
    return [o for o in ops if o["kind"] == kind and all(o[k] == v for k, v in kw.items())]


# ---------------------------------------------------------------------------------------------------------------------
def check_regime_plan(nblk, ops):
    """the operations a regime case is there for: a retune of the defaults fails here instead of hollowing the case"""
    streams = {o["stream"] for o in ops if o["kind"] != PUBLISH}
    if nblk == 1:
        assert [o["kind"] for o in ops] == [DIAG]
    elif nblk == 2:
        assert {o["kind"] for o in ops} == {DIAG, TRSM_Q, UPD_Q}
    elif nblk == 3:
        assert len(streams) == 3 and kinds(ops, UPD_PIPE, nst=16, stream=2)
    elif nblk == 6:
        for k, s in ((TRSM_Q, 0), (UPD_Q, 0), (TRSM_Q, 1), (UPD_Q, 1), (UPD_PIPE, 2)):
            assert kinds(ops, k, stream=s), (k, s)
    elif nblk == 27:
        assert kinds(ops, UPD_PIPE, nst=32, stream=2) and not kinds(ops, TRSM_PIPE)
    elif nblk == 34:
        assert kinds(ops, TRSM_PIPE) and not kinds(ops, SINV)
    elif nblk == 48:
        assert len(kinds(ops, SINV, g=4)) == 8 and {o["dj"] for o in kinds(ops, SINV)} == {0, 1}
        assert kinds(ops, UPD_PIPE, nst=64, stream=2) and kinds(ops, UPD_PIPE, small=1) and kinds(ops, PGEMM, small=1)
        assert [o for o in kinds(ops, PGEMM) if o["fuse_with"] >= 0] and [o for o in kinds(ops, PGEMM, small=0) if o["fuse_with"] < 0]
        assert kinds(ops, TRSM_PIPE) and kinds(ops, UPD_PIPE, nst=32)
    else:
        raise AssertionError(nblk)


@pytest.mark.parametrize("nblk,n", R.REGIMES)
def test_regimes_at_the_shipping_parameters(tmp_path, nblk, n):
    check_regime_plan(nblk, plan_of(nblk, R.SHIP))
    assert (n + R.BLOCK - 1) // R.BLOCK == nblk
    t0 = time.time()
    sysm = system("spectrum", n, 1e2, 100 + nblk)
    print("system and reference: %.2f s" % (time.time() - t0))
    case = R.Case("regime%d" % nblk, "s", n, "fused")
    res = run_tool(tmp_path, {"s": (sysm.S, sysm.b)}, [case])[case.name]
    assert res["nblk"] == nblk
    assert judge(sysm, res, case.name) is None


def check_shrunk_plan(nblk, prm, ops):
    tails = [o for o in kinds(ops, PGEMM) if o["fuse_with"] >= 0]
    if nblk == 7:
        assert kinds(ops, TRSM_PIPE) and kinds(ops, UPD_PIPE, nst=16, stream=2) and kinds(ops, UPD_PIPE, nst=32, stream=2) and not kinds(ops, SINV)
        return
    g = prm[0]
    assert kinds(ops, UPD_PIPE, nst=16 * g, stream=2) and {o["dj"] for o in kinds(ops, SINV, g=g)} == {0, 1}
    if nblk == 12:
        assert len(kinds(ops, SINV)) == 8
    if nblk == 16:
        assert kinds(ops, UPD_PIPE, nst=64, stream=2)
    if prm[5] and prm[6]:        # head_small, fuse_tail
        assert len(tails) == (3 if nblk == 12 else len(tails)) and tails and kinds(ops, PGEMM, small=1) and kinds(ops, UPD_PIPE, small=1)
    else:
        assert not tails and not kinds(ops, PGEMM, small=1) and not kinds(ops, UPD_PIPE, small=1)
        assert len(kinds(ops, PGEMM, small=0)) >= 2 * len({o["kb"] for o in kinds(ops, SINV)}) - 1      # per super-step: the head rows' product and the rows' below


@pytest.mark.parametrize("nblk,prm", R.SHRUNK)
def test_the_same_kernels_at_the_smallest_shapes(tmp_path, nblk, prm):
    check_shrunk_plan(nblk, prm, plan_of(nblk, prm))
    nf, npl = R.BLOCK * nblk - 28, R.BLOCK * nblk      # fused: a ragged last block; plain: an exact multiple, the forward substitution kernel at full blocks
    systems, cases, sy = {}, [], {}
    for kind, arg in (("wishart", 1.0), ("spectrum", 1e2)):
        for mode, n in (("fused", nf), ("plain", npl)):
            name = "%s_%s" % (kind, mode)
            sy[name] = system(kind, n, arg, 200 + nblk)
            systems[name] = (sy[name].S, sy[name].b)
            cases.append(R.Case(name, name, n, mode, prm=prm))
    res = run_tool(tmp_path, systems, cases)
    bad = [e for e in (judge(sy[c.name], res[c.name], c.name) for c in cases) if e]
    assert all(res[c.name]["nblk"] == nblk for c in cases) and not bad, bad


EDGES = [1, 2, 15, 16, 17, 31, 127, 128, 129, 143, 144, 145, 255, 256, 257, 383, 384, 385]


def test_padding_edges(tmp_path):
    """n = 128 k - 1: the right-hand-side row is the last row of the last block; 128 k + 1: a last block of one live row and the
    right-hand-side row; 15 / 16 / 17 and 143 / 144 / 145 straddle the 16-wide leaf; 128 k: only the plain form exists, with the
    forward substitution as a kernel of its own"""
    systems, cases, sy = {}, [], {}
    for n in EDGES:
        name = "n%d" % n
        sy[name] = system("wishart", n, 1.0, 300 + n)
        systems[name] = (sy[name].S, sy[name].b)
        for mode in (("plain",) if n % R.BLOCK == 0 else ("plain", "row", "fused")):
            cases.append(R.Case("%s_%s" % (name, mode), name, n, mode))
    res = run_tool(tmp_path, systems, cases)
    bad = [e for e in (judge(sy[c.system], res[c.name], c.name) for c in cases) if e]
    assert not bad, bad


def test_conditioning_and_scaling(tmp_path):
    n = 700
    sy = {"kappa1e%d" % e: system("spectrum", n, 10.0 ** e, 400 + e) for e in (1, 4, 8, 10)}
    sy["graded"] = system("graded", n, 1e6, 411)
    sy["times1e12"] = system("wishart", n, 1e12, 412)
    sy["times1e-12"] = system("wishart", n, 1e-12, 413)
    cases = [R.Case("%s_%s" % (name, mode), name, n, mode) for name in sy for mode in ("fused", "plain")]
    res = run_tool(tmp_path, {k: (v.S, v.b) for k, v in sy.items()}, cases)
    bad = [e for e in (judge(sy[c.system], res[c.name], c.name) for c in cases) if e]
    assert not bad, bad


def test_same_bits_on_one_stream_and_on_three_and_with_per_step_substitution(tmp_path):
    """the unit's own claim: no operation's arithmetic depends on where it runs"""
    (n12, shrunk12), (n16, shrunk16) = R.SHRUNK[1:3]
    assert (n12, n16) == (12, 16) and shrunk12[5:] == shrunk16[5:] == (1, 1)      # (on three streams the products ride as tails, on one they are launches of their own)
    sy = {"b6": system("wishart", 700, 1.0, 500), "b12": system("wishart", 1508, 1.0, 502), "b16": system("wishart", 2020, 1.0, 501)}
    cases = []
    for name, prm in (("b6", R.SHIP), ("b12", shrunk12), ("b16", shrunk16)):
        n = sy[name].n
        cases += [R.Case(name + "_three", name, n, "fused", prm=prm), R.Case(name + "_one", name, n, "fused", safe=1, prm=prm),
                  R.Case(name + "_steps", name, n, "fused", trsv_chain=0, prm=prm), R.Case(name + "_plain_steps", name, n, "plain", trsv_chain=0, prm=prm),
                  R.Case(name + "_plain", name, n, "plain", prm=prm)]
    res = run_tool(tmp_path, {k: (v.S, v.b) for k, v in sy.items()}, cases)
    bad = [e for e in (judge(sy[c.system], res[c.name], c.name) for c in cases) if e]
    assert not bad, bad
    for name in sy:
        x = res[name + "_three"]["x"]
        assert x.tobytes() == res[name + "_one"]["x"].tobytes(), name + ": one stream and three give different bits"
        assert x.tobytes() == res[name + "_steps"]["x"].tobytes(), name + ": k_trsv_bwd per step and the one-launch chain give different bits"
        assert res[name + "_plain"]["x"].tobytes() == res[name + "_plain_steps"]["x"].tobytes(), name + ": (plain) per-step and one-launch substitution differ"


def test_the_factor_itself(tmp_path):
    """|S - F F'|_F / |S|_F <= n u with F put together from the unit's buffers (sub-diagonal tiles from L, diagonal tile k as the
    triangular inverse of Linv[k]); Linv[k] F_kk = I to 128 u kappa_inf(F_kk); and the factor of the last block as stored in S, which
    is what carries the right-hand-side row, against its inverse in the same way"""
    sy, cases = {}, []
    for n, mode in ((100, "fused"), (200, "fused"), (256, "plain"), (300, "row"), (700, "fused"), (768, "plain")):
        name = "f%d" % n
        sy[name] = system("wishart", n, 1.0, 600 + n)
        cases.append(R.Case(name, name, n, mode, dump=1))
    res = run_tool(tmp_path, {k: (v.S, v.b) for k, v in sy.items()}, cases)
    bad = [e for e in (judge(sy[c.system], res[c.name], c.name) for c in cases) if e]
    for c in cases:
        r, S, n = res[c.name], sy[c.system].S, c.n
        assert r["nblk"] <= 6
        F, tiles = R.assemble_factor(r, n)
        err = np.linalg.norm(S - F @ F.T) / np.linalg.norm(S)
        print("%-6s |S - F F'|_F / |S|_F = %.2e (n u = %.1e)" % (c.name, err, n * R.U))
        if not err <= n * R.U:
            bad.append("%s: factor residual %.3e above n u" % (c.name, err))
        last = r["nblk"] - 1
        sl = slice(last * R.BLOCK, (last + 1) * R.BLOCK)
        stored = np.tril(r["Sf"][sl, sl])
        live = n - last * R.BLOCK          # (below the live rows of the last block: the right-hand-side row under beta, then identity)
        for k, Fkk, what in [(k, t, "assembled") for k, t in enumerate(tiles)] + [(last, stored, "stored")]:
            m = live if k == last else R.BLOCK
            A, Fm = np.tril(r["Linv"][k])[:m, :m], Fkk[:m, :m]
            dev = np.abs(A @ Fm - np.eye(m)).sum(axis=1).max()
            lim = 128 * R.U * np.linalg.cond(Fm, np.inf)
            print("%-6s block %d (%s): |Linv F_kk - I|_inf = %.2e (128 u kappa_inf = %.1e)" % (c.name, k, what, dev, lim))
            if not dev <= lim:
                bad.append("%s: block %d (%s) inverse off by %.3e" % (c.name, k, what, dev))
    assert not bad, bad


def test_breakdown_is_reported_at_once_and_nothing_stays_latched(tmp_path):
    """A pivot that is not positive, or a NaN, raises flag 1 -- a defined numerical outcome.  The raised flag releases every later wait
    of that factorisation at once (a single timed-out wait would be 2 s), the schedule does not change, and the next system is
    solved as if nothing had happened."""
    n = 700
    good = system("wishart", n, 1.0, 700)
    systems, cases = {"good": (good.S, good.b)}, []
    for i in (0, 15, 16, 127, 128, 300, 640, 699):
        systems["p%d" % i] = (R.break_pivot(good.S, i), good.b)
    Sn = good.S.copy()
    Sn[350, 20] = Sn[20, 350] = np.nan
    systems["nan"] = (Sn, good.b)
    broken = [k for k in systems if k != "good"]
    for name in broken:
        cases += [R.Case(name + "_three", name, n, "fused"), R.Case(name + "_one", name, n, "fused", safe=1)]
    cases += [R.Case("good_three", "good", n, "fused"), R.Case("good_one", "good", n, "fused", safe=1)]
    res = run_tool(tmp_path, systems, cases)
    for c in cases[:-2]:
        r = res[c.name]
        print("%-12s flag %d schedule %d %.3f ms" % (c.name, r["flag"], r["schedule"], r["wall_ms"]))
    for c in cases[:-2]:
        r = res[c.name]
        assert r["flag"] == 1 and r["schedule"] == 0 and r["wall_ms"] < 2000.0, (c.name, r["flag"], r["schedule"], r["wall_ms"])
    bad = [e for e in (judge(good, res[c.name], c.name) for c in cases[-2:]) if e]
    assert not bad, bad
    assert res["good_three"]["x"].tobytes() == res["good_one"]["x"].tobytes()
