"""GPU suite: the fp16 coarse pass's error bound on inputs that reach it (tests/coarse_stress.py; tests/test_coarse_stress_ref.py
shows on the CPU that the sets do what they claim).

Child processes on the diagnostic build, one at a time, run tools/mfma_error_stress.py -- the aligned, accumulation-only and
misranked sets at D = 32, 40, 64, 100, 128, 256 through `measure` (the kernel's packed candidate table against float64
accumulators) -- on the MFMA shape the library picks per D, on either shape forced at every D, and on k_coarse_w4.

The shipping library then matches the misranked and the band grids: the tables must equal the oracle's (a certificate priced from
too small a bound certifies some of these rows wrongly), no row of a band grid may be certified from coarse values (k_filter's eps
on the device is at least the formula's: the rows are undecided with eps and decided with eps / 2), and the bound the library
reports equals the Python formula."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import coarse_stress as cs  # noqa: E402

FORMS = [{"RCN_COARSE_I8": "0"}, {"RCN_COARSE_S16": "0"}, {"RCN_COARSE_S16": "1"}, {"RCN_COARSE_W4": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("switches", FORMS, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_stress_sets_stay_inside_the_bound_on_every_form_of_k1(switches, tmp_path):
    diag = os.path.join(ROOT, "tools", "librcn_diag.so")
    assert os.path.exists(diag), "run __graft_entry__.build() first"
    out = str(tmp_path / "stress.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mfma_error_stress.py"), out],
                       env=dict(os.environ, RCN_LIB=diag, **switches), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    res = json.load(open(out))
    w4 = "RCN_COARSE_W4" in switches
    dims = [D for D in cs.DIMS if not (w4 and cs.padded(D) < 64)]          # k_coarse_w4: DP >= 64 only
    for D in dims:
        a, o, m = res["aligned D=%d" % D], res["accumulation_only D=%d" % D], res["misranked D=%d" % D]
        for e in (a, o, m):
            assert e["DP"] == cs.padded(D) and e["excursion_in_eps"] <= 1.0 and e["non_candidate_shortfall_in_eps"] <= 1.0, e
            assert ("k_coarse_w4" in e["kernel_form"]) == w4, e
            if "RCN_COARSE_S16" in switches:
                assert ("16x16x32" in e["kernel_form"]) == (switches["RCN_COARSE_S16"] == "1"), e
        assert min(a["most_positive_excursion_in_eps"], -a["most_negative_excursion_in_eps"]) >= a["emulated_excursion_in_eps"] - 0.1, a
        assert a["emulated_excursion_in_eps"] >= 0.85, a
        assert o["excursion_in_eps_acc"] <= 1.0, o
        assert m["misranked_seconds_in_device_table"] >= 1, m


# ---- the shipping library ----------------------------------------------------------------------------------------------------
GRIDS = [("misranked", D, False) for D in cs.DIMS if D != 256] + [("band", D, False) for D in cs.DIMS if D != 256] + \
        [("misranked", 256, True), ("band", 256, True), ("misranked", 256, False), ("band", 256, False)]
_ORACLE = {}


def grid_with_oracle(kind, D, peaked):
    """The images, the pair list and the oracle's tables: computed once per grid, shared, never written to."""
    key = (kind, D, peaked)
    if key not in _ORACLE:
        from oracle import orc
        g = (cs.misranked if kind == "misranked" else cs.band)(D, peaked)
        pairs = np.array(g["pairs"], np.int32)
        exp, ec = orc.match_grid(g["images"], pairs, threads=4)
        for a in g["images"] + [pairs, exp, ec]:
            a.setflags(write=False)
        _ORACLE[key] = (g["images"], pairs, exp, ec)
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,D,peaked", GRIDS, ids=lambda v: str(v))
def test_tables_of_the_misranked_and_band_grids_equal_the_oracle(gpu_ctx, kind, D, peaked):
    from reconstructor_amd.matcher import HipL2Matcher
    ims, pairs, exp, ec = grid_with_oracle(kind, D, peaked)
    m = HipL2Matcher(ctx=gpu_ctx)
    m.clear()
    for i, im in enumerate(ims):
        m.upload(i, im)
    out, cnt = m.match_grid(pairs, exp.shape[1])
    st = m.stats()
    m.clear()
    bad = np.argwhere(out != exp)
    assert len(bad) == 0, (kind, D, "table differs from the oracle", len(bad), [(int(p), int(q), int(out[p, q]), int(exp[p, q])) for p, q in bad[:8]])
    assert np.array_equal(cnt, ec)
    assert st["used_mfma_path"] == 1
    if D == 256 and not peaked:
        return                                  # the int8 coarse pass (its keys are exact): only the table is asserted
    assert st["coarse_dtype"] == 1, st
    mdl = cs.model(ims, D)
    want = cs.err_bound_d2(mdl)
    assert abs(st["err_bound_d2"] - want) <= 1e-12 * want, (st["err_bound_d2"], want)
    if kind == "band":
        # every row is undecided with eps (and decided with eps / 2): none may be certified from the coarse values
        assert st["rows_total"] == sum(len(ims[a]) for a, _ in pairs) >= 32
        assert st["rows_reranked"] == st["rows_total"], st
