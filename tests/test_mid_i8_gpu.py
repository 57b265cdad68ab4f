"""GPU suite: the middle tier's sweep on the resident int8 rows (csrc/mid_i8.h, k_mid_eval_i8) and the integer threshold the re-rank
hands it (mid_thr_acc).  The shipping library sends a few rows in ten thousand through the tier; the diagnostic build can send
every row (RCN_RERANK_PASS=1: certify's verdict is ignored; RCN_FILTER_PASS=1: k_filter certifies nothing), split the grid into
pipeline chunks (RCN_CHUNK_ROWS: the deferred list) and shrink the tier's budget (RCN_MID_ROWS), and it can switch the int8 sweep
off (RCN_MID_I8=0: every row through the fp32 sweep).  The checks live in tools/mid_i8_check.py and run in child processes."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "librcn_diag.so")

SETTINGS = {
    "shipping-settings": {},
    "every-re-ranked-row": {"RCN_RERANK_PASS": "1"},
    "every-row": {"RCN_RERANK_PASS": "1", "RCN_FILTER_PASS": "1"},
    "every-row-deferred-list": {"RCN_RERANK_PASS": "1", "RCN_FILTER_PASS": "1", "RCN_CHUNK_ROWS": "4096"},
    "every-row-list-too-small": {"RCN_RERANK_PASS": "1", "RCN_FILTER_PASS": "1", "RCN_CHUNK_ROWS": "4096", "RCN_MID_ROWS": "40"},
}


def run(*args, **env):
    assert os.path.exists(DIAG), "run __graft_entry__.build() first"
    base = {k: v for k, v in os.environ.items() if k not in ("RCN_MID_I8", "RCN_RERANK_PASS", "RCN_FILTER_PASS", "RCN_CHUNK_ROWS", "RCN_MID_ROWS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mid_i8_check.py"), *args], env=dict(base, RCN_LIB=DIAG, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    print(r.stdout)
    return json.loads(r.stdout.strip().splitlines()[-2])


def check_stats(res, env, overflow=True):
    a, b = res["i8"], res["f32"]
    assert a["coarse_dtype"] == 2 and b["coarse_dtype"] == 2
    # the int8 sweep changes which kernel finds a row's candidates, not which rows reach the tier
    assert a["rows_total"] == b["rows_total"] and a["rows_reranked"] == b["rows_reranked"] and a["rows_exact_fallback"] == b["rows_exact_fallback"]
    assert a["chunks"] == b["chunks"] and (a["chunks"] > 3 if "RCN_CHUNK_ROWS" in env else a["chunks"] == 1)
    if "RCN_FILTER_PASS" in env:
        # Every row of every pair whose train image has at least two rows goes past the re-rank: k_filter passes all of them on, and the
        # re-rank does not decide.  (A train image of exactly two rows sends its rows there under the shipping settings too -- the
        # re-rank never certifies against two rows -- so the count is that of the pairs with at least TWO train rows; it contains
        # every row of the pairs with at least three.)
        assert a["rows_exact_fallback"] == res["rows_train_ge2"] >= res["rows_train_ge3"] > 0
        if overflow:      # the forty planted near-ties: more than 32 rows under a threshold, the list overflows to K2b
            assert a["rows_brute_force"] > 0 and b["rows_brute_force"] > 0
    if "RCN_MID_ROWS" in env:
        assert a["rows_brute_force"] > a["rows_exact_fallback"] // 2        # beyond the tier's budget


@pytest.mark.parametrize("name", list(SETTINGS))
def test_ragged_grid_equals_the_oracle_with_and_without_the_int8_sweep(name):
    """256-d, K = 700, 300, 1024, 64, 513, 2, 900, exact ties and 1e-4 near-ties, all pairs in both orientations and self pairs: the
    tables equal the oracle's (asserted in the child) with the int8 sweep and with RCN_MID_I8=0, table for table"""
    env = SETTINGS[name]
    check_stats(run("grid", "ragged", **env), env)


@pytest.mark.parametrize("name", ["shipping-settings", "every-row"])
def test_rows_of_200_elements(name):
    """D = 200 pads to 256: the tail chunks of every int8 row are zero on both sides of the dot product"""
    env = SETTINGS[name]
    check_stats(run("grid", "d200", **env), env, overflow=False)


@pytest.mark.parametrize("name", ["shipping-settings", "every-re-ranked-row"])
def test_a_bin_with_rows_of_both_sweeps(name):
    """a train image whose bin holds tied rows (integer threshold: k_mid_eval_i8) beside a query row with a NaN element (none:
    k_mid_eval); every row of the tier is handled by exactly one of the two kernels"""
    env = SETTINGS[name]
    res = run("grid", "mixed", **env)
    assert res["i8"]["coarse_dtype"] == 2 and res["i8"]["rows_exact_fallback"] == res["f32"]["rows_exact_fallback"] > 0


def test_the_emitted_rows_are_exactly_the_rows_under_the_integer_threshold():
    """one 1024 x 1024 pair, every row through the tier: ccount >= 2, both K1 candidates listed, and the list equals
    {t : acc <= thr_acc} of the numpy model -- integers against integers"""
    res = run("lists", RCN_RERANK_PASS="1", RCN_FILTER_PASS="1")
    assert res["rows"] == 1024 and res["own"] == 1024 and res["over"] > 0
