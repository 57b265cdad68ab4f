"""GPU suite: the exact re-rank on the whole-row gather of csrc/exact_gather.h (k_rerank_lds): a wave owns a tile of eight survivors,
requests their 24 rows whole and walks the canonical fp64 chains out of its own LDS image.  The shipping library sends about one
row in a hundred through the re-rank; the diagnostic build can send every row (RCN_FILTER_PASS=1: k_filter certifies nothing, so
every query row of every pair whose train image has at least two rows is a survivor), pass every one of those on to the middle tier
(RCN_RERANK_PASS=1: certify's verdict is ignored) and split the grid into pipeline chunks (RCN_CHUNK_ROWS: several launches, the
deferred list).  Every table is compared with the oracle's in the child process (tools/exact_gather_check.py); the row counts
asserted here prove that the kernel under test decided the rows."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "librcn_diag.so")
SWITCHES = ("RCN_MID_I8", "RCN_RERANK_PASS", "RCN_FILTER_PASS", "RCN_CHUNK_ROWS", "RCN_MID_ROWS")

EVERY_ROW = {"RCN_FILTER_PASS": "1"}
EVERY_ROW_ON = {"RCN_FILTER_PASS": "1", "RCN_RERANK_PASS": "1"}


def run(name, **env):
    assert os.path.exists(DIAG), "run __graft_entry__.build() first"
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "exact_gather_check.py"), name], env=dict(base, RCN_LIB=DIAG, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    print(r.stdout)
    return json.loads(r.stdout.strip().splitlines()[-2])


def check_counts(res, env):
    assert res["rows_train_ge2"] > 0 and res["matches"] > 0
    # k_filter passed every row of every pair with at least two train rows on: the re-rank decided them
    assert res["rows_reranked"] == res["rows_train_ge2"]
    if "RCN_RERANK_PASS" in env:
        assert res["rows_exact_fallback"] == res["rows_train_ge2"]          # ... and handed every one to the middle tier
    assert res["chunks"] > 3 if "RCN_CHUNK_ROWS" in env else res["chunks"] == 1


@pytest.mark.parametrize("env", [EVERY_ROW, EVERY_ROW_ON], ids=["every-row", "every-row-to-the-tier"])
def test_tile_edges_at_256_elements(env):
    """images of 1, 63, 64, 65, 193, 2, 3 and 130 rows on the int8 coarse path: partial tiles, tiles that span pairs, the 2-row and
    the 3-row train image, nothing from the 1-row one"""
    res = run("edges256", **env)
    assert res["coarse_dtype"] == 2
    check_counts(res, env)


@pytest.mark.parametrize("env", [EVERY_ROW, EVERY_ROW_ON], ids=["every-row", "every-row-to-the-tier"])
@pytest.mark.parametrize("D", [128, 36, 200])
def test_tile_edges_at_shorter_rows(D, env):
    """the same images at D = 128 (fp16 coarse path, half a tile row), D = 36 and D = 200: the lanes beyond D request nothing and the
    chain ends at D"""
    check_counts(run("edges%d" % D, **env), env)


def test_ties_and_near_ties():
    """exact duplicates and 1e-4 near-duplicates among the train rows: the (value, index) order of the two candidates decides, and the
    forty near-ties overflow a candidate list of the tier"""
    res = run("ragged", **EVERY_ROW_ON)
    assert res["coarse_dtype"] == 2
    check_counts(res, EVERY_ROW_ON)
    assert res["rows_brute_force"] > 0


def test_several_launches_and_the_deferred_list():
    """RCN_CHUNK_ROWS=4096: the re-rank runs once per chunk, the tier once behind the last"""
    env = dict(EVERY_ROW_ON, RCN_CHUNK_ROWS="4096")
    res = run("edges256", **env)
    assert res["coarse_dtype"] == 2
    check_counts(res, env)


def test_an_empty_list():
    """only pairs with a one-row train image: no survivor, every table entry -1"""
    res = run("empty", **EVERY_ROW_ON)
    assert res["rows_reranked"] == 0 and res["rows_train_ge2"] == 0 and res["all_minus_one"] and res["matches"] == 0


def test_shipping_settings():
    """no diagnostic switch: the rows k_filter leaves undecided, as in production"""
    res = run("edges256")
    assert res["coarse_dtype"] == 2 and res["rows_reranked"] > 0 and res["chunks"] == 1
