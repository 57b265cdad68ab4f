"""GPU suite: the middle tier's int8 sweep on v_mfma_i32_16x16x64_i8 (csrc/mid_i8.h, k_mid_eval_i8) against the oracle and against its
dot4 form, which the diagnostic build keeps behind RCN_MID_I8_MFMA=0.  The checks live in tools/mid_i8_mfma_check.py and run in child
processes on tools/librcn_diag.so; RCN_RERANK_PASS=1 sends every re-ranked row to the tier, RCN_FILTER_PASS=1 every row at all."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "librcn_diag.so")
SWITCHES = ("RCN_MID_I8", "RCN_MID_I8_MFMA", "RCN_RERANK_PASS", "RCN_FILTER_PASS", "RCN_CHUNK_ROWS", "RCN_MID_ROWS")


def run(name, **env):
    assert os.path.exists(DIAG), "run __graft_entry__.build() first"
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mid_i8_mfma_check.py"), name], env=dict(base, RCN_LIB=DIAG, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    print(r.stdout)
    return json.loads(r.stdout.strip().splitlines()[-2])


@pytest.mark.parametrize("every_row", [False, True])
def test_ragged_train_images_equal_the_oracle_and_the_dot4_sweep(every_row):
    """train images of 2, 17, 130, 512, 513 and 1100 rows (one 16-row block, a wave's share, the tile edge, padded rows), all ordered pairs
    and self pairs: the oracle's tables on both sweeps, ccount equal row for row, equal candidate sets (asserted in the child).  The forty
    duplicates of a second neighbour overflow the candidate list of the row that meets them, which K2b then resolves; query rows without an
    integer threshold share bins with rows that have one."""
    env = {"RCN_RERANK_PASS": "1"}
    if every_row:
        env["RCN_FILTER_PASS"] = "1"
    res = run("ragged", **env)
    assert res["own"] > 0 and res["rows"] > res["own"]              # rows of both sweeps in the tier
    assert res["bins_with_both_kinds"]
    assert res["over"] >= 1 and res["longest"] >= 41 and res["stats"]["rows_brute_force"] >= 1
    if every_row:
        assert res["on_threshold"] >= 1           # accumulators equal to their row's threshold were there, and were emitted (asserted in the child)
        ks = [2, 17, 130, 512, 513, 1100]       # every image is the query image of six pairs, every train image has two rows or more
        assert res["rows"] == res["stats"]["rows_exact_fallback"] == 6 * sum(ks)


def test_bins_of_1_16_17_and_33_rows_and_empty_bins():
    """a chain of pairs with every row sent to the tier: bins of exactly 1, 16, 17 and 33 rows (a part batch, one column block, one and a
    row, a batch and a row), two empty bins, a row without an integer threshold inside the bin of 33"""
    res = run("bins", RCN_RERANK_PASS="1", RCN_FILTER_PASS="1")
    assert res["bins"] == [0, 1, 16, 17, 33, 0]
    assert res["bins_with_both_kinds"] == [4] and res["own"] == 66
