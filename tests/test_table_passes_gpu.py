"""GPU suite: the two passes over the dense match table, k_unique_pair (csrc/match.hip) and the compaction k_cmp_fill (csrc/store.hip),
against a numpy restatement.  The checks live in tools/table_passes_check.py and run in a child process on tools/librcn_diag.so (the
diagnostic build exports the uniqueness kernel alone).  Per K three tables: rows of whole 16-byte groups (four entries per lane and round;
the row in registers up to 4096 entries, read again above), rows of an odd length, and rows of whole groups that start off a 16-byte
boundary (both entry by entry) -- always with out_stride > K, so that the tail must become -1."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "librcn_diag.so")


def specs(K):
    vec = (K // 4 + 1) * 4                       # the next multiple of 4 above K
    odd = vec + 1
    return ["%d:%d" % (K, vec), "%d:%d" % (K, odd), "%d:%d:1" % (K, vec)]


def run(*args):
    assert os.path.exists(DIAG), "run __graft_entry__.build() first"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "table_passes_check.py"), *args], env=dict(os.environ, RCN_LIB=DIAG),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    print(r.stdout)


@pytest.mark.parametrize("K", [0, 1, 3, 255, 256, 257, 1023, 1025, 4096])
def test_uniqueness_and_compaction_equal_numpy(K):
    """several queries claiming one train row (the smallest wins), a pair without a match, a pair in which nothing changes; the lists
    ascend in the query row; counts smaller than a row's non-negative entries drop the surplus and leave the next pair's list alone"""
    run(*specs(K))


def test_the_benchmark_shape():
    """K = out_stride = 4096: no tail, the whole row in registers; and 8192 entries per row, twice what the registers hold"""
    run("4096:4096", "4096:8192", "4000:4096")
