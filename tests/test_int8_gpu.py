"""GPU suite: the int8 coarse pass (csrc/coarse_i8.h, k_prepare_i8, fix_scale) on the hardware.  The checks themselves live in
tools/int8_check.py and run in child processes against the diagnostic build, the only binary that returns the candidate table and
the int8 images and that knows the switches RCN_COARSE_I8 / RCN_COARSE_I8_S16."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG = os.path.join(ROOT, "tools", "librcn_diag.so")


def run(mode, **env):
    assert os.path.exists(DIAG), "run __graft_entry__.build() first"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "int8_check.py"), mode], env=dict(os.environ, RCN_LIB=DIAG, **env),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["1", "0"])
def test_int8_keys_are_exact_norms_are_upper_bounds_and_the_choice_is_right(shape):
    """Equality, not a bound: every key the kernel leaves is (exact integer accumulator << 12 | train row) of the two smallest;
    v_mfma_i32_16x16x64_i8 (shape 1, what ships) and v_mfma_i32_32x32x32_i8 (shape 0)."""
    run("keys", RCN_COARSE_I8_S16=shape)


@pytest.mark.gpu
def test_int8_grid_equals_the_oracle_and_the_fp16_path():
    a = run("grid")
    b = run("grid", RCN_COARSE_I8="0")
    assert "DTYPE 2" in a and "DTYPE 1" in b, a + b
    ha, hb = re.search(r"HASH (\w+)", a).group(1), re.search(r"HASH (\w+)", b).group(1)
    assert ha == hb, "the table with int8 forced off differs"
