"""csrc/wgprim.h on the GPU: the workgroup scan and rank primitives every compaction of the pipeline is built from."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_workgroup_primitives_one_by_one():
    """wg_scan_array, wg_scan_incl and wg_rank each against a host loop, exact integer equality (tools/wgprim_check, built by
    __graft_entry__.build()): array lengths from 0 over a ragged last run to many elements per thread, a 64-bit total past 2^31,
    256 and 1024 threads, every call twice in a row on the same LDS words."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "wgprim_check")
    assert os.path.exists(exe), "tools/wgprim_check missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
    assert "FAILED" not in r.stdout
