"""GPU suite: how the int8 coarse kernel (csrc/coarse_i8.h) stages and addresses its ring -- ONE half-norm image per ring buffer,
brought by the wave whose turn it is (tile number modulo 8), counted waits that are the same for every wave, LDS reads as a per-tile
base plus an immediate (csrc/coarse_i8_addr.h), and a row block's opening reads issued inside the block before -- against the CPU
oracle, at the smallest grid where each of these can go wrong.

One grid of 12 images at D = 256 with 1, 2, 127, 128, 129, 640, 1153, 1400, 129, 2, 640, 1153 keypoints, all 66 pairs:
  * 1 keypoint: a train image with no tile (the staging cursor skips it); 2: one tile that is nearly all padding;
  * 127 / 128: one tile, staged by the prologue alone; 129: a second tile that is all padding but one row;
  * 640 = 5 tiles, 1153 = 10 tiles with a partly padded last one, 1400 = 11 tiles: more than eight tiles, so every wave takes the
    issuer's turn for the half-norms and the ring of four buffers wraps more than twice;
  * a query's train images go through the kernel four pairs at a time with ONE staging cursor: consecutive train images differ in
    tile count (0, 1, 2, 5, 10, 11 tiles), so the cursor crosses from pair to pair in the middle of the ring and the issuer's turn
    does not restart with a pair; queries 8 .. 10 leave groups of fewer than four pairs.
Table and counts must equal oracle.orc.match_grid exactly, and the int8 kernel must have run (coarse_dtype 2).  The shipping library
runs the 16x16x64 shape; a child process runs the same grid on the diagnostic build with RCN_COARSE_I8_S16=0, the 32x32x32 shape,
which shares the staging and the half-norm image."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KS = [1, 2, 127, 128, 129, 640, 1153, 1400, 129, 2, 640, 1153]

_CASE = []


def case_with_oracle():
    """The images, the pair list and the oracle's tables: computed once, shared, never written to."""
    if not _CASE:
        from oracle import orc
        from reconstructor_amd import synth
        from reconstructor_amd.matcher import all_pairs
        ims = [np.ascontiguousarray(im, np.float32) for im in synth.descriptor_set("superpoint", len(KS), KS, n_world=2048, seed=23)]
        assert [len(im) for im in ims] == KS
        pairs = all_pairs(len(KS))
        assert len(pairs) == 66
        exp, ec = orc.match_grid(ims, pairs, threads=8)
        assert ec.sum() > 1000, "the grid must have matches to lose"
        for a in ims + [pairs, exp, ec]:
            a.setflags(write=False)
        _CASE.append((ims, pairs, exp, ec))
    return _CASE[0]


def run_grid(m):
    ims, pairs, exp, ec = case_with_oracle()
    m.clear()
    for i, im in enumerate(ims):
        m.upload(i, im)
    out, cnt = m.match_grid(pairs, exp.shape[1])
    st = m.stats()
    m.clear()
    assert st["coarse_dtype"] == 2 and st["used_mfma_path"] == 1, st           # the int8 coarse kernel ran
    bad = np.argwhere(out != exp)
    assert len(bad) == 0, ("table differs from the oracle", len(bad), [(int(p), int(q), int(out[p, q]), int(exp[p, q])) for p, q in bad[:8]])
    assert np.array_equal(cnt, ec), "counts differ from the oracle"
    return st


@pytest.mark.gpu
def test_shared_half_norms_and_immediate_addresses_equal_the_oracle(gpu_ctx):
    from reconstructor_amd.matcher import HipL2Matcher
    run_grid(HipL2Matcher(ctx=gpu_ctx))


@pytest.mark.gpu
def test_the_32x32x32_shape_of_the_diagnostic_build_reads_the_shared_half_norms():
    diag = os.path.join(ROOT, "tools", "librcn_diag.so")
    assert os.path.exists(diag), "run __graft_entry__.build() first"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, RCN_LIB=diag, RCN_COARSE_I8_S16="0"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


if __name__ == "__main__":
    import torch  # noqa: F401  (first: one shared HIP runtime)
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    assert b"DIAGNOSTIC" in _lib.load().rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    matcher = HipL2Matcher(device=0)
    s = run_grid(matcher)
    print("coarse_dtype %d  re-ranked %d  past the re-rank %d  brute force %d" % (s["coarse_dtype"], s["rows_reranked"], s["rows_exact_fallback"], s["rows_brute_force"]), flush=True)
    matcher.ctx.close()
    print("OK")
