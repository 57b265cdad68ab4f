"""GPU suite: the batched top-2 fold of the coarse kernels (csrc/top2_fold.h in k_coarse_top2 / k_coarse_top2_i8) against the CPU
oracle, at the smallest shapes where taking a column block's keys four at a time can go wrong.

Grid: 6 images of 300 / 333 / 512 / 333 / 300 / 512 keypoints, all 15 pairs -- the first three images are the 3-image grid, image 0
is the query of five pairs (a group of four and a group of one), 300 and 333 leave padded rows and a partial last tile, 512 fills a
query tile and spans several train tiles at both tile sizes (64, 128).

Planted rows: for chosen queries of image j - 1, two rows of image j are near-copies of the query, the best at distance d and the
second at 1.2 d (ratio test fails: the expected entry is -1, and it turns into a match as soon as EITHER of the two is lost, every
other row being far away), in some cases with a third row at 1.1 d; and pairs at d / 2 d (the ratio test passes: the entry is the
best row).  Best and second are placed by train row so that they fall into one pair of a batch (rows 4k, 4k + 1), two pairs of one
batch (4k + 1, 4k + 2), the two 16-row halves of a 32-row block, adjacent row blocks, the last row block of a tile and the first of
the next (tiles of 64 and of 128 rows), the last row block of the image (the drain), and rows 0 and K - 1; each in both orders.

The tables must equal the oracle's and no row may reach the brute-force kernel: the certificates are priced from the candidate
values, so a wrong second candidate is either a wrong table or rows leaving the coarse path.  The shipping library runs D = 256 on
int8, D = 256 on fp16 (one peaked row makes fix_scale refuse int8), D = 128 and D = 32; child processes run the same grids on the
diagnostic build for the other MFMA shape of every kernel and for the two folds kept there for timing (RCN_COARSE_ABL = 16 / 32)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KS = [300, 333, 512, 333, 300, 512]
CONFIGS = {          # name: (descriptor kind, distance of the best planted row, expected coarse_dtype)
    "d256_int8": ("superpoint", 0.15, 2),
    "d256_fp16": ("superpoint", 0.15, 1),
    "d128": ("sift", 16.0, 1),
    "d32": ("orb", 12.0, 1),
}


def placements(K, j):
    """(best row, second row, third row or None, second's distance / best's) for a train image of K rows (image j of the grid)."""
    L0 = 32 * ((K - 1) // 32)                       # first row of the image's last 32-row block
    P = [
        (40, 41, None, 1.2), (45, 44, None, 1.2),               # one pair of a batch
        (49, 50, None, 1.2), (54, 53, None, 1.2),               # two pairs of one batch
        (56, 57, 58, 1.2), (61, 60, 62, 1.2),                   # ... with a third row: the whole quad
        (73, 74, 75, 1.2), (78, 77, 76, 1.2),
        (3, 19, None, 1.2), (21, 5, None, 1.2),                 # the two 16-row halves of a 32-row block
        (10, 43, None, 1.2), (47, 12, None, 1.2),               # adjacent row blocks
        (63, 64, None, 1.2), (70, 35, None, 1.2),               # last row block of a 64-row tile, first of the next
        (127, 128, None, 1.2), (140, 101, None, 1.2),           # ... of a 128-row tile
        (L0 + 1, L0 + 6, None, 1.2), (L0 + 10, L0 + 2, None, 1.2),      # both in the image's last row block: the drain
        (L0 - 7, L0 + 3, None, 1.2), (L0 + 8, L0 - 12, None, 1.2),      # the block before it and the drain
        (88, 89, None, 2.0), (93, 92, None, 2.0),               # the ratio test passes: the best row is the match
        (110, 150, None, 2.0), (152, 112, None, 2.0),
    ]
    P.append((0, K - 1, None, 1.2) if j in (1, 4, 5) else (K - 1, 0, None, 1.2))     # rows 0 and K - 1 (333 and 512 get both orders)
    rows = [r for p in P for r in p[:3] if r is not None]
    assert len(set(rows)) == len(rows) and min(rows) >= 0 and max(rows) < K, (K, sorted(rows))
    return P


def near_copy(q, dist, kind, rng):
    """q moved by about `dist` in the kind's format (integer-valued and non-negative for SIFT / ORB)."""
    n = rng.standard_normal(q.shape)
    if kind == "superpoint":
        return (q + dist * n / np.linalg.norm(n)).astype(np.float32)
    n = np.abs(n) * np.where(q > 200, -1.0, 1.0)                # stay inside 0..255
    return np.rint(q + dist * n / np.linalg.norm(n)).clip(0, 255).astype(np.float32)


def make_case(name):
    from reconstructor_amd import synth
    kind, delta, _ = CONFIGS[name]
    ims = synth.descriptor_set(kind, len(KS), KS, n_world=2048, seed=17)
    rng = np.random.default_rng(5)
    planted = [set() for _ in KS]
    expect = []                                                 # (query image, query row, train image, expected entry)
    for j in range(1, len(KS)):
        free = [r for r in range(KS[j - 1]) if r not in planted[j - 1]]
        P = placements(KS[j], j)
        queries = free[2::len(free) // len(P)][:len(P)]
        assert len(queries) == len(P)
        for qrow, (rb, rs, rt, far) in zip(queries, P):
            q = ims[j - 1][qrow]
            ims[j][rb] = near_copy(q, delta, kind, rng)
            ims[j][rs] = near_copy(q, far * delta, kind, rng)
            if rt is not None:
                ims[j][rt] = near_copy(q, 1.1 * delta, kind, rng)
            planted[j].update(r for r in (rb, rs, rt) if r is not None)
            # the construction itself: best < (third <) second, all three far below every other row, ratio test as intended
            d = np.sqrt(((ims[j].astype(np.float64) - q.astype(np.float64)) ** 2).sum(1))
            order = np.argsort(d, kind="stable")
            want = [rb, rs] if rt is None else [rb, rt, rs]
            assert list(order[:len(want)]) == want, (name, j, qrow, order[:4], d[order[:4]])
            assert d[order[len(want)]] > 1.5 * d[rs], (name, j, qrow, d[order[:4]])
            assert (d[order[0]] < 0.7 * d[order[1]]) == (far == 2.0), (name, j, qrow, d[order[:3]])
            expect.append((j - 1, qrow, j, rb if far == 2.0 else -1))
    if name == "d256_fp16":                                     # one peaked row: max |x| sqrt(D) / Nmax = 14.4, int8 is refused
        x = ims[5][7].copy()
        assert 7 not in planted[5]
        x[17] = 0.0
        x *= np.sqrt(1.0 - 0.81) / np.linalg.norm(x)
        x[17] = 0.9
        ims[5][7] = x
    return [np.ascontiguousarray(im, np.float32) for im in ims], expect


_ORACLE = {}


def case_with_oracle(name):
    """The images, the pair list and the oracle's tables: computed once per configuration, shared, never written to."""
    if name not in _ORACLE:
        from oracle import orc
        from reconstructor_amd.matcher import all_pairs
        ims, expect = make_case(name)
        pairs = all_pairs(len(KS))
        exp, ec = orc.match_grid(ims, pairs, threads=8)
        for qi, qrow, ti, want in expect:                       # the planted rows decide their entries, as intended (uniqueness aside)
            p = int(np.nonzero((pairs[:, 0] == qi) & (pairs[:, 1] == ti))[0][0])
            assert exp[p, qrow] in (want, -1), (name, qi, qrow, ti, want, exp[p, qrow])
        for a in ims + [pairs, exp, ec]:
            a.setflags(write=False)
        _ORACLE[name] = (ims, pairs, exp, ec)
    return _ORACLE[name]


def run_config(m, name, dtype=None):
    ims, pairs, exp, ec = case_with_oracle(name)
    m.clear()
    for i, im in enumerate(ims):
        m.upload(i, im)
    out, cnt = m.match_grid(pairs, exp.shape[1])
    st = m.stats()
    m.clear()
    assert st["coarse_dtype"] == (dtype or CONFIGS[name][2]) and st["used_mfma_path"] == 1, (name, st)
    bad = np.argwhere(out != exp)
    assert len(bad) == 0, (name, "table differs from the oracle", len(bad), [(int(p), int(q), int(out[p, q]), int(exp[p, q])) for p, q in bad[:8]])
    assert np.array_equal(cnt, ec), (name, "counts differ from the oracle")
    assert st["rows_brute_force"] == 0, (name, st)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_batched_fold_keeps_the_exact_second_neighbour(gpu_ctx, name):
    from reconstructor_amd.matcher import HipL2Matcher
    run_config(HipL2Matcher(ctx=gpu_ctx), name)


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [
    {"RCN_COARSE_S16": "0"},                                  # the fp16 kernel on 32x32 MFMAs at every D (consecutive registers of a column block)
    {"RCN_COARSE_S16": "1"},                                  # ... on 16x16 MFMAs at every D (one register quad); either switch keeps int8 off
    {"RCN_COARSE_I8_S16": "0"},                               # the int8 kernel on 32x32 MFMAs
    {"RCN_COARSE_ABL": "16"},                                 # diagnostic build: the fold key by key, kept for timing, results correct
    {"RCN_COARSE_ABL": "32"},                                 # ... the batched fold in the placement the shipping kernel does not use
], ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_other_shapes_and_the_timing_folds_of_the_diagnostic_build(switches):
    diag = os.path.join(ROOT, "tools", "librcn_diag.so")
    assert os.path.exists(diag), "run __graft_entry__.build() first"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, RCN_LIB=diag, **switches),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


if __name__ == "__main__":
    import torch  # noqa: F401  (first: one shared HIP runtime)
    from reconstructor_amd import _lib
    from reconstructor_amd.matcher import HipL2Matcher
    assert b"DIAGNOSTIC" in _lib.load().rcn_version(), "run with RCN_LIB=tools/librcn_diag.so"
    matcher = HipL2Matcher(device=0)
    for cfg in CONFIGS:
        s = run_config(matcher, cfg, 1 if "RCN_COARSE_S16" in os.environ else None)      # a forced fp16 shape takes D = 256 off int8
        print("%-10s coarse_dtype %d  re-ranked %d  past the re-rank %d  brute force %d" % (cfg, s["coarse_dtype"], s["rows_reranked"], s["rows_exact_fallback"], s["rows_brute_force"]), flush=True)
    matcher.ctx.close()
    print("OK")
