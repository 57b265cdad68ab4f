"""GPU suite of the ORB stage (csrc/orb.hip) against tests/orb_ref.py.  Every comparison is bit for bit,
except `angle` (informative, read by no decision): two float64 atan2 results that agree to a few fp64 ulps land at most one
fp32 value apart after rounding, so 1 fp32 ulp.  Pyramid, score maps, the staged and the fused call, the golden file,
determinism, the cap, ties, the edges, a caller's pattern, argument errors, and the producer chain into the matcher at D = 32."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import orb_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("xy", "xy_int", "size", "response", "octave", "rows", "packed")
SHAPES = ((96, 128), (97, 131), (200, 264))


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "orb_small.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def image(H, W, seed=1):
    return orb_ref.corner_image(H, W, seed, n_rect=max(40, H * W // 350))


@functools.lru_cache(maxsize=None)
def reference(H, W, K, seed=1, nfeatures=500):
    return orb_ref.detect_and_compute(image(H, W, seed), K, dict(nfeatures=nfeatures))


def to_np(r):
    return {k: v.cpu().numpy() for k, v in r.items() if v is not None}


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ulp32(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126))) - 23)


def angle_within_one_ulp(got, want, m, what=""):
    """1 fp32 ulp of the reference value for the m emitted keypoints (a reference of exactly 0 admits the smallest subnormal
    only); the padding is exactly 0"""
    m = min(m, len(got))                                   # beyond the cap K nothing is emitted
    err = np.abs(got[:m].astype(np.float64) - want[:m].astype(np.float64)) / ulp32(want[:m])
    print("%s, worst angle error %.2f fp32 ulps" % (what, err.max() if m else 0.0))
    assert (err <= 1.0).all() and (got >= 0).all() and (got < 360).all(), what
    assert got[m:].tobytes() == np.zeros(len(got) - m, np.float32).tobytes() and (want[m:] == 0).all(), what


def same_as_ref(g, i, ref, what=""):
    """image i of a GPU result against the restatement's padded arrays"""
    assert int(g["counts"][i]) == ref["count"], what
    for k in EXACT:
        if k in g:
            assert g[k][i].dtype == ref[k].dtype and g[k][i].tobytes() == ref[k].tobytes(), (what, k)
    angle_within_one_ulp(g["angle"][i], ref["angle"], max(ref["count"], 0), "%s image %d: %d keypoints" % (what, i, ref["count"]))


def same_results(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in EXACT + ("angle", "counts"))


def fused(ctx, imgs, K, opt=None):
    from reconstructor_amd import orb
    return to_np(orb.detect_and_compute(ctx, imgs if hasattr(imgs, "is_cuda") else cuda(imgs), K, opt))


# ---- 1. pyramid and score maps ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_pyramid_and_fast_maps_equal_the_restatement(gpu_ctx, shape):
    from reconstructor_amd import orb
    H, W = shape
    L = orb_ref.layout(H, W)
    imgs = np.stack([image(H, W, 1), image(H, W, 2)])
    want = np.stack([orb_ref.pack(orb_ref.pyramid(im, L), L) for im in imgs])
    pyr = orb.pyramid(gpu_ctx, cuda(imgs))
    assert np.array_equal(pyr.cpu().numpy(), want)
    # a float image of equal values, and one off the integers: halves go to even, the ends are clamped
    assert np.array_equal(orb.pyramid(gpu_ctx, cuda(imgs.astype(np.float32))).cpu().numpy(), want)
    f = imgs.astype(np.float32) + np.random.default_rng(5).choice(np.array([-0.5, 0.5, 0.25, -300.0, 300.0], np.float32), size=imgs.shape)
    wantf = np.stack([orb_ref.pack(orb_ref.pyramid(im, L), L) for im in f])
    assert np.array_equal(orb.pyramid(gpu_ctx, cuda(f)).cpu().numpy(), wantf)
    got = orb.fast(gpu_ctx, pyr, H, W).cpu().numpy()
    for i in range(2):
        lv, sc = orb_ref.unpack(want[i], L), orb_ref.unpack(got[i], L)
        for l in range(L["n_levels"]):
            ws = orb_ref.fast_scores(lv[l], 20)
            assert np.array_equal(sc[l], ws), (i, l)
        assert (sc[0] > 0).sum() > 20
    assert np.array_equal(got, np.stack([orb_ref.pack([orb_ref.fast_scores(a, 20) for a in orb_ref.unpack(w, L)], L) for w in want]))


# ---- 2. staged and fused calls ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_staged_and_fused_equal_the_restatement(gpu_ctx, shape):
    from reconstructor_amd import orb
    H, W, K = shape[0], shape[1], 1024
    imgs = np.stack([image(H, W, 1), image(H, W, 2)])
    refs = [reference(H, W, K, 1), reference(H, W, K, 2)]
    dev = cuda(imgs)
    pyr = orb.pyramid(gpu_ctx, dev)
    kp = orb.detect(gpu_ctx, pyr, H, W, K)
    rows, packed = orb.describe(gpu_ctx, pyr, H, W, kp)
    staged = to_np(dict(kp, rows=rows, packed=packed))
    fu = fused(gpu_ctx, dev, K)
    for i in range(2):
        assert refs[i]["count"] > (20 if H < 200 else 200)
        same_as_ref(staged, i, refs[i], "staged %dx%d" % shape)
        same_as_ref(fu, i, refs[i], "fused %dx%d" % shape)
    assert same_results(staged, fu)


def test_golden_file(gpu_ctx):
    from reconstructor_amd import orb
    g = golden()
    opt = orb.options(nfeatures=24)
    for idx in ((0, 1), (2,)):
        r = fused(gpu_ctx, np.stack([g["image%d" % i] for i in idx]), 256, opt)
        for j, i in enumerate(idx):
            assert int(r["counts"][j]) == int(g["counts"][i]) < int(g["candidates"][i])
            for k in EXACT:
                assert r[k][j].tobytes() == g["%s%d" % (k, i)].tobytes(), (i, k)
            angle_within_one_ulp(r["angle"][j], g["angle%d" % i], int(g["counts"][i]), "golden image %d" % i)


# ---- 3. determinism -----------------------------------------------------------------------------------------------------------------

def test_determinism_pairs(gpu_ctx):
    import torch
    from reconstructor_amd import orb
    H, W, K = 97, 131, 512
    imgs = np.stack([image(H, W, s) for s in (1, 2, 3)])
    dev = cuda(imgs)
    base = fused(gpu_ctx, dev, K)
    assert same_results(base, fused(gpu_ctx, dev, K))                                      # two runs
    for i in range(3):                                                                      # batch 1 against batch n
        one = fused(gpu_ctx, dev[i:i + 1], K)
        assert all(one[k][0].tobytes() == base[k][i].tobytes() for k in EXACT + ("angle", "counts"))
    try:                                                                                    # chunk 1 against the default
        orb.set_chunk_images(gpu_ctx, 1)
        assert same_results(base, fused(gpu_ctx, dev, K))
        orb.set_chunk_images(gpu_ctx, 2)
        assert same_results(base, fused(gpu_ctx, dev, K))
    finally:
        orb.set_chunk_images(gpu_ctx, 0)
    big = torch.zeros((3, H + 5, 2 * W + 3), dtype=torch.uint8, device="cuda")             # strided against dense
    big[:, 2:2 + H, 1:1 + 2 * W:2] = dev
    assert same_results(base, fused(gpu_ctx, big[:, 2:2 + H, 1:1 + 2 * W:2], K))
    assert same_results(base, fused(gpu_ctx, dev.permute(0, 2, 1).contiguous().permute(0, 2, 1), K))
    assert same_results(base, fused(gpu_ctx, dev.to(torch.float32), K))                    # byte against float


# ---- 4. cap and ties ----------------------------------------------------------------------------------------------------------------

def test_cap_emits_the_top_k_in_canonical_order(gpu_ctx):
    H, W, K = 200, 264, 40
    ref_all, ref_cap = reference(H, W, 1024), reference(H, W, K)
    assert ref_all["count"] > 4 * K and ref_cap["count"] == ref_all["count"]
    r = fused(gpu_ctx, image(H, W)[None], K)
    same_as_ref(r, 0, ref_cap, "cap")
    # the restatement's own cap, spelled out: the K largest responses (fp64, the canonical rank breaking ties) in canonical order
    order = sorted(range(ref_all["count"]), key=lambda e: (-ref_all["response64"][e], e))[:K]
    keep = sorted(order)
    assert np.array_equal(r["xy"][0], ref_all["xy"][keep]) and np.array_equal(r["packed"][0], ref_all["packed"][keep])
    keys = list(zip(r["octave"][0].tolist(), r["xy"][0, :, 1].tolist(), r["xy"][0, :, 0].tolist()))
    assert keys == sorted(keys)


def test_tie_image_keeps_more_than_the_quota(gpu_ctx):
    from reconstructor_amd import orb
    img = np.tile(np.random.default_rng(21).integers(0, 256, (16, 16), dtype=np.uint8), (10, 10))
    ref = orb_ref.detect_and_compute(img, 4096, dict(nfeatures=40, nlevels=1))
    assert ref["count"] > 40
    r = fused(gpu_ctx, img[None], 4096, orb.options(nfeatures=40, nlevels=1))
    same_as_ref(r, 0, ref, "ties")


# ---- 5. edges -----------------------------------------------------------------------------------------------------------------------

def test_constant_image_and_empty_batch(gpu_ctx):
    import torch
    from reconstructor_amd import orb
    r = to_np(orb.detect_and_compute(gpu_ctx, torch.full((2, 96, 128), 93, dtype=torch.uint8, device="cuda"), 16))
    assert (r["counts"] == 0).all() and (r["rows"] == 0).all() and (r["packed"] == 0).all() and (r["xy"] == -1).all() and (r["xy_int"] == -1).all()
    assert (r["size"] == 0).all() and (r["angle"] == 0).all() and (r["response"] == 0).all() and (r["octave"] == 0).all()
    r = orb.detect_and_compute(gpu_ctx, torch.empty((0, 96, 128), dtype=torch.uint8, device="cuda"), 16)
    assert r["counts"].shape == (0,) and r["rows"].shape == (0, 16, 32)
    assert orb.pyramid(gpu_ctx, torch.empty((0, 96, 128), dtype=torch.float32, device="cuda")).shape[0] == 0


def smallest_legal():
    for s in range(1, 64):
        try:
            orb_ref.layout(s, s)
            return s
        except ValueError:
            pass


def test_smallest_image_and_levels_too_small(gpu_ctx):
    """the smallest square the layout admits (every level a pixel at least, none halving its predecessor) and a 62 x 90 image,
    all of whose levels lie inside the edge border: pyramids and score maps as the restatement's, no keypoints; 63 x 63 has
    one pixel inside the border at level 0"""
    from reconstructor_amd import orb
    s = smallest_legal()
    print("smallest legal square: %d" % s)
    rng = np.random.default_rng(8)
    for H, W in ((s, s), (62, 90), (63, 63)):
        img = rng.integers(0, 256, (1, H, W), dtype=np.uint8)
        L = orb_ref.layout(H, W)
        lv = orb_ref.pyramid(img[0], L)
        pyr = orb.pyramid(gpu_ctx, cuda(img))
        assert np.array_equal(pyr.cpu().numpy()[0], orb_ref.pack(lv, L))
        sc = orb.fast(gpu_ctx, pyr, H, W).cpu().numpy()[0]
        assert np.array_equal(sc, orb_ref.pack([orb_ref.fast_scores(a, 20) for a in lv], L))
        ref = orb_ref.detect_and_compute(img[0], 8)
        same_as_ref(fused(gpu_ctx, img, 8), 0, ref, "%dx%d" % (H, W))
        if (H, W) != (63, 63):
            assert ref["count"] == 0 and not any(L["active"])


def test_tile_seams_at_several_levels(gpu_ctx):
    """200 x 264: 5 x 13 tiles of 64 x 16 at level 0 and ragged last tiles at every level.  A seam in the FAST or the blur kernel
    would show as wrong scores or descriptor bits along a multiple of the tile: checked through the rows of keypoints on every
    level, and the score maps (test 1)."""
    ref = reference(200, 264, 1024)
    assert len(set(ref["level"].tolist())) >= 5
    ys, xs = ref["y"][ref["level"] == 0], ref["x"][ref["level"] == 0]
    near = ((ys % 16 < 3) | (ys % 16 > 12) | (xs % 64 < 3) | (xs % 64 > 60)).sum()
    assert near > 10                                       # keypoints whose patches straddle tile borders
    same_as_ref(fused(gpu_ctx, image(200, 264)[None], 1024), 0, ref, "seams")


# ---- 6. pattern and arguments -------------------------------------------------------------------------------------------------------

def test_caller_supplied_pattern(gpu_ctx):
    from reconstructor_amd import orb
    H, W, K = 97, 131, 256
    rng = np.random.default_rng(77)
    pat = rng.integers(-15, 16, 1024).astype(np.int8)
    pat[:8] = (15, 15, -15, -15, -15, 15, 15, -15)           # the longest reach: 21.2 pixels turned, 22 after rounding
    ref = orb_ref.detect_and_compute(image(H, W), K, None, pat)
    r = fused(gpu_ctx, image(H, W)[None], K, orb.options(pattern=pat))
    same_as_ref(r, 0, ref, "pattern")
    assert not np.array_equal(ref["packed"], reference(H, W, K)["packed"])
    same_as_ref(fused(gpu_ctx, image(H, W)[None], K, orb.options(pattern=orb_ref.default_pattern())), 0, reference(H, W, K), "default pattern passed in")


def test_other_thresholds_and_scale_factor(gpu_ctx):
    """fast_threshold 7, edge_threshold 22 (the smallest: with tests of the longest reach every read touches the level's first
    and last rows and columns at the most), scale_factor 1.5, 4 levels: k_orb_fast's threshold, the border of k_orb_nms and
    the resize tables at another factor, staged and fused against the restatement"""
    from reconstructor_amd import orb
    H, W, K = 97, 131, 1024
    pat = np.random.default_rng(78).integers(-15, 16, 1024).astype(np.int8)
    pat[:8] = (15, 15, -15, -15, -15, 15, 15, -15)
    kw = dict(fast_threshold=7, edge_threshold=22, scale_factor=1.5, nlevels=4, nfeatures=300)
    opt = orb.options(pattern=pat, **kw)
    L = orb_ref.layout(H, W, kw)
    assert L["level_h"] == orb.layout(H, W, opt)["level_h"] and sum(L["active"]) >= 2
    imgs = np.stack([image(H, W, 1), image(H, W, 4)])
    refs = [orb_ref.detect_and_compute(im, K, kw, pat) for im in imgs]
    dev = cuda(imgs)
    pyr = orb.pyramid(gpu_ctx, dev, opt)
    assert np.array_equal(pyr.cpu().numpy(), np.stack([orb_ref.pack(r["levels"], L) for r in refs]))
    sc = orb.fast(gpu_ctx, pyr, H, W, opt).cpu().numpy()
    assert np.array_equal(sc, np.stack([orb_ref.pack([orb_ref.fast_scores(a, 7) for a in r["levels"]], L) for r in refs]))
    kp = orb.detect(gpu_ctx, pyr, H, W, K, opt)
    rows, packed = orb.describe(gpu_ctx, pyr, H, W, kp, opt)
    staged = to_np(dict(kp, rows=rows, packed=packed))
    fu = fused(gpu_ctx, dev, K, opt)
    for i in range(2):
        assert refs[i]["count"] > reference(H, W, K, (1, 4)[i])["count"]              # the lower threshold and the narrower border find more
        e = 22
        on_border = ((refs[i]["x"] == e) | (refs[i]["y"] == e) | (refs[i]["x"] == np.array(L["level_w"])[refs[i]["level"]] - e - 1) |
                     (refs[i]["y"] == np.array(L["level_h"])[refs[i]["level"]] - e - 1)).sum()
        print("image %d: %d keypoints on the first or last admitted row or column" % (i, on_border))
        same_as_ref(staged, i, refs[i], "options staged")
        same_as_ref(fu, i, refs[i], "options fused")
    assert same_results(staged, fu)


def test_argument_errors(gpu_ctx):
    import torch
    from reconstructor_amd import _lib, orb
    lib, h = gpu_ctx.lib, gpu_ctx.h
    img = torch.zeros((1, 96, 128), dtype=torch.uint8, device="cuda")
    out = orb._outputs(1, 8, img.device)
    rows = torch.zeros((1, 8, 32), dtype=torch.float32, device="cuda")
    p = orb._ptr
    kp = orb._kp_ptrs(out)
    ERR = -1

    def dc(images=p(img), dtype=orb.INPUT_U8, n=1, H=96, W=128, opt=None, K=8, kp=kp, r=p(rows)):
        return lib.rcn_orb_detect_and_compute_device(h, images, dtype, 96 * 128, 128, 1, n, H, W, opt, K, *kp, r, None)
    assert dc() == 0
    assert dc(images=None) == ERR and dc(r=None) == ERR and dc(kp=[None] + kp[1:]) == ERR and dc(kp=kp[:6] + [None]) == ERR
    assert b"null pointer" in lib.rcn_last_error(h)
    assert dc(n=-1) == ERR and dc(K=0) == ERR and dc(H=0) == ERR and dc(W=1) == ERR and dc(dtype=2) == ERR
    assert b"dtype" in lib.rcn_last_error(h)
    assert dc(H=65535, W=65535) == ERR                       # H W > 2^31 - 1 (nothing is read: the check comes first)
    for kw in (dict(nlevels=0), dict(nlevels=17), dict(nfeatures=0), dict(edge_threshold=21), dict(fast_threshold=0), dict(scale_factor=1.0),
               dict(scale_factor=2.0)):
        assert dc(opt=C.byref(orb.options(**kw))) == ERR, kw
    pat = orb_ref.default_pattern()
    pat[1023] = 16
    assert dc(opt=C.byref(orb.options(pattern=pat))) == ERR
    assert b"pattern" in lib.rcn_last_error(h)
    pat[1023] = -16
    assert dc(opt=C.byref(orb.options(pattern=pat))) == ERR
    pyr = orb.pyramid(gpu_ctx, img)
    assert lib.rcn_orb_pyramid_device(h, p(img), 7, 96 * 128, 128, 1, 1, 96, 128, None, p(pyr)) == ERR
    assert lib.rcn_orb_pyramid_device(h, p(img), 1, 96 * 128, 128, 1, 1, 96, 128, None, None) == ERR
    assert lib.rcn_orb_fast_device(h, p(pyr), 1, 96, 128, None, None) == ERR
    assert lib.rcn_orb_detect_device(h, None, 1, 96, 128, None, 8, *kp) == ERR
    assert lib.rcn_orb_detect_device(h, p(pyr), 1, 96, 128, None, 0, *kp) == ERR
    assert lib.rcn_orb_describe_device(h, p(pyr), 1, 96, 128, None, 8, p(out["xy"]), p(out["octave"]), None, p(rows), None) == ERR
    assert lib.rcn_orb_describe_device(h, p(pyr), 1, 96, 128, None, 8, p(out["xy"]), p(out["octave"]), p(out["counts"]), None, None) == ERR
    assert lib.rcn_orb_set_chunk_images(None, 1) == ERR
    with pytest.raises(_lib.RcnError):
        orb.layout(0, 8)
    assert dc(n=0) == 0 and dc(n=0, images=None, r=None) == 0


# ---- 7. producer chain --------------------------------------------------------------------------------------------------------------

def test_detector_feeds_the_matcher_at_d32(gpu_ctx):
    """four overlapping crops of one scene: rows in the landing slot -> exchange(local_K = min(counts, K)) -> match at D = 32,
    equal to the oracle's lists for the same rows"""
    import torch
    from oracle import orc
    from reconstructor_amd import orb, pairgrid
    from reconstructor_amd.matcher import all_pairs
    n, H, W, K, D = 4, 128, 160, 192, 32
    scene = image(152, 192, 5)
    imgs = np.stack([scene[dy:dy + H, dx:dx + W] for dy, dx in ((0, 0), (6, 10), (12, 4), (16, 24))])
    dev = cuda(imgs)
    sh = pairgrid.Shard(gpu_ctx, 0, 1, pairgrid.unique_id())
    try:
        gpu_ctx.check(gpu_ctx.lib.rcn_desc_clear(gpu_ctx.h))
        slot = sh.reserve(n, K, D)
        r = orb.detect_and_compute(gpu_ctx, dev, K, out=slot, packed=False)
        assert r["rows"] is None and r["packed"] is None
        counts = np.minimum(r["counts"].cpu().numpy(), K)
        assert (counts > 30).all()
        again = fused(gpu_ctx, dev, K)
        rows = [np.ascontiguousarray(again["rows"][i, :counts[i]]) for i in range(n)]
        assert all(np.array_equal(x, np.rint(x)) and x.min() >= 0 and x.max() <= 255 for x in rows)
        exp, ec = orc.match_grid(rows, all_pairs(n), threads=4)
        sh.exchange(None, counts)
        P = n * (n - 1) // 2
        out = torch.empty((P, K), dtype=torch.int32, device="cuda")
        cnt = torch.empty((P,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sh.match(0.7, out.data_ptr(), K, cnt.data_ptr())
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        got = out.cpu().numpy()
        assert np.array_equal(cnt.cpu().numpy(), ec) and ec.sum() > 10
        for q, (i, j) in enumerate(all_pairs(n)):
            assert np.array_equal(got[q, :counts[i]], exp[q, :counts[i]]), q
    finally:
        sh.close()
