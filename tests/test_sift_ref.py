"""CPU tier of the SIFT stage: the restatement of tests/sift_ref.py against what is known about the
detector -- where it puts a blob, what it says of its size, what a rotation does -- plus the library's host-only layout
function, the golden file against its generator and the guard band of the golden inputs."""
import importlib.util
import math
import os

import numpy as np
import pytest

import sift_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(pyr):
    return [[np.asarray(l, dtype=np.float32) for l in layers] for layers in pyr]


def generator():
    spec = importlib.util.spec_from_file_location("make_sift_golden", os.path.join(ROOT, "tests", "golden", "make_sift_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("H,W", [(16, 16), (48, 64), (45, 67), (120, 160), (512, 384)])
@pytest.mark.parametrize("S", [3, 2])
def test_library_layout_equals_the_restatement(H, W, S):
    """rcn_sift_layout is host code: octave count, sizes (45 x 67: nearest-neighbour halving of odd sizes), sigmas, taps, offsets"""
    from reconstructor_amd import _build, sift
    _build.build()
    got, want = sift.layout(H, W, sift.options(n_octave_layers=S)), sift_ref.layout(H, W, S)
    assert got == want
    assert got["oct_h"][0] == 2 * H and got["floats_per_image"] == (S + 3) * sum(h * w for h, w in zip(got["oct_h"], got["oct_w"]))
    if (H, W, S) == (45, 67, 3):
        assert got["oct_h"] == [90, 45, 22, 11, 5] and got["oct_w"] == [134, 67, 33, 16, 8] and got["layer_taps"] == [0, 11, 13, 17, 21, 27]


def test_layout_rejects_what_the_entries_reject():
    from reconstructor_amd import _build, _lib, sift
    _build.build()
    for H, W, kw in [(15, 64, {}), (64, 15, {}), (32768, 16385, {}), (64, 64, dict(n_octave_layers=0)), (64, 64, dict(n_octave_layers=6)),
                     (64, 64, dict(sigma=0.0)), (64, 64, dict(sigma=40.0)), (64, 64, dict(edge_threshold=0.0)), (64, 64, dict(contrast_threshold=-1.0))]:
        with pytest.raises(_lib.RcnError):
            sift.layout(H, W, sift.options(**kw))


def test_nearest_halving_takes_the_even_pixels():
    """min(floor(x * (src / dst)), src - 1) with dst = src // 2: for src = 2 m + 1 that is floor(2 x + x / m) = 2 x for every x < m, so
    the index rule, written out as INTER_NEAREST states it, picks the even pixels for odd sizes as well as for even ones"""
    src = np.arange(45 * 67, dtype=np.float64).reshape(45, 67)
    assert np.array_equal(sift_ref.decimate(src, 22, 33), src[:44:2, :66:2])
    assert np.array_equal(sift_ref.decimate(src[:44, :66], 22, 33), src[:44:2, :66:2])
    assert np.array_equal(sift_ref.decimate(src[:5, :8], 2, 4), src[:4:2, :8:2])


@pytest.mark.parametrize("s,cx,cy", [(3.0, 30.3, 26.7), (2.2, 33.6, 29.15), (4.5, 31.4, 30.8)])
def test_blob_is_found_at_its_centre_with_its_size(s, cx, cy):
    """A Gaussian blob of deviation s at a non-integer centre.  Position: 0.1 px -- around (cx + 1/4, cy + 1/4): the doubled
    image samples the source at (d + 1/2) / 2 - 1/2 and the first-octave correction halves d, so every coordinate the
    detector reports carries + 1/4 (cv::SIFT without its precise-upscale option does the same).  Size: the DoG of a
    Gaussian of variance v at nominal scale t is v / (v + k^2 t^2) - v / (v + t^2), extremal at t = sqrt(v / k); in the doubled
    image v = 4 s^2 - 1 (the pyramid assumes a blur of 1 there), and the reported size is that t.  The parabola through three
    samples a third of an octave apart reproduces the extremum of this curve to better than 3 %."""
    from reconstructor_amd.synth import blob_image
    img = blob_image(64, 64, [(cx, cy, s, s, 0.0, 100.0)]).astype(np.float32)
    out = sift_ref.detect_and_compute(f32(sift_ref.pyramid(img)))
    assert out["count"] >= 1
    want = math.sqrt(4 * s * s - 1) * 2.0 ** (-1.0 / 6.0)
    best = int(np.argmax(out["response"]))
    print("blob s=%.1f: (%.3f, %.3f) size %.3f (expected %.3f), %d orientations" % (s, out["x"][best] - cx, out["y"][best] - cy, out["size"][best], want, out["count"]))
    assert (np.abs(out["x"] - (cx + 0.25)) < 0.1).all() and (np.abs(out["y"] - (cy + 0.25)) < 0.1).all()
    assert (np.abs(out["size"] / want - 1.0) < 0.03).all()
    assert (out["octave"] == out["octave"][0]).all() and len(set(out["angle"].tolist())) == out["count"]


def test_rotation_by_a_quarter_turn_keeps_the_descriptors():
    """The descriptor is taken in the keypoint's own frame, so a quarter turn of the image (the pixel grid onto itself) leaves
    its 128 elements where they are -- the known permutation is the identity -- and moves the keypoint: (x, y) -> (y, W - 1/2 - x)
    (the + 1/4 of the doubled image), angle - 90.  Exact for the doubled octave; the halving of later octaves takes even
    pixels from the left, which a rotation turns into odd ones, so those keypoints only resemble each other."""
    from reconstructor_amd.synth import blob_image
    rng = np.random.default_rng(3)
    H, W = 72, 88
    blobs = [(rng.uniform(10, W - 10), rng.uniform(10, H - 10), rng.uniform(0.9, 2.0), rng.uniform(0.9, 2.0), rng.uniform(0, 3.1),
              rng.uniform(40, 110) * rng.choice([-1, 1])) for _ in range(30)]
    img = np.rint(blob_image(H, W, blobs, texture=3.0, seed=2)).astype(np.uint8)
    a = sift_ref.detect_and_compute(f32(sift_ref.pyramid(img)))
    b = sift_ref.detect_and_compute(f32(sift_ref.pyramid(np.rot90(img))))
    fa = [i for i in range(a["count"]) if (a["octave"][i] & 255) == 255]
    fb = [j for j in range(b["count"]) if (b["octave"][j] & 255) == 255]
    assert len(fa) == len(fb) >= 10
    used = set()
    for j in fb:
        hit = [i for i in fa if i not in used and abs(float(a["y"][i]) - float(b["x"][j])) < 1e-3 and abs(W - 0.5 - float(a["x"][i]) - float(b["y"][j])) < 1e-3
               and abs((float(b["angle"][j]) - float(a["angle"][i])) % 360.0 - 270.0) < 1e-2 and a["octave"][i] == b["octave"][j]]
        assert len(hit) == 1, j
        used.add(hit[0])
        d = np.abs(a["rows"][hit[0]].astype(int) - b["rows"][j].astype(int))
        assert d.max() <= 1 and (d > 0).sum() <= 1           # row pass first on both: the two pyramids differ in the last bits of float64
    assert len(used) == len(fa)


def test_fp32_sequence_stays_within_the_derived_bound_of_the_float64_pyramid():
    """pyramid_f32 (what the GPU runs) against pyramid (float64): the bound of tests/test_sift_gpu.py, here for the emulation"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "sift_small.npz"))
    img = g["images"][0]
    p32, p64 = sift_ref.pyramid_f32(img), sift_ref.pyramid(img)
    bound = sift_ref.pyramid_bound(120, 160)
    for o in range(len(p64)):
        for i in range(len(p64[o])):
            assert p32[o][i].dtype == np.float32
            assert np.abs(p32[o][i].astype(np.float64) - p64[o][i]).max() <= bound[o][i]


def test_select_orders_dedupes_and_caps():
    mk = lambda x, y, r, ident: dict(x=np.float32(x), y=np.float32(y), size=np.float32(2), angle=np.float32(10), response=np.float32(r), octave=511, ident=ident, margin=1.0)   # noqa: E731
    kps = [mk(5, 1, 0.3, (0, 1, 2, 10, 4)), mk(2, 7, 0.1, (0, 1, 14, 4, 0)), mk(2, 3, 0.2, (0, 1, 6, 4, 1)), mk(2, 7, 0.1, (0, 1, 14, 4, 0)), mk(9, 9, 0.2, (0, 1, 18, 18, 3))]
    out, count = sift_ref.select(kps)
    assert count == 4 and [float(k["x"]) for k in out] == [2, 2, 5, 9] and [float(k["y"]) for k in out] == [3, 7, 1, 9]
    out, count = sift_ref.select(kps, K=2)
    assert count == 4 and [(float(k["x"]), float(k["y"])) for k in out] == [(2, 3), (5, 1)]      # 0.3, then the earlier of the two 0.2, in canonical order


def test_golden_file_equals_its_generator():
    gen = generator()
    g = np.load(os.path.join(ROOT, "tests", "golden", "sift_small.npz"))
    want = gen.make(int(g["seed"]))
    assert g["images"].shape == (3, 120, 160) and g["images"].dtype == np.uint8
    for k, v in want.items():
        assert g[k].dtype == v.dtype and np.array_equal(g[k], v), k
    assert g["counts"].min() > 20 and len(set(g["counts"].tolist())) == 3 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "sift_small.npz")) < 1 << 20


def test_golden_inputs_keep_the_guard_band():
    """at most 2 % of the golden keypoints (candidates that gave none included) have a decision within the guard of flipping:
    a condition on the images, not on any code under test"""
    gen = generator()
    g = np.load(os.path.join(ROOT, "tests", "golden", "sift_small.npz"))
    share = gen.band_share({k: g[k] for k in g.files})
    print("inside the guard band: %.2f %% of %d keypoints" % (100 * share, len(g["sure"])))
    assert share <= 0.02
    assert np.unpackbits(g["row_sure"], axis=1).mean() > 0.98
