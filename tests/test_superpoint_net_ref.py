"""CPU suite of SuperPoint's convolutional network: the float64 reference tests/spnet_ref.py against
the fp32 torch transcription of the published forward (this MEASURES the figures the GPU test's tolerances are four times
of), the liveness conditions on the seeded weights, the packing of pack_state_dict, the delta-weight case and the golden
file."""
import hashlib
import os

import numpy as np
import pytest

import spnet_ref as R
from reconstructor_amd import superpoint_net as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# max |x32 - x64| / max |x64| per image of the fp32 torch transcription (F.conv2d, F.max_pool2d on the CPU) over
# spnet_ref.SHAPES, as measured and printed by test_fp32_transcription_deviation.  Per case, in the order of SHAPES
# (8 x 8, 16 x 24, 40 x 72, 8 x 264, 136 x 8, 64 x 96):
#   logits                    1.56e-7  8.02e-7  9.68e-7  5.61e-7  5.05e-7  1.01e-6
#   descriptors, normalised   1.82e-7  5.42e-7  7.85e-7  5.34e-7  5.12e-7  7.48e-7
#   descriptors, as they are  9.76e-8  5.74e-7  5.83e-7  4.87e-7  4.84e-7  8.19e-7
DEV32_LOGITS = 1.01e-6
DEV32_DESC = {True: 7.85e-7, False: 8.19e-7}          # normalised, not normalised
# what the GPU test allows: the project's factor 4 (DESIGN sections 20, 21) covers the other reduction order (tiles, cin
# slices) and the device's sqrtf and division
LOGITS_TOL = 4 * DEV32_LOGITS
DESC_TOL = {k: 4 * v for k, v in DEV32_DESC.items()}


def rel_dev(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def test_fp32_transcription_deviation():
    import torch
    worst_l, worst_d = 0.0, {True: 0.0, False: 0.0}
    for H, W in R.SHAPES:
        for norm in (True, False):
            img, lg, ds = R.case(H, W, norm)
            l32, d32 = R.forward_torch(R.weights(), img[None], norm, dtype=torch.float32)
            dl, dd = rel_dev(l32[0].numpy(), lg), rel_dev(d32[0].numpy(), ds)
            print("dev32 %3d x %3d normalise %d: logits %.3g   descriptors %.3g" % (H, W, norm, dl, dd))
            worst_l, worst_d[norm] = max(worst_l, dl), max(worst_d[norm], dd)
    print("dev32 logits %.3g (constant %.3g), descriptors %.3g / %.3g (constants %.3g / %.3g)" %
          (worst_l, DEV32_LOGITS, worst_d[True], worst_d[False], DEV32_DESC[True], DEV32_DESC[False]))
    # the constants are measurements; another BLAS or vector width may move them a little, not by a factor
    assert DEV32_LOGITS / 2 <= worst_l <= DEV32_LOGITS * 2
    for norm in (True, False):
        assert DEV32_DESC[norm] / 2 <= worst_d[norm] <= DEV32_DESC[norm] * 2


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_seeded_network_is_alive(H, W):
    """Conditions on the cases: every ReLU layer between 20 % and 80 % positive, the logits' standard deviation at least 0.1."""
    alive = {}
    lg, _ = R.forward(R.weights(), R.image(H, W), alive=alive)
    print("%d x %d: positive fractions %s, logits std %.3f" % (H, W, {k: round(v, 2) for k, v in alive.items()}, lg.std()))
    assert sorted(alive) == sorted(SP.RELU_LAYERS)
    assert all(0.2 <= v <= 0.8 for v in alive.values())
    assert lg.std() >= 0.1
    assert 0.0 <= R.image(H, W).min() and R.image(H, W).max() <= 1.0


def test_float64_statement_against_torch_float64():
    """Two independent transcriptions of the forward agree to rounding in float64 (taps, padding, pooling, the two heads)."""
    import torch
    for H, W in [(16, 24), (40, 72)]:
        for norm in (True, False):
            img, lg, ds = R.case(H, W, norm)
            l64, d64 = R.forward_torch(R.weights(), img[None], norm, dtype=torch.float64)
            assert rel_dev(l64[0].numpy(), lg) <= 1e-12 and rel_dev(d64[0].numpy(), ds) <= 1e-12


def test_pack_state_dict():
    sd = dict(R.weights())
    params = SP.pack_state_dict(sd)
    assert params.dtype == np.float32 and params.size == SP.N_PARAMS == SP.param_count() == 1300865
    assert SP.param_count() == 640 + 3 * 36928 + 73856 + 3 * 147584 + 2 * 295168 + 16705 + 65792
    hdr = open(os.path.join(ROOT, "include", "rcn.h")).read()
    assert "#define RCN_SP_N_PARAMS %d" % SP.param_count() in hdr
    names = [t[0] for t in SP.layer_table()]
    assert names == ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb"]
    at = 0
    for name, co, ci, k in SP.layer_table():
        W, b = sd[name + ".weight"], sd[name + ".bias"]
        assert W.shape == (co, ci, k, k)
        assert np.array_equal(params[at:at + W.size], W.ravel()) and np.array_equal(params[at + W.size:at + W.size + co], b)
        at += W.size + co
    assert at == params.size
    import torch
    assert np.array_equal(SP.pack_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}), params)
    bad = dict(sd)
    bad["conv3a.weight"] = sd["conv3a.weight"][:, :32]
    with pytest.raises(ValueError):
        SP.pack_state_dict(bad)
    bad = dict(sd)
    bad["convPb.bias"] = sd["convPb.bias"][:64]
    with pytest.raises(ValueError):
        SP.pack_state_dict(bad)
    with pytest.raises(KeyError):
        SP.pack_state_dict({k: v for k, v in sd.items() if k != "conv4b.bias"})
    with pytest.raises(KeyError):
        SP.pack_state_dict(dict(sd, **{"bn1a.weight": np.zeros(64, np.float32)}))


def test_prep_u8_is_the_double_division():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(SP.prep_u8(v), (v.astype(np.float64) / 255.0).astype(np.float32))
    assert (SP.prep_u8(v) != v.astype(np.float32) * np.float32(1.0 / 255.0)).any()       # not the multiplication by the rounded reciprocal


@pytest.mark.parametrize("H,W", [(40, 72), (8, 264)])
def test_delta_case_is_exact_in_float64(H, W):
    """One non-zero weight, 1, per output channel, biases 0, an image of integers over 256: the network is shifts, channel
    picks, ReLU of non-negatives and max pooling, so every value of the float64 reference is one of the image's and survives
    the cast to fp32; and the case is not trivial (about half of the outputs are non-zero; a few per cent where the image is one cell high)."""
    sd = R.delta_weights()
    for name, co, ci, k in SP.layer_table():
        Wt = sd[name + ".weight"]
        assert ((Wt != 0).reshape(co, -1).sum(axis=1) == 1).all() and set(np.unique(Wt)) == {0.0, 1.0} and not sd[name + ".bias"].any()
    img = R.delta_image(H, W)
    assert np.array_equal(img * 256, np.round(img * 256)) and img.max() < 1
    lg, ds = R.forward(sd, img, normalize=False)
    vals = set(np.unique(img).tolist()) | {0.0}
    assert set(np.unique(lg).tolist()) <= vals and set(np.unique(ds).tolist()) <= vals
    assert np.array_equal(lg.astype(np.float32).astype(np.float64), lg)
    floor = 0.25 if min(H, W) > 8 else 0.03          # one cell high: two taps in three read padding only
    assert (lg != 0).mean() > floor and (ds != 0).mean() > floor


def weights_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode() + np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def desc_subset(ds, H, W):
    """What the golden file keeps of a descriptor map [256][Hc][Wc]: all of it, but every second cell of the 40 x 72 case."""
    return ds[:, ::2, ::2] if (H, W) == (40, 72) else ds


GOLDEN = os.path.join(ROOT, "tests", "golden", "superpoint_net_small.npz")


def test_golden_file():
    assert os.path.getsize(GOLDEN) < 100 * 1024
    g = np.load(GOLDEN)
    assert str(g["weights_sha256"]) == weights_digest(R.weights()), "the seeded weights changed"
    for H, W in R.GOLDEN_SHAPES:
        img, lg, ds = R.case(H, W)
        assert np.array_equal(g["image_%d_%d" % (H, W)], img)
        assert rel_dev(lg, g["logits_%d_%d" % (H, W)]) <= 1e-12
        assert rel_dev(desc_subset(ds, H, W), g["desc_%d_%d" % (H, W)]) <= 1e-12
