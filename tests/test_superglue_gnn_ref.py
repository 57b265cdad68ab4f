"""CPU suite of SuperGlue's attentional graph network: the float64 reference tests/gnn_ref.py against
the fp32 torch transcription of the published forward (this MEASURES the two figures the GPU test's tolerances are four times
of), the BatchNorm folding, the head interleave, permutation equivariance, the integer-centre rule of the coordinates, the
packing of fold_state_dict, the conditions on the shared cases, and the golden file."""
import functools
import hashlib
import os

import numpy as np
import pytest

import gnn_ref
import sg_ref
from reconstructor_amd import superglue_gnn as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# max |mdesc_fp32 - mdesc_f64| / max |mdesc_f64| of the torch transcription over CASES, as measured and printed by
# test_fp32_transcription_deviation
DEV32_REL = 8.4e-7
REL_TOL = 4 * DEV32_REL            # what the GPU test allows: the other reduction order (tiles, online softmax), the folded BatchNorm, the device's expf
# max |logP_fp32 - logP_f64| end to end over END2END, per depth of the net (the scores, and with them the absolute error of a
# score, grow with the depth: about 25 at 2 layers, about 100 at 18)
DEV32_LOGP = {2: 2.4e-5, 18: 2.2e-4}
LOGP_TOL = {L: 4 * d for L, d in DEV32_LOGP.items()}
CASES = [(2, m, n) for m, n in gnn_ref.SHAPES + [(272, 272)]] + [(18, 33, 47), (18, 200, 257)]
END2END = [(2, 33, 47), (2, 200, 257), (18, 200, 257)]          # (a side of 47 at 18 layers has one column undecided: above 2 %)


def types_of(L):
    return [G.SELF, G.CROSS] * (L // 2)


def rel_dev(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def torch32(L, m, n):
    import torch
    inp = gnn_ref.inputs(m, n)
    return gnn_ref.forward_torch(gnn_ref.weights(L), types_of(L), *[a.copy() for a in inp[:6]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def logp_case(L, m, n):
    """float64 logP [m + 1][n + 1] of the case end to end, alpha = the seeded net's bin_score."""
    md = gnn_ref.case(m, n, L)[1]
    logP = sg_ref.assign(gnn_ref.scores(*md), alpha=float(gnn_ref.weights(L)["bin_score"]))[0]
    logP.setflags(write=False)
    return logP


def test_fp32_transcription_deviation():
    worst = 0.0
    for L, m, n in CASES:
        md = gnn_ref.case(m, n, L)[1]
        dev = max(rel_dev(a, b) for a, b in zip(torch32(L, m, n), md))
        print("dev32_rel L = %2d (%3d, %3d) = %.3g   max |mdesc| = %.1f" % (L, m, n, dev, max(np.abs(a).max() for a in md)))
        worst = max(worst, dev)
    print("dev32_rel = %.3g (constant in the tests: %.3g)" % (worst, DEV32_REL))
    # the constant is a measurement; another BLAS or vector width may move it a little, not by a factor
    assert DEV32_REL / 2 <= worst <= DEV32_REL * 2
    for L in sorted(DEV32_LOGP):
        worst = 0.0
        for l, m, n in END2END:
            if l != L:
                continue
            S32 = gnn_ref.scores(*torch32(L, m, n)).astype(np.float32)
            dev = float(np.abs(sg_ref.assign_torch32(S32, alpha=float(gnn_ref.weights(L)["bin_score"])).astype(np.float64) - logp_case(L, m, n)).max())
            print("dev32_logp L = %2d (%3d, %3d) = %.3g   scores in [%.1f, %.1f]" % (L, m, n, dev, S32.min(), S32.max()))
            worst = max(worst, dev)
        print("dev32_logp L = %2d: %.3g (constant in the tests: %.3g)" % (L, worst, DEV32_LOGP[L]))
        assert DEV32_LOGP[L] / 2 <= worst <= DEV32_LOGP[L] * 2


@pytest.mark.parametrize("m,n", [(7, 3), (33, 47), (65, 130)])
def test_folded_equals_unfolded(m, n):
    inp, md = gnn_ref.case(m, n)
    got = gnn_ref.forward_folded(G.fold_layers(gnn_ref.weights(2)), gnn_ref.TYPES2, *inp[:6])
    assert max(rel_dev(a, b) for a, b in zip(got, md)) <= 1e-12


@pytest.mark.parametrize("m,n", [(7, 3), (33, 47)])
def test_head_interleave_against_the_view(m, n):
    """Channel c is head c % 4 at depth c / 4: the numpy statement against the transcription that says view(b, 64, 4, n)."""
    import torch
    inp, md = gnn_ref.case(m, n)
    got = gnn_ref.forward_torch(gnn_ref.weights(2), gnn_ref.TYPES2, *[a.copy() for a in inp[:6]], dtype=torch.float64)
    assert max(rel_dev(a, b) for a, b in zip(got, md)) <= 1e-12
    # and the interleave matters: heads of 64 contiguous channels give something else
    q = np.random.default_rng(1).standard_normal((5, 256))
    assert np.abs(gnn_ref.attention(q, q, q) - gnn_ref.attention(q.reshape(5, 4, 64).transpose(0, 2, 1).reshape(5, 256), q, q)).max() > 1e-3


def test_permutation_equivariance():
    m, n = 33, 47
    inp, md = gnn_ref.case(m, n)
    rng = np.random.default_rng(5)
    p0, p1 = rng.permutation(m), rng.permutation(n)
    k0, s0, d0, k1, s1, d1 = inp[:6]
    got = gnn_ref.forward(gnn_ref.weights(2), gnn_ref.TYPES2, k0[p0], s0[p0], d0[p0], k1[p1], s1[p1], d1[p1])
    assert rel_dev(got[0], md[0][p0]) <= 1e-12 and rel_dev(got[1], md[1][p1]) <= 1e-12
    # swapping the images swaps the outputs
    sw = gnn_ref.forward(gnn_ref.weights(2), gnn_ref.TYPES2, k1, s1, d1, k0, s0, d0)
    assert rel_dev(sw[0], md[1]) <= 1e-12 and rel_dev(sw[1], md[0]) <= 1e-12


def test_integer_centre_rule():
    H, W = 481, 641                                   # odd: W / 2 = 320, not 320.5
    kp = np.array([[320.0, 240.0], [0.0, 0.0], [640.0, 480.0], [320.5, 240.5]], np.float32)
    k = gnn_ref.normalize(kp, (H, W))
    scale = 641 * 0.7
    assert k.dtype == np.float32 and k[0, 0] == 0 and k[0, 1] == 0
    assert np.array_equal(k, ((kp.astype(np.float64) - [320.0, 240.0]) / scale).astype(np.float32))
    assert k[3, 0] == np.float32(0.5 / scale) and k[3, 0] != 0          # the published centre (size / 2 in floating point) would give 0 here
    assert np.array_equal(gnn_ref.normalize(kp, (W, H))[:, 0], ((kp[:, 0].astype(np.float64) - 240.0) / scale).astype(np.float32))
    # the forward with shapes is the forward on the normalised coordinates
    inp = gnn_ref.inputs(7, 3)
    px0, px1 = (inp[0] * 400 + 320).astype(np.float32), (inp[3] * 300 + 200).astype(np.float32)
    sh = ((H, W), (403, 377))
    a = gnn_ref.forward(gnn_ref.weights(2), gnn_ref.TYPES2, px0, inp[1], inp[2], px1, inp[4], inp[5], shapes=sh)
    b = gnn_ref.forward(gnn_ref.weights(2), gnn_ref.TYPES2, gnn_ref.normalize(px0, sh[0]), inp[1], inp[2], gnn_ref.normalize(px1, sh[1]), inp[4], inp[5])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_fold_state_dict_packing():
    sd = dict(gnn_ref.weights(2))
    params, types, bin_score = G.fold_state_dict(sd)
    assert params.dtype == np.float32 and params.size == G.param_count(2) == 109376 + 2 * 657152 + 65792
    assert types == [G.SELF, G.CROSS] and bin_score == float(sd["bin_score"])
    assert G.fold_state_dict(sd, ["cross", "self"])[1] == [G.CROSS, G.SELF]
    # the order: the encoder's five (W, b), per layer q, k, v, merge, mlp0, mlp1, the final projection; BatchNorm folded
    layers = G.fold_layers(sd)
    assert [W.shape for W, _ in layers] == [(32, 3), (64, 32), (128, 64), (256, 128), (256, 256)] + \
        [(256, 256)] * 4 + [(512, 512), (256, 512)] + [(256, 256)] * 4 + [(512, 512), (256, 512)] + [(256, 256)]
    at = 0
    for W, b in layers:
        assert np.array_equal(params[at:at + W.size], W.astype(np.float32).ravel()) and np.array_equal(params[at + W.size:at + W.size + b.size], b.astype(np.float32))
        at += W.size + b.size
    assert at == params.size
    s = sd["kenc.encoder.1.weight"].astype(np.float64) / np.sqrt(sd["kenc.encoder.1.running_var"].astype(np.float64) + 1e-5)
    assert np.array_equal(layers[0][0], s[:, None] * sd["kenc.encoder.0.weight"][:, :, 0].astype(np.float64))
    assert np.array_equal(layers[0][1], s * (sd["kenc.encoder.0.bias"].astype(np.float64) - sd["kenc.encoder.1.running_mean"]) + sd["kenc.encoder.1.bias"])
    assert np.array_equal(layers[8][0], sd["gnn.layers.0.attn.merge.weight"][:, :, 0].astype(np.float64))     # no BatchNorm: as it came
    # torch tensors are taken as well
    import torch
    assert np.array_equal(G.fold_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})[0], params)
    # a wrong shape, a missing BatchNorm array and a wrong number of layer types are rejected
    bad = dict(sd)
    bad["gnn.layers.1.mlp.0.weight"] = sd["gnn.layers.1.mlp.0.weight"][:, :256]
    with pytest.raises(ValueError):
        G.fold_state_dict(bad)
    bad = dict(sd)
    bad["kenc.encoder.4.running_var"] = sd["kenc.encoder.4.running_var"][:10]
    with pytest.raises(ValueError):
        G.fold_state_dict(bad)
    bad = {k: v for k, v in sd.items() if k != "gnn.layers.0.mlp.1.running_mean"}
    with pytest.raises(KeyError):
        G.fold_state_dict(bad)
    with pytest.raises(ValueError):
        G.fold_state_dict(sd, [G.SELF])


def test_attention_is_not_degenerate():
    """The seeded weights give attention that is neither uniform nor one-hot, sharpening over the layers."""
    probs = []
    inp = gnn_ref.inputs(33, 47)
    gnn_ref.forward(gnn_ref.weights(18), gnn_ref.TYPES18, *inp[:6], probs=probs)
    peak = [float(P.max(axis=2).mean()) for P in probs]
    print("mean peak probability, first layers %s, last layers %s" % (np.round(peak[:4], 3), np.round(peak[-4:], 3)))
    assert 0.01 < np.mean(peak[:4]) < 0.5 and 0.15 < np.mean(peak[-4:]) < 0.9


@pytest.mark.parametrize("L,m,n", END2END)
def test_cases_meet_the_conditions(L, m, n):
    """Conditions on the cases, for the reference alone: at most 2 % of a side undecided within the tolerance, at least 90 % of
    the planted matches recovered."""
    logP = logp_case(L, m, n)
    target = gnn_ref.inputs(m, n)[6]
    rows, cols = sg_ref.undecided(logP, LOGP_TOL[L])
    sel = sg_ref.select(logP)
    planted = target >= 0
    print("L = %d (%d, %d): %d rows, %d columns undecided; %d of %d planted matches" % (L, m, n, rows.sum(), cols.sum(), (sel["table"][planted] == target[planted]).sum(), planted.sum()))
    assert rows.sum() <= 0.02 * m and cols.sum() <= 0.02 * n
    assert (sel["table"][planted] == target[planted]).sum() >= 0.9 * planted.sum()


def weights_digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode() + np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


GOLDEN = os.path.join(ROOT, "tests", "golden", "superglue_gnn_small.npz")
GOLDEN_CASES = [(1, 1), (1, 5), (7, 3)]


def test_golden_file():
    g = np.load(GOLDEN)
    assert str(g["weights_sha256"]) == weights_digest(gnn_ref.weights(2)), "the seeded weights changed"
    for m, n in GOLDEN_CASES:
        inp, md = gnn_ref.case(m, n)
        for name, a in zip(("kpts0", "scores0", "d0", "kpts1", "scores1", "d1"), inp):
            assert np.array_equal(g["%s_%d_%d" % (name, m, n)], a), name
        for side in (0, 1):
            assert rel_dev(md[side], g["mdesc%d_%d_%d" % (side, m, n)]) <= 1e-12
