"""GPU suite of SuperGlue's attentional graph network (csrc/superglue_gnn.hip) against tests/gnn_ref.py.

Tolerance: per pair |mdesc - mdesc_f64| <= REL_TOL x max |mdesc_f64| with REL_TOL = 4 x DEV32_REL, DEV32_REL being what the
fp32 torch transcription of the published forward deviates on the same cases (measured and printed by
tests/test_superglue_gnn_ref.py); the factor 4 allows for the other reduction order (tiles, online softmax), the folded
BatchNorm and the device's expf.  End to end, logP within 4 x DEV32_LOGP of the float64 statement and the selection equal on
the rows and columns that cannot turn within that.  The figures are printed; measured on an MI355X: mdesc
within 1.02e-6 relative over all cases (allowed 3.36e-6), logP within 4.1e-5 at two layers (allowed 9.6e-5) and 2.4e-4 at 18
(allowed 8.8e-4), 120 of 120 planted matches.  Two layers (self, cross) except where stated."""
import ctypes as C
import functools

import numpy as np
import pytest

import gnn_ref
import sg_ref
from test_superglue_gnn_ref import LOGP_TOL, REL_TOL, logp_case

pytestmark = pytest.mark.gpu

ERR_ARG, UNSUPPORTED = -1, -4
CAP = 272


def G():
    from reconstructor_amd import superglue_gnn
    return superglue_gnn


@pytest.fixture(scope="module")
def nets(gpu_ctx):
    """name -> Net on the session's ctx; made on first use, closed with the module."""
    made = {}

    def get(name):
        if name not in made:
            L, types = {"2": (2, None), "18": (18, None), "self": (2, [0, 0]), "cross": (2, [1, 1]), "0": (0, None)}[name]
            made[name] = G().Net.from_state_dict(gpu_ctx, gnn_ref.weights(L), types)
        return made[name]
    yield get
    for n in made.values():
        n.close()


def pack(pairs, M, N, channel_first=False, pad=np.nan):
    """The inputs of `pairs` (tuples as gnn_ref.inputs returns) in one batch of capacity M x N, padding filled with `pad`;
    CUDA tensors (kpts0, scores0, d0, kpts1, scores1, d1), counts m, n."""
    import torch
    B = len(pairs)
    k0, s0, d0 = np.full((B, M, 2), pad, np.float32), np.full((B, M), pad, np.float32), np.full((B, M, 256), pad, np.float32)
    k1, s1, d1 = np.full((B, N, 2), pad, np.float32), np.full((B, N), pad, np.float32), np.full((B, N, 256), pad, np.float32)
    for b, p in enumerate(pairs):
        m, n = len(p[1]), len(p[4])
        k0[b, :m], s0[b, :m], d0[b, :m], k1[b, :n], s1[b, :n], d1[b, :n] = p[:6]
    t = [torch.from_numpy(a).cuda() for a in (k0, s0, d0, k1, s1, d1)]
    if channel_first:
        t[2], t[5] = t[2].permute(0, 2, 1).contiguous(), t[5].permute(0, 2, 1).contiguous()
    cnt = lambda i: torch.tensor([len(p[i]) for p in pairs], dtype=torch.int32).cuda()
    return t, cnt(1), cnt(4)


def forward(ctx, net, pairs, M=None, N=None, channel_first=False, sentinel=None, **kw):
    """mdesc0 [B][M][256], mdesc1 [B][N][256] as numpy."""
    import torch
    M = M or max(len(p[1]) for p in pairs)
    N = N or max(len(p[4]) for p in pairs)
    t, m, n = pack(pairs, M, N, channel_first)
    out = None
    if sentinel is not None:
        out = (torch.full((len(pairs), M, 256), sentinel, dtype=torch.float32).cuda(), torch.full((len(pairs), N, 256), sentinel, dtype=torch.float32).cuda())
    a, b = G().forward(ctx, net, *t, m=m, n=n, channel_first=channel_first, out=out, **kw)
    return a.cpu().numpy(), b.cpu().numpy()


def check_mdesc(got, want, tag):
    dev = [float(np.abs(g.astype(np.float64) - w).max() / np.abs(w).max()) for g, w in zip(got, want)]
    print("%s: max |mdesc - f64| / max |f64| = %.3g, %.3g (allowed %.3g)" % (tag, dev[0], dev[1], REL_TOL))
    assert max(dev) <= REL_TOL


@pytest.mark.parametrize("channel_first", [False, True], ids=["rows", "channel_first"])
@pytest.mark.parametrize("m,n", gnn_ref.SHAPES)
def test_mdesc(gpu_ctx, nets, m, n, channel_first):
    inp, md = gnn_ref.case(m, n)
    a, b = forward(gpu_ctx, nets("2"), [inp], channel_first=channel_first)
    check_mdesc((a[0], b[0]), md, "(%d, %d)" % (m, n))
    a2, b2 = forward(gpu_ctx, nets("2"), [inp], channel_first=channel_first)             # run to run
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()


def test_both_layouts_give_the_same_bits(gpu_ctx, nets):
    inp = gnn_ref.inputs(65, 130)
    a = forward(gpu_ctx, nets("2"), [inp])
    b = forward(gpu_ctx, nets("2"), [inp], channel_first=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def check_selection(r, b, m, n, logP, tol, target, tag):
    """Pair b of a match result against the float64 logP [m + 1][n + 1] (as test_superglue_gpu.check_pair, at this tolerance)."""
    M, N = r["matches0"].shape[1], r["matches1"].shape[1]
    got = r["logP"][b].astype(np.float64)
    inner = np.abs(got[:m, :n] - logP[:m, :n]).max()
    dust = max(np.abs(got[:m, N] - logP[:m, n]).max(), np.abs(got[M, :n] - logP[m, :n]).max(), abs(got[M, N] - logP[m, n]))
    print("%s (%d, %d): max |logP - f64| = %.3g inner, %.3g dustbins (allowed %.3g)" % (tag, m, n, inner, dust, tol))
    assert inner <= tol and dust <= tol
    sel = sg_ref.select(logP)
    rows, cols = sg_ref.undecided(logP, tol)
    assert rows.sum() <= 0.02 * m and cols.sum() <= 0.02 * n
    assert np.abs(r["mscores0"][b, :m] - sel["mscores0"])[~rows].max(initial=0) <= tol
    assert np.abs(r["mscores1"][b, :n] - sel["mscores1"])[~cols].max(initial=0) <= tol
    assert np.array_equal(r["matches0"][b, :m][~rows], sel["matches0"][~rows])
    assert np.array_equal(r["matches1"][b, :n][~cols], sel["matches1"][~cols])
    assert np.array_equal(r["table"][b, :m][~rows], sel["table"][~rows])
    assert r["counts"][b] == (r["table"][b] >= 0).sum() and r["status"][b] == 0
    assert (r["matches0"][b, m:] == -1).all() and (r["matches1"][b, n:] == -1).all() and (r["table"][b, m:] == -1).all()
    planted = target >= 0
    hit = (r["table"][b, :m][planted] == target[planted]).sum()
    print("%s: %d of %d planted matches" % (tag, hit, planted.sum()))
    assert hit >= 0.9 * planted.sum()


def match(ctx, net, pairs, M=None, N=None, want_logp=True):
    M = M or max(len(p[1]) for p in pairs)
    N = N or max(len(p[4]) for p in pairs)
    t, m, n = pack(pairs, M, N)
    r = G().match(ctx, net, *t, m=m, n=n, want_logp=want_logp)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in r.items()}


@pytest.mark.parametrize("m,n", [(33, 47), (200, 257)])
def test_end_to_end_two_layers(gpu_ctx, nets, m, n):
    inp = gnn_ref.inputs(m, n)
    check_selection(match(gpu_ctx, nets("2"), [inp]), 0, m, n, logp_case(2, m, n), LOGP_TOL[2], inp[6], "L = 2")


def test_eighteen_layers(gpu_ctx, nets):
    m, n = 200, 257
    inp, md = gnn_ref.case(m, n, 18)
    a, b = forward(gpu_ctx, nets("18"), [inp])
    check_mdesc((a[0], b[0]), md, "L = 18 (%d, %d)" % (m, n))
    check_selection(match(gpu_ctx, nets("18"), [inp]), 0, m, n, logp_case(18, m, n), LOGP_TOL[18], inp[6], "L = 18")


@functools.lru_cache(maxsize=None)
def ragged_pairs():
    return tuple(gnn_ref.inputs(m, n) if m and n else tuple(a[:k] for a, k in zip(gnn_ref.inputs(max(m, 1), max(n, 1))[:6], (m, m, m, n, n, n)))
                 for m, n in gnn_ref.RAGGED)


def test_ragged_batch(gpu_ctx, nets):
    """NaN in all padding, sentinel-filled outputs: padding and the empty pair untouched, every pair bit-equal to itself alone
    and to the batch at one pair per chunk."""
    pairs, net, SENT = list(ragged_pairs()), nets("2"), -7.0
    a, b = forward(gpu_ctx, net, pairs, CAP, CAP, sentinel=SENT)
    try:
        G().set_chunk_pairs(gpu_ctx, 1)
        a1, b1 = forward(gpu_ctx, net, pairs, CAP, CAP, sentinel=SENT)
        G().set_chunk_pairs(gpu_ctx, 3)
        a3, b3 = forward(gpu_ctx, net, pairs, CAP, CAP, sentinel=SENT)
    finally:
        G().set_chunk_pairs(gpu_ctx, 0)
    assert a.tobytes() == a1.tobytes() == a3.tobytes() and b.tobytes() == b1.tobytes() == b3.tobytes()
    for i, (m, n) in enumerate(gnn_ref.RAGGED):
        if m == 0 or n == 0:
            assert (a[i] == SENT).all() and (b[i] == SENT).all()
            continue
        assert (a[i, m:] == SENT).all() and (b[i, n:] == SENT).all()
        check_mdesc((a[i, :m], b[i, :n]), gnn_ref.case(m, n)[1], "batch (%d, %d)" % (m, n))
        alone = forward(gpu_ctx, net, [pairs[i]])
        assert alone[0][0].tobytes() == a[i, :m].tobytes() and alone[1][0].tobytes() == b[i, :n].tobytes()


def test_swapping_the_images_swaps_the_outputs(gpu_ctx, nets):
    for m, n in [(65, 130), (5, 300)]:
        p = gnn_ref.inputs(m, n)
        a = forward(gpu_ctx, nets("2"), [p])
        b = forward(gpu_ctx, nets("2"), [p[3:6] + p[:3]])
        assert a[0].tobytes() == b[1].tobytes() and a[1].tobytes() == b[0].tobytes()


@pytest.mark.parametrize("name,L,types", [("self", 2, [0, 0]), ("cross", 2, [1, 1]), ("0", 0, [])], ids=["all_self", "all_cross", "no_layer"])
def test_layer_lists(gpu_ctx, nets, name, L, types):
    inp = gnn_ref.inputs(33, 47)
    want = gnn_ref.forward(gnn_ref.weights(L), types, *inp[:6])
    a, b = forward(gpu_ctx, nets(name), [inp])
    check_mdesc((a[0], b[0]), want, name)


def test_match_equals_forward_then_match(gpu_ctx, nets):
    from reconstructor_amd import superglue
    pairs, net = list(ragged_pairs()), nets("2")
    t, m, n = pack(pairs, CAP, CAP)
    one = G().match(gpu_ctx, net, *t, m=m, n=n, want_logp=True, table_stride=CAP + 3)
    md0, md1 = G().forward(gpu_ctx, net, *t, m=m, n=n)
    two = superglue.match(gpu_ctx, md0, md1, m, n, superglue.options(gpu_ctx, alpha=net.bin_score), want_logp=True, table_stride=CAP + 3)
    for k in one:
        assert one[k].cpu().numpy().tobytes() == two[k].cpu().numpy().tobytes(), k
    assert one["counts"].cpu().numpy()[1] == 0 and one["counts"].cpu().numpy()[0] > 100


def test_image_shapes_equal_prenormalised_input(gpu_ctx, nets):
    import torch
    inp = gnn_ref.inputs(65, 130)
    shapes = ((481, 641), (403, 377))                     # odd sizes: the centre is W / 2 in integers
    px0, px1 = (inp[0] * 400 + 320).astype(np.float32), (inp[3] * 300 + 200).astype(np.float32)
    pixel = (px0, inp[1], inp[2], px1, inp[4], inp[5])
    normed = (gnn_ref.normalize(px0, shapes[0]), inp[1], inp[2], gnn_ref.normalize(px1, shapes[1]), inp[4], inp[5])
    sh = [torch.tensor([s], dtype=torch.int32).cuda() for s in shapes]
    a = forward(gpu_ctx, nets("2"), [pixel], shapes0=sh[0], shapes1=sh[1])
    b = forward(gpu_ctx, nets("2"), [normed])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    check_mdesc((a[0][0], a[1][0]), gnn_ref.forward(gnn_ref.weights(2), gnn_ref.TYPES2, *pixel, shapes=shapes), "with shapes")


def test_non_finite_input_propagates(gpu_ctx, nets):
    inp = [a.copy() for a in gnn_ref.inputs(33, 47)[:6]]
    inp[2][5, 17] = np.nan
    r = match(gpu_ctx, nets("2"), [tuple(inp)], want_logp=False)
    assert r["status"][0] == 1 and (r["matches0"][0] == -1).all() and r["counts"][0] == 0


def test_argument_errors(gpu_ctx, nets):
    import torch
    from reconstructor_amd import _lib
    lib, h, net = gpu_ctx.lib, gpu_ctx.h, nets("2")
    params, types, bin_score = G().fold_state_dict(gnn_ref.weights(2))
    ty = np.array(types, np.int32)
    out = C.c_void_p()
    create = lambda types_p, L, p, n, bs, o=C.byref(out): lib.rcn_sg_net_create(h, types_p, L, p, n, bs, o)
    assert create(ty.ctypes.data, 2, params.ctypes.data, params.size - 1, 1.0) == ERR_ARG
    assert "parameters" in lib.rcn_last_error(h).decode()
    assert create(ty.ctypes.data, 1, params.ctypes.data, params.size, 1.0) == ERR_ARG
    assert create(ty.ctypes.data, -1, params.ctypes.data, params.size, 1.0) == ERR_ARG
    assert create(None, 2, params.ctypes.data, params.size, 1.0) == ERR_ARG
    assert create(ty.ctypes.data, 2, None, params.size, 1.0) == ERR_ARG
    assert create(np.array([0, 2], np.int32).ctypes.data, 2, params.ctypes.data, params.size, 1.0) == ERR_ARG
    assert create(ty.ctypes.data, 2, params.ctypes.data, params.size, float("nan")) == ERR_ARG
    assert create(ty.ctypes.data, 2, params.ctypes.data, params.size, 1.0, None) == ERR_ARG
    assert lib.rcn_sg_net_create(None, ty.ctypes.data, 2, params.ctypes.data, params.size, 1.0, C.byref(out)) == ERR_ARG
    assert out.value is None
    lib.rcn_sg_net_destroy(None)
    assert lib.rcn_sg_net_set_chunk_pairs(None, 1) == ERR_ARG

    B, M, N = 2, 8, 9
    f = lambda *s: torch.zeros(s, dtype=torch.float32).cuda()
    k0, s0, d0, k1, s1, d1, o0, o1 = f(B, M, 2), f(B, M), f(B, M, 256), f(B, N, 2), f(B, N), f(B, N, 256), f(B, M, 256), f(B, N, 256)
    shp = torch.full((B, 2), 480, dtype=torch.int32).cuda()
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(ctx=h, net_h=net.h, k0=k0, s0=s0, d0=d0, k1=k1, s1=s1, d1=d1, sh0=None, sh1=None, B=B, M=M, N=N, D=256, o0=o0, o1=o1):
        return lib.rcn_sg_net_forward_device(ctx, net_h, p(k0), p(s0), p(d0), M * 256, 256, 1, p(k1), p(s1), p(d1), N * 256, 256, 1, p(sh0), p(sh1), None, None,
                                             B, M, N, D, p(o0), p(o1))
    assert fwd() == 0 and fwd(sh0=shp, sh1=shp) == 0 and fwd(B=0) == 0
    assert fwd(ctx=None) == ERR_ARG and fwd(net_h=None) == ERR_ARG
    for name in ("k0", "s0", "d0", "k1", "s1", "d1", "o0", "o1"):
        assert fwd(**{name: None}) == ERR_ARG, name
    assert fwd(sh0=shp) == ERR_ARG and fwd(sh1=shp) == ERR_ARG
    assert fwd(B=-1) == ERR_ARG and fwd(M=0) == ERR_ARG and fwd(N=0) == ERR_ARG
    assert fwd(D=128) == UNSUPPORTED and fwd(D=512) == UNSUPPORTED
    assert "RCN_" not in lib.rcn_last_error(h).decode()
    assert fwd(M=4097) == UNSUPPORTED and fwd(N=4097) == UNSUPPORTED
    with _lib.Context(0) as other:                      # a net belongs to its ctx
        assert fwd(ctx=other.h) == ERR_ARG

    i32 = lambda *s: torch.zeros(s, dtype=torch.int32).cuda()
    m0, tab, cnt = i32(B, M), i32(B, M), i32(B)

    def mat(net_h=net.h, D=256, opt=None, m0=m0, tab=tab, stride=M, cnt=cnt, d0=d0, B=B):
        return lib.rcn_sg_net_match_device(h, net_h, p(k0), p(s0), p(d0), M * 256, 256, 1, p(k1), p(s1), p(d1), N * 256, 256, 1, None, None, None, None,
                                           B, M, N, D, opt, p(m0), None, None, None, p(tab), stride, p(cnt), None, None)
    assert mat() == 0 and mat(B=0) == 0
    assert mat(net_h=None) == ERR_ARG and mat(d0=None) == ERR_ARG and mat(m0=None) == ERR_ARG
    assert mat(stride=M - 1) == ERR_ARG and mat(cnt=None) == ERR_ARG and mat(D=64) == UNSUPPORTED
    from reconstructor_amd import superglue
    assert mat(opt=C.byref(superglue.options(gpu_ctx, iterations=-1))) == ERR_ARG
    assert mat(opt=C.byref(superglue.options(gpu_ctx, match_threshold=1.5))) == ERR_ARG
    assert mat(opt=C.byref(superglue.options(gpu_ctx, alpha=float("nan")))) == 0          # alpha is the net's bin_score: the option is ignored
    gpu_ctx.check(lib.rcn_synchronize(h))
