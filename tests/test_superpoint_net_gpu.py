"""GPU suite of SuperPoint's convolutional network (csrc/superpoint_net.hip) against tests/spnet_ref.py.

Tolerance: per image max |x - x_f64| <= TOL x max |x_f64| with TOL = 4 x DEV32, DEV32 being what the fp32 torch transcription
of the published forward deviates on the same cases (measured and printed by tests/test_superpoint_net_ref.py); the factor 4
allows for the other reduction order (tiles, cin slices) and the device's sqrtf and division.  Everything else is bit for
bit: run to run, batch and chunk invariance, strides, byte input, the fused call, and the delta-weight case against the
float64 reference itself.  No keypoint set is compared with the float64 reference: a relative change of 4e-6 of one
confidence can reorder an NMS, and the flip cascades.  Measured on an MI355X: logits within 1.50e-6
(allowed 4.04e-6), descriptors within 1.22e-6 normalised (allowed 3.14e-6) and 1.29e-6 as they are (allowed 3.28e-6)."""
import ctypes as C

import numpy as np
import pytest

import spnet_ref as R
from test_superpoint_net_ref import DESC_TOL, LOGITS_TOL, rel_dev

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SENTINEL = -7777.0


def S():
    from reconstructor_amd import superpoint_net
    return superpoint_net


@pytest.fixture(scope="module")
def nets(gpu_ctx):
    """name -> Net on the session's ctx; made on first use, closed with the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = S().Net.from_state_dict(gpu_ctx, {"seeded": R.weights, "delta": R.delta_weights}[name]())
        return made[name]
    yield get
    for n in made.values():
        n.close()


def forward(ctx, net, imgs, normalize=True, sentinel=True):
    """imgs: numpy [n][H][W] or a CUDA tensor; returns (logits [n][Hc][Wc][65], desc [n][Hc][Wc][256]) as numpy."""
    import torch
    t = torch.from_numpy(np.array(imgs)).cuda() if isinstance(imgs, np.ndarray) else imgs
    n, H, W = t.shape
    out = None
    if sentinel:
        out = (torch.full((n, H // 8, W // 8, 65), SENTINEL, dtype=torch.float32).cuda(), torch.full((n, H // 8, W // 8, 256), SENTINEL, dtype=torch.float32).cuda())
    lg, ds = S().forward(ctx, net, t, normalize=normalize, out=out)
    return lg.cpu().numpy(), ds.cpu().numpy()


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("normalize", [True, False], ids=["normalised", "as_is"])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_parity(gpu_ctx, nets, H, W, normalize):
    img, lg64, ds64 = R.case(H, W, normalize)
    got = forward(gpu_ctx, nets("seeded"), img[None], normalize)
    dl, dd = rel_dev(got[0][0].transpose(2, 0, 1), lg64), rel_dev(got[1][0].transpose(2, 0, 1), ds64)
    print("%d x %d: logits %.3g (allowed %.3g), descriptors %.3g (allowed %.3g)" % (H, W, dl, LOGITS_TOL, dd, DESC_TOL[normalize]))
    assert dl <= LOGITS_TOL and dd <= DESC_TOL[normalize]
    assert same(got, forward(gpu_ctx, nets("seeded"), img[None], normalize))             # run to run


@pytest.mark.parametrize("H,W", [(40, 72), (8, 264)])
def test_delta_weights_exact(gpu_ctx, nets, H, W):
    """Shifts, channel picks, ReLU of non-negatives and max pooling: every sum has one non-zero term, so the device must EQUAL
    the float64 reference cast to fp32.  Pins taps, padding, pooling and channel indexing independently of any tolerance."""
    img = R.delta_image(H, W)
    lg64, ds64 = R.forward(R.delta_weights(), img, normalize=False)
    lg, ds = forward(gpu_ctx, nets("delta"), img[None], normalize=False)
    assert (lg64 != 0).any() and (ds64 != 0).any()
    assert np.array_equal(lg[0].transpose(2, 0, 1), lg64.astype(np.float32))
    assert np.array_equal(ds[0].transpose(2, 0, 1), ds64.astype(np.float32))


def test_batch_and_chunk_invariance(gpu_ctx, nets):
    H, W = 40, 72
    imgs = np.stack([R.image(H, W, seed) for seed in (0, 1, 2)])
    net = nets("seeded")
    batch = forward(gpu_ctx, net, imgs)
    assert not (batch[0] == SENTINEL).any() and not (batch[1] == SENTINEL).any()
    for i in range(3):
        alone = forward(gpu_ctx, net, imgs[i:i + 1])
        assert alone[0][0].tobytes() == batch[0][i].tobytes() and alone[1][0].tobytes() == batch[1][i].tobytes(), i
    assert rel_dev(batch[0][1].transpose(2, 0, 1), R.case(H, W, True, 1)[1]) <= LOGITS_TOL
    try:
        for chunk in (1, 2):
            S().set_chunk_images(gpu_ctx, chunk)
            assert same(forward(gpu_ctx, net, imgs), batch), chunk
    finally:
        S().set_chunk_images(gpu_ctx, 0)


def test_strided_input(gpu_ctx, nets):
    import torch
    H, W = 40, 72
    imgs = np.stack([R.image(H, W, seed) for seed in (0, 1)])
    want = forward(gpu_ctx, nets("seeded"), imgs)
    big = torch.full((2, H + 5, W + 3), 0.123, dtype=torch.float32).cuda()
    big[:, 2:2 + H, 1:1 + W] = torch.from_numpy(imgs).cuda()
    view = big[:, 2:2 + H, 1:1 + W]                      # a crop of a larger tensor, read through the strides
    assert not view.is_contiguous()
    assert same(forward(gpu_ctx, nets("seeded"), view), want)
    wide = torch.zeros((2, H, 2 * W), dtype=torch.float32).cuda()
    wide[:, :, ::2] = torch.from_numpy(imgs).cuda()
    assert same(forward(gpu_ctx, nets("seeded"), wide[:, :, ::2]), want)                 # stride_x = 2
    tr = torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 2, 1))).cuda().permute(0, 2, 1)   # column-major images
    assert same(forward(gpu_ctx, nets("seeded"), tr), want)


def test_u8_input(gpu_ctx, nets):
    import torch
    H, W = 40, 72
    u8 = np.random.default_rng(3).integers(0, 256, (2, H, W)).astype(np.uint8)
    u8[0, 0, :256 - 200] = np.arange(200, 256)           # the top of the range is there
    want = forward(gpu_ctx, nets("seeded"), S().prep_u8(u8))
    assert same(forward(gpu_ctx, nets("seeded"), torch.from_numpy(u8).cuda()), want)


@pytest.mark.parametrize("mode", [0, 1], ids=["reference_heat", "softmax_heat"])
def test_fused_detect_equals_three_calls(gpu_ctx, nets, mode):
    import torch
    from reconstructor_amd import keypoints
    H, W = 64, 96
    imgs = torch.from_numpy(np.stack([R.image(H, W, seed) for seed in (0, 1)])).cuda()
    net = nets("seeded")
    for K in (256, 20):                                   # room for all, and the cap
        lg, ds = S().forward(gpu_ctx, net, imgs)
        r = keypoints.detect(gpu_ctx, lg.permute(0, 3, 1, 2), H, W, K, mode=mode, want_heat=True)
        rows = keypoints.sample_batch(gpu_ctx, ds, r["xy"], r["counts"], channel_last=True)
        f = S().detect(gpu_ctx, net, imgs, K, mode=mode, want_heat=True)
        for key in ("xy", "conf", "counts", "rounds", "heat"):
            assert torch.equal(f[key], r[key]), key
        assert f["rows"].cpu().numpy().tobytes() == rows.cpu().numpy().tobytes()
        counts = f["counts"].cpu().numpy()
        assert (counts > 20).all() and (counts < 256).all()
        fr = f["rows"].cpu().numpy()
        for i in range(2):
            m = min(int(counts[i]), K)
            assert (fr[i, m:] == 0).all() and np.allclose(np.linalg.norm(fr[i, :m].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_non_finite_input_propagates(gpu_ctx, nets):
    img = R.image(16, 24).copy()
    img[5, 7] = np.nan
    lg, ds = forward(gpu_ctx, nets("seeded"), img[None])
    assert np.isnan(lg).any() and np.isnan(ds).any()


def test_argument_errors(gpu_ctx, nets):
    import torch
    from reconstructor_amd import _lib
    lib, h, net = gpu_ctx.lib, gpu_ctx.h, nets("seeded")
    params = S().pack_state_dict(R.weights())
    out = C.c_void_p()
    assert lib.rcn_sp_net_create(h, params.ctypes.data, params.size - 1, C.byref(out)) == ERR_ARG
    assert "parameters" in lib.rcn_last_error(h).decode() and "RCN_" not in lib.rcn_last_error(h).decode()
    assert lib.rcn_sp_net_create(h, params.ctypes.data, params.size + 1, C.byref(out)) == ERR_ARG
    assert lib.rcn_sp_net_create(h, None, params.size, C.byref(out)) == ERR_ARG
    assert lib.rcn_sp_net_create(h, params.ctypes.data, params.size, None) == ERR_ARG
    assert lib.rcn_sp_net_create(None, params.ctypes.data, params.size, C.byref(out)) == ERR_ARG
    assert out.value is None
    lib.rcn_sp_net_destroy(None)
    assert lib.rcn_sp_net_set_chunk_images(None, 1) == ERR_ARG

    n, H, W, K = 2, 16, 24, 32
    img = torch.rand((n, H, W), dtype=torch.float32).cuda()
    lg = torch.empty((n, H // 8, W // 8, 65), dtype=torch.float32).cuda()
    ds = torch.empty((n, H // 8, W // 8, 256), dtype=torch.float32).cuda()
    p = lambda t: None if t is None else t.data_ptr()

    def fwd(ctx=h, net_h=net.h, img=img, dtype=0, n=n, H=H, W=W, flags=1, lg=lg, ds=ds):
        return lib.rcn_sp_net_forward_device(ctx, net_h, p(img), dtype, H * W, W, 1, n, H, W, flags, p(lg), p(ds))
    assert fwd() == 0 and fwd(flags=0) == 0 and fwd(n=0) == 0
    assert fwd(ctx=None) == ERR_ARG and fwd(net_h=None) == ERR_ARG
    for name in ("img", "lg", "ds"):
        assert fwd(**{name: None}) == ERR_ARG, name
    assert fwd(n=-1) == ERR_ARG
    for bad in (0, -8, 12, 20, 7):
        assert fwd(H=bad) == ERR_ARG and fwd(W=bad) == ERR_ARG, bad
    assert fwd(H=65536, W=32768) == ERR_ARG              # H * W = 2^31
    assert fwd(dtype=2) == ERR_ARG and fwd(dtype=-1) == ERR_ARG
    assert fwd(flags=2) == ERR_ARG and fwd(flags=3) == ERR_ARG
    assert "RCN_" not in lib.rcn_last_error(h).decode()
    with _lib.Context(0) as other:                       # a net belongs to its ctx
        assert fwd(ctx=other.h) == ERR_ARG

    xy = torch.empty((n, K, 2), dtype=torch.int32).cuda()
    conf = torch.empty((n, K), dtype=torch.float32).cuda()
    cnt = torch.empty((n,), dtype=torch.int32).cuda()
    rows = torch.empty((n, K, 256), dtype=torch.float32).cuda()

    def det(net_h=net.h, img=img, dtype=0, n=n, H=H, W=W, flags=1, mode=0, thresh=0.015, radius=4, border=4, K=K, D=256, xy=xy, conf=conf, cnt=cnt,
            rows=rows):
        return lib.rcn_sp_net_detect_device(h, net_h, p(img), dtype, H * W, W, 1, n, H, W, flags, mode, thresh, radius, border, K, D, p(xy), p(conf),
                                            p(cnt), p(rows), None, None)
    assert det() == 0 and det(n=0) == 0 and det(conf=None) == 0
    assert det(net_h=None) == ERR_ARG and det(img=None) == ERR_ARG and det(n=-1) == ERR_ARG
    assert det(H=12) == ERR_ARG and det(W=0) == ERR_ARG and det(dtype=3) == ERR_ARG and det(flags=4) == ERR_ARG
    # the keypoint arguments' own errors pass through
    assert det(K=0) == ERR_ARG and det(radius=9) == ERR_ARG and det(border=-1) == ERR_ARG and det(mode=2) == ERR_ARG
    assert det(xy=None) == ERR_ARG and det(cnt=None) == ERR_ARG and det(rows=None) == ERR_ARG
    assert det(D=0) == ERR_ARG and det(D=257) == ERR_ARG
    gpu_ctx.check(lib.rcn_synchronize(h))
