"""GPU suite of the retrieval ImageMatcher (csrc/retrieval.hip, reconstructor_amd/retrieval.py) against tests/retr_ref.py.
Every comparison is bitwise unless it says otherwise."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import retr_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "retrieval_small.npz"))
    return {k: g[k] for k in g.files}


# ---------------------------------------------------------------------------------------------------------------- assign

@functools.lru_cache(maxsize=None)
def _assign_case(D, Cn):
    rng = np.random.default_rng(1000 * D + Cn)
    mu = rng.standard_normal((Cn, D)).astype(np.float32)
    x = rng.standard_normal((1000, D)).astype(np.float32)
    x[:200] = mu[rng.integers(0, Cn, 200)] + 0.05 * rng.standard_normal((200, D)).astype(np.float32)    # rows that sit at a centroid
    return mu, x, retr_ref.assign(x, mu)


@pytest.mark.parametrize("Cn", [1, 8, 65, 200])
@pytest.mark.parametrize("D", [32, 128, 256])
def test_assign(gpu_ctx, D, Cn):
    """C = 200 at D = 256 sweeps four LDS tiles, C = 65 two 64-lane groups of one tile; 1000 rows are four workgroups."""
    from reconstructor_amd import retrieval
    mu, x, want = _assign_case(D, Cn)
    cb = retrieval.Codebook(gpu_ctx, mu)
    xd = _dev(x)
    for rows in (1, 63, 64, 65, 1000):
        assert _bits(retrieval.assign(gpu_ctx, cb, xd[:rows].contiguous()).cpu().numpy(), want[:rows]), rows
    assert retrieval.assign(gpu_ctx, cb, xd[:0].contiguous()).shape == (0,)
    cb.close()


def test_assign_ties_go_to_the_lowest_index(gpu_ctx):
    from reconstructor_amd import retrieval
    rng = np.random.default_rng(3)
    D, Cn = 256, 200                                          # tiles of 64 centroids
    mu = rng.standard_normal((Cn, D)).astype(np.float32)
    mu[9] = mu[5]                                             # inside one tile
    mu[70] = mu[3]                                            # across two tiles
    mu[199] = mu[130]                                         # across two later tiles
    x = np.stack([mu[5], mu[9], mu[3], mu[70], mu[130], mu[199]]) + 0.01 * rng.standard_normal((6, D)).astype(np.float32)
    cb = retrieval.Codebook(gpu_ctx, mu)
    got = retrieval.assign(gpu_ctx, cb, _dev(x.astype(np.float32))).cpu().numpy()
    cb.close()
    assert got.tolist() == [5, 5, 3, 3, 130, 130] and _bits(got, retr_ref.assign(x, mu))
    # integer rows at equal distance from two centroids
    mu = np.zeros((4, 32), np.float32)
    mu[1, 0], mu[2, 0], mu[3, 1] = 2, 2, 2
    x = np.zeros((3, 32), np.float32)
    x[0, 0] = 1                                               # between 0 and 1 (and 2)
    x[1, 0], x[1, 1] = 2, 1                                   # nearest 1 and 2
    x[2, 0], x[2, 1] = 1, 1                                   # all four at distance 2
    cb = retrieval.Codebook(gpu_ctx, mu)
    got = retrieval.assign(gpu_ctx, cb, _dev(x)).cpu().numpy()
    cb.close()
    assert got.tolist() == [0, 1, 0] and _bits(got, retr_ref.assign(x, mu))


# ---------------------------------------------------------------------------------------------------------------- training

RAGGED = np.array([40, 0, 2, 17, 40, 33], np.int32)          # an image without rows, one with fewer rows than the stride of 3


@functools.lru_cache(maxsize=None)
def _ragged_scene():
    rng = np.random.default_rng(21)
    desc = rng.standard_normal((6, 40, 32)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=2, keepdims=True)
    return desc


@functools.lru_cache(maxsize=None)
def _ragged_history(stride):
    return retr_ref.train(_ragged_scene(), RAGGED, 6, 5, stride)


@pytest.mark.parametrize("stride", [1, 3])
def test_training_steps(gpu_ctx, stride):
    from reconstructor_amd import retrieval
    want = _ragged_history(stride)
    dev, cn = _dev(_ragged_scene()), _dev(RAGGED)
    for steps in (0, 1, 2, 5):
        cb = retrieval.train_codebook(gpu_ctx, dev, cn, n_centroids=6, iterations=steps, train_row_stride=stride)
        assert (cb.C, cb.D) == (6, 32) and _bits(cb.centroids(), want[steps]), steps
        cb.close()


def test_training_empty_cluster_keeps_its_centroid_and_too_few_rows_fail(gpu_ctx):
    from reconstructor_amd import _lib, retrieval
    desc = _ragged_scene().copy()
    rows = [(i, r) for i in range(6) for r in range(RAGGED[i])]
    second = rows[(1 * len(rows)) // 6]                       # M = 132, C = 6: the initial rows are training rows 0, 22, 44, ...
    desc[second[0], second[1]] = desc[0, 0]                   # centroids 0 and 1 start equal: 1 never wins a row
    want = retr_ref.train(desc, RAGGED, 6, 3, 1)
    assert _bits(want[0][0], want[0][1]) and _bits(want[3][1], want[0][1]) and not _bits(want[3][0], want[0][0])
    cb = retrieval.train_codebook(gpu_ctx, _dev(desc), _dev(RAGGED), n_centroids=6, iterations=3, train_row_stride=1)
    assert _bits(cb.centroids(), want[3])
    cb.close()
    with pytest.raises(_lib.RcnError) as e:                   # stride 3: 14 + 0 + 1 + 6 + 14 + 11 = 46 training rows
        retrieval.train_codebook(gpu_ctx, _dev(desc), _dev(RAGGED), n_centroids=47, iterations=1, train_row_stride=3)
    assert e.value.code == ERR_ARG
    cb = retrieval.train_codebook(gpu_ctx, _dev(desc), _dev(RAGGED), n_centroids=46, iterations=0, train_row_stride=3)
    assert _bits(cb.centroids(), retr_ref.train(desc, RAGGED, 46, 0, 3)[0])
    cb.close()


def test_supplied_codebook_reads_back_unchanged(gpu_ctx):
    from reconstructor_amd import retrieval
    mu = np.random.default_rng(4).standard_normal((65, 128)).astype(np.float32)
    cb = retrieval.Codebook(gpu_ctx, mu)
    assert (cb.C, cb.D) == (65, 128) and _bits(cb.centroids(), mu)
    cb.close()


def test_training_across_workspace_chunks(gpu_ctx):
    """With C D = 65536 the per-image workspace is half a MiB, so 2100 images take two chunks (of 2031) of the 1 GiB workspace.  On integer
    rows every sum is exact, so the same rows as ONE image (one chunk) must train the same centroids; and an image's G does not
    depend on the chunk it falls into."""
    from reconstructor_amd import retrieval
    n, D, Cn = 2100, 256, 256
    rows = np.random.default_rng(8).integers(0, 256, (n, D)).astype(np.float32)
    many, one = _dev(rows.reshape(n, 1, D)), _dev(rows.reshape(1, n, D))
    a = retrieval.train_codebook(gpu_ctx, many, None, n_centroids=Cn, iterations=2, train_row_stride=1)
    b = retrieval.train_codebook(gpu_ctx, one, None, n_centroids=Cn, iterations=2, train_row_stride=1)
    mu = a.centroids()
    assert _bits(mu, b.centroids()) and not _bits(mu, rows[(np.arange(Cn) * n) // Cn])
    G = retrieval.encode(gpu_ctx, a, many)
    tail = retrieval.encode(gpu_ctx, a, many[2024:2040].contiguous())              # the first chunk ends behind image 2030
    assert _bits(G[2024:2040].cpu().numpy(), tail.cpu().numpy()) and G[-1].abs().sum().item() > 0
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- encode

def test_encode_ragged(gpu_ctx):
    from reconstructor_amd import retrieval
    desc, mu = _ragged_scene(), _ragged_history(1)[5]
    want = retr_ref.encode(desc, RAGGED, mu)
    cb = retrieval.Codebook(gpu_ctx, mu)
    dev = _dev(desc)
    got = retrieval.encode(gpu_ctx, cb, dev, _dev(RAGGED)).cpu().numpy()
    assert _bits(got, want) and not got[1].any() and got[0].any()
    # the same image alone, in a batch, and under a larger K padding (whatever the padding holds)
    for i in (0, 2, 3):
        alone = retrieval.encode(gpu_ctx, cb, dev[i:i + 1].contiguous(), _dev(RAGGED[i:i + 1])).cpu().numpy()
        padded = np.full((1, 57, 32), 7.0, np.float32)
        padded[0, :RAGGED[i]] = desc[i, :RAGGED[i]]
        wide = retrieval.encode(gpu_ctx, cb, _dev(padded), _dev(RAGGED[i:i + 1])).cpu().numpy()
        assert _bits(alone[0], want[i]) and _bits(wide[0], want[i]), i
    full = retrieval.encode(gpu_ctx, cb, dev, None).cpu().numpy()                     # counts == NULL: K rows each
    assert _bits(full, retr_ref.encode(desc, None, mu))
    cb.close()


@pytest.mark.parametrize("Cn,D,K", [(200, 256, 30), (8200, 4, 50), (1, 1, 5)])
def test_encode_shapes(gpu_ctx, Cn, D, K):
    """200 x 256: slices of 40 columns, assignment over four tiles; 8200 x 4: more centroids than one workgroup's accumulators
    hold (two chunks of C), three tiles; 1 x 1: the smallest."""
    from reconstructor_amd import retrieval
    rng = np.random.default_rng(Cn + D)
    desc = rng.standard_normal((2, K, D)).astype(np.float32)
    mu = rng.standard_normal((Cn, D)).astype(np.float32)
    counts = np.array([K, K - 3], np.int32)
    cb = retrieval.Codebook(gpu_ctx, mu)
    got = retrieval.encode(gpu_ctx, cb, _dev(desc), _dev(counts)).cpu().numpy()
    cb.close()
    assert _bits(got, retr_ref.encode(desc, counts, mu))


# ---------------------------------------------------------------------------------------------------------------- similarity, top-k

@pytest.mark.parametrize("n", [1, 2, 12])
def test_similarity_and_topk_on_the_golden_scene(gpu_ctx, n):
    from reconstructor_amd import retrieval
    g = _golden()
    G = g["G"][:n]
    sim = retrieval.similarity(gpu_ctx, _dev(G), 32)
    assert sim.dtype.is_floating_point and sim.element_size() == 8
    assert _bits(sim.cpu().numpy(), g["sim"][:n, :n] if n == 12 else retr_ref.similarity(G, 32))
    for k in (1, n - 1, n + 5):
        if k < 1:
            continue
        nbr = retrieval.top_k(gpu_ctx, sim, k).cpu().numpy()
        assert nbr.shape == (n, max(min(k, n - 1), 0)) and _bits(nbr, retr_ref.top_k(sim.cpu().numpy(), k)), k
    if n == 12:
        assert _bits(retrieval.top_k(gpu_ctx, sim, 3).cpu().numpy(), g["nbr"])


def test_similarity_tiles_and_identical_images(gpu_ctx):
    """40 images are three tiles a side (mirrored blocks, a ragged last tile); images 7 and 31 are one image: equal similarities,
    the lower slot first."""
    from reconstructor_amd import retrieval
    rng = np.random.default_rng(12)
    G = rng.standard_normal((40, 3 * 256)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    G[31] = G[7]
    sim = retrieval.similarity(gpu_ctx, _dev(G), 256)
    s = sim.cpu().numpy()
    assert _bits(s, retr_ref.similarity(G, 256)) and _bits(s, s.T.copy()) and _bits(s[7], s[31])
    nbr = retrieval.top_k(gpu_ctx, sim, 39).cpu().numpy()
    assert _bits(nbr, retr_ref.top_k(s, 39))
    for i in range(40):
        if i not in (7, 31):
            row = nbr[i].tolist()
            assert row.index(31) == row.index(7) + 1
    assert nbr[7, 0] == 31 and nbr[31, 0] == 7


# ---------------------------------------------------------------------------------------------------------------- pairs

def test_pairs(gpu_ctx):
    import torch
    from reconstructor_amd import _lib, retrieval
    g = _golden()
    nbr = _dev(g["nbr"])
    assert _bits(retrieval.pairs(gpu_ctx, nbr, 3, first_img_id=100), g["pairs"])
    P = len(g["pairs"])
    assert _bits(retrieval.pairs(gpu_ctx, nbr, 3, first_img_id=100, capacity=P), g["pairs"])
    buf = torch.full((P, 2), -7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = gpu_ctx.lib.rcn_retr_pairs_device(gpu_ctx.h, C.c_void_p(nbr.data_ptr()), 12, 3, 100, C.c_void_p(buf.data_ptr()), P - 1, C.c_void_p(cnt.data_ptr()))
    assert rc == ERR_ARG and cnt.item() == P and str(P) in gpu_ctx.lib.rcn_last_error(gpu_ctx.h).decode()      # the needed count is written
    assert _bits(buf[:P - 1].cpu().numpy(), g["pairs"][:P - 1]) and (buf[P - 1] == -7).all()
    with pytest.raises(_lib.RcnError):
        retrieval.pairs(gpu_ctx, nbr, 3, capacity=0)
    # k >= n - 1: the canonical grid
    from reconstructor_amd.matcher import all_pairs
    sim = _dev(g["sim"])
    assert _bits(retrieval.pairs(gpu_ctx, retrieval.top_k(gpu_ctx, sim, 17), 17), all_pairs(12))
    assert retrieval.pairs(gpu_ctx, retrieval.top_k(gpu_ctx, sim[:1, :1].contiguous(), 4), 4).shape == (0, 2)


def test_image_pairs_equals_the_staged_calls(gpu_ctx):
    from reconstructor_amd import _lib, retrieval
    g = _golden()
    dev = _dev(g["scene"])
    cb = retrieval.train_codebook(gpu_ctx, dev, None, n_centroids=8, iterations=5, train_row_stride=1)
    assert _bits(cb.centroids(), g["centroids"][-1])
    for steps in (1, 3):
        c2 = retrieval.train_codebook(gpu_ctx, dev, None, n_centroids=8, iterations=steps, train_row_stride=1)
        assert _bits(c2.centroids(), g["centroids"][steps])
        c2.close()
    a = np.stack([retrieval.assign(gpu_ctx, cb, dev[i]).cpu().numpy() for i in range(12)])
    assert _bits(a, g["assign"])
    G = retrieval.encode(gpu_ctx, cb, dev)
    assert _bits(G.cpu().numpy(), g["G"])
    staged = retrieval.pairs(gpu_ctx, retrieval.top_k(gpu_ctx, retrieval.similarity(gpu_ctx, G, 32), 3), 3, first_img_id=100)
    got = retrieval.image_pairs(gpu_ctx, cb, dev, None, top_k=3, first_img_id=100)
    assert _bits(got, staged) and _bits(got, g["pairs"])
    with pytest.raises(_lib.RcnError) as e:
        retrieval.image_pairs(gpu_ctx, cb, dev, None, top_k=3, capacity=len(got) - 1)
    assert e.value.code == ERR_ARG
    assert retrieval.image_pairs(gpu_ctx, cb, dev[:1].contiguous(), None, top_k=3).shape == (0, 2)
    assert retrieval.image_pairs(gpu_ctx, cb, dev[:0].contiguous(), None, top_k=3).shape == (0, 2)
    cb.close()


# ---------------------------------------------------------------------------------------------------------------- end to end

def test_ring_scene_end_to_end(gpu_ctx):
    from oracle import orc
    from reconstructor_amd import retrieval
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    n, K, D, step, k = 24, 64, 32, 16, 4
    scene = retr_ref.ring_scene(n, K, D, step, 0.05, 1)
    dev = _dev(scene)
    cb = retrieval.train_codebook(gpu_ctx, dev, None, n_centroids=8, iterations=5)
    mu = cb.centroids()
    assert _bits(mu, retr_ref.train(scene, None, 8, 5)[-1])
    got = retrieval.image_pairs(gpu_ctx, cb, dev, None, top_k=k)
    sim = retrieval.similarity(gpu_ctx, retrieval.encode(gpu_ctx, cb, dev), D)
    nbr = retrieval.top_k(gpu_ctx, sim, k + 1).cpu().numpy()
    s = sim.cpu().numpy()
    cb.close()
    assert _bits(got, retr_ref.image_pairs(scene, None, mu, k))
    have = {tuple(p) for p in got.tolist()}
    assert all(retr_ref.ring_distance(a, b, n) <= 3 for a, b in have)
    assert all((min(i, (i + 1) % n), max(i, (i + 1) % n)) in have for i in range(n))
    assert min(s[i, nbr[i, k - 1]] - s[i, nbr[i, k]] for i in range(n)) > 1e-4
    m = HipL2Matcher(ctx=gpu_ctx)
    m.clear()
    m.upload_batch_device(0, n, dev.data_ptr(), K, D)
    out, counts = m.match_grid(got, K)
    _, full = m.match_grid(all_pairs(n), K)
    m.clear()
    exp, ec = orc.match_grid(list(scene), got, threads=2)
    assert np.array_equal(out, exp) and np.array_equal(counts, ec)
    print("retrieval: %d of %d pairs keep %d of the full grid's %d matches (%.1f %%)" % (len(got), n * (n - 1) // 2, counts.sum(), full.sum(),
                                                                                      100.0 * counts.sum() / max(int(full.sum()), 1)))


# ---------------------------------------------------------------------------------------------------------------- argument errors

def test_argument_errors(gpu_ctx):
    import torch
    from reconstructor_amd import _lib, retrieval
    L, h = gpu_ctx.lib, gpu_ctx.h
    desc = _dev(_ragged_scene())
    p = C.c_void_p(desc.data_ptr())
    out = C.c_void_p()
    opt = retrieval.options(6, 1, 1, 3)
    assert (lambda o: (o.n_centroids, o.iterations, o.train_row_stride, o.top_k))(retrieval.options()) == (64, 10, 0, 20)
    train = L.rcn_retr_codebook_train_device
    assert train(h, None, None, 6, 40, 32, C.byref(opt), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 6, 40, 32, C.byref(opt), None) == ERR_ARG
    assert train(h, p, None, -1, 40, 32, C.byref(opt), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 6, -1, 32, C.byref(opt), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 6, 40, 0, C.byref(opt), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 6, 40, 257, C.byref(opt), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 0, 40, 32, C.byref(opt), C.byref(out)) == ERR_ARG                     # no rows: M < C
    assert train(h, p, None, 8193, 40, 32, C.byref(opt), C.byref(out)) == ERR_UNSUPPORTED
    for bad in (retrieval.options(0, 1, 1), retrieval.options(6, -1, 1), retrieval.options(6, 1, -1)):
        assert train(h, p, None, 6, 40, 32, C.byref(bad), C.byref(out)) == ERR_ARG
    assert train(h, p, None, 6, 40, 32, C.byref(retrieval.options(2049, 1, 1)), C.byref(out)) == ERR_UNSUPPORTED     # C D > 65536
    assert not out.value
    mu = np.zeros((4, 32), np.float32)
    create = L.rcn_retr_codebook_create
    assert create(h, None, 4, 32, C.byref(out)) == ERR_ARG and create(h, mu.ctypes.data, 0, 32, C.byref(out)) == ERR_ARG
    assert create(h, mu.ctypes.data, 4, 300, C.byref(out)) == ERR_ARG and create(h, mu.ctypes.data, 4096, 32, C.byref(out)) == ERR_UNSUPPORTED
    assert L.rcn_retr_codebook_read(None, None, None, None) == ERR_ARG
    L.rcn_retr_codebook_destroy(None)
    cb = retrieval.Codebook(gpu_ctx, mu)
    cb16 = retrieval.Codebook(gpu_ctx, np.zeros((4, 16), np.float32))
    a = torch.zeros(64, dtype=torch.int32, device="cuda")
    ap = C.c_void_p(a.data_ptr())
    assert L.rcn_retr_assign_device(h, None, p, 4, ap) == ERR_ARG and L.rcn_retr_assign_device(h, cb.h, None, 4, ap) == ERR_ARG
    assert L.rcn_retr_assign_device(h, cb.h, p, -1, ap) == ERR_ARG and L.rcn_retr_assign_device(h, cb.h, p, 4, None) == ERR_ARG
    G = torch.zeros((6, 128), dtype=torch.float32, device="cuda")
    gp = C.c_void_p(G.data_ptr())
    enc = L.rcn_retr_encode_device
    assert enc(h, cb16.h, p, None, 6, 40, 32, gp) == ERR_ARG                                       # the codebook has another D
    assert enc(h, None, p, None, 6, 40, 32, gp) == ERR_ARG and enc(h, cb.h, None, None, 6, 40, 32, gp) == ERR_ARG
    assert enc(h, cb.h, p, None, 6, 40, 32, None) == ERR_ARG and enc(h, cb.h, p, None, -1, 40, 32, gp) == ERR_ARG
    assert enc(h, cb.h, p, None, 8193, 40, 32, gp) == ERR_UNSUPPORTED
    assert enc(h, cb.h, None, None, 0, 40, 32, None) == 0                                          # n == 0 launches nothing
    sim = torch.zeros((6, 6), dtype=torch.float64, device="cuda")
    sp = C.c_void_p(sim.data_ptr())
    simf = L.rcn_retr_similarity_device
    assert simf(h, None, 6, 128, 32, sp) == ERR_ARG and simf(h, gp, 6, 128, 32, None) == ERR_ARG and simf(h, gp, -1, 128, 32, sp) == ERR_ARG
    assert simf(h, gp, 6, 128, 48, sp) == ERR_ARG and simf(h, gp, 6, 0, 32, sp) == ERR_ARG and simf(h, gp, 8193, 128, 32, sp) == ERR_UNSUPPORTED
    assert simf(h, gp, 6, 65536 + 32, 32, sp) == ERR_UNSUPPORTED and simf(h, None, 0, 128, 32, None) == 0
    topk = L.rcn_retr_topk_device
    assert topk(h, sp, 6, 0, ap) == ERR_ARG and topk(h, None, 6, 2, ap) == ERR_ARG and topk(h, sp, 6, 2, None) == ERR_ARG
    assert topk(h, sp, -1, 2, ap) == ERR_ARG and topk(h, sp, 8193, 2, ap) == ERR_UNSUPPORTED and topk(h, None, 0, 2, None) == 0
    prs = L.rcn_retr_pairs_device
    assert prs(h, ap, 6, 0, 0, ap, 8, ap) == ERR_ARG and prs(h, None, 6, 2, 0, ap, 8, ap) == ERR_ARG and prs(h, ap, 6, 2, 0, ap, 8, None) == ERR_ARG
    assert prs(h, ap, 6, 2, 0, None, 8, ap) == ERR_ARG and prs(h, ap, 6, 2, 0, ap, -1, ap) == ERR_ARG and prs(h, ap, 8193, 2, 0, ap, 8, ap) == ERR_UNSUPPORTED
    host = np.zeros((32, 2), np.int32)
    cnt = C.c_int32(-1)
    ip = L.rcn_retr_image_pairs
    assert ip(h, cb.h, p, None, 6, 40, 32, 0, 0, host.ctypes.data, 32, C.byref(cnt)) == ERR_ARG   # top_k < 1
    assert ip(h, cb16.h, p, None, 6, 40, 32, 0, 2, host.ctypes.data, 32, C.byref(cnt)) == ERR_ARG
    assert ip(h, cb.h, None, None, 6, 40, 32, 0, 2, host.ctypes.data, 32, C.byref(cnt)) == ERR_ARG
    assert ip(h, cb.h, p, None, 6, 40, 32, 0, 2, None, 32, C.byref(cnt)) == ERR_ARG and ip(h, cb.h, p, None, 6, 40, 32, 0, 2, host.ctypes.data, 32, None) == ERR_ARG
    assert ip(h, cb.h, p, None, 6, 40, 32, 0, 2, host.ctypes.data, -1, C.byref(cnt)) == ERR_ARG
    assert ip(h, cb.h, p, None, 8193, 40, 32, 0, 2, host.ctypes.data, 32, C.byref(cnt)) == ERR_UNSUPPORTED
    assert ip(h, cb.h, None, None, 0, 40, 32, 0, 2, None, 0, C.byref(cnt)) == 0 and cnt.value == 0
    assert b"RCN_" not in L.rcn_last_error(h)
    cb.close()
    cb16.close()
