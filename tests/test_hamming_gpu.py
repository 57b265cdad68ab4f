"""The Hamming matcher on the GPU (reconstructor_amd/csrc/hamming.hip through reconstructor_amd/hamming.py) against tests/hamming_ref.py:
equality everywhere, everything is integer.  Random rows sit near d = 128, so distance ties are plentiful and a padded zero row (which
looks like d = 128) would win if it were not masked."""
import ctypes as C
import functools

import numpy as np
import pytest

import hamming_ref as hr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def cases():
    c = dict(hr.shape_cases())
    c.update(hr.planted_cases())
    c["far_rows"] = hr.far_rows_case()
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    q, t = cases()[name]
    return hr.knn2(q, t), hr.match_pair(q, t)[0]


def gpu_pair(ctx, q, t):
    """knn2 and the match table of one pair through the resident path, and the match table through rcn_match_pair_hamming."""
    from reconstructor_amd import hamming
    hamming.clear(ctx)
    hamming.upload(ctx, 5, q)
    hamming.upload(ctx, 2, t)
    stride = max(len(q), 1)
    knn = hamming.knn2(ctx, [(5, 2)], stride)[0, :len(q)]
    out, counts = hamming.match_grid(ctx, [(5, 2)], stride)
    assert counts[0] == (out[0] >= 0).sum() and (out[0, len(q):] == -1).all()
    pair = hamming.match_pair(ctx, q, t)
    hamming.clear(ctx)
    return knn, out[0, :len(q)], pair


@pytest.mark.parametrize("name", list(hr.shape_cases()) + list(hr.planted_cases()) + ["far_rows"])
def test_knn2_and_matches_equal_the_reference(gpu_ctx, name):
    q, t = cases()[name]
    want_knn, want_out = expected(name)
    knn, out, pair = gpu_pair(gpu_ctx, q, t)
    assert np.array_equal(knn, want_knn)
    assert np.array_equal(out, want_out) and np.array_equal(pair, want_out)


def test_planted_answers(gpu_ctx):
    """What the planted rows were planted to give, stated here and not only through the reference."""
    c = cases()
    knn, out, _ = gpu_pair(gpu_ctx, *c["twins"])
    assert knn[2].tolist() == [9, 3, 31, 3] and out[2] == -1
    knn, out, _ = gpu_pair(gpu_ctx, *c["exact"])
    assert knn[1, :2].tolist() == [5, 0] and out[1] == 5 and knn[2].tolist() == [11, 0, 12, 0] and out[2] == -1
    for d0, d1 in hr.EDGES:
        knn, out, pair = gpu_pair(gpu_ctx, *c["edge_%d_%d" % (d0, d1)])
        assert knn.tolist() == [[4, d0, 1, d1]] and out.tolist() == [-1] and pair.tolist() == [-1]
    knn, out, pair = gpu_pair(gpu_ctx, *c["edge_6_10"])
    assert knn.tolist() == [[4, 6, 1, 10]] and out.tolist() == [4] and pair.tolist() == [4]
    knn, out, _ = gpu_pair(gpu_ctx, *c["extremes"])
    assert knn.tolist() == [[1, 0, 0, 256], [0, 0, 2, 0]] and out.tolist() == [1, -1]
    knn, _, _ = gpu_pair(gpu_ctx, *c["extremes_only"])
    assert knn.tolist() == [[0, 256, 1, 256]] * 2
    knn, out, _ = gpu_pair(gpu_ctx, *c["far_rows"])
    assert knn[0].tolist() == [3, 5, 4099, 5] and knn[1, :2].tolist() == [4099, 3] and out.tolist() == [-1, 4099]


def test_counts_on_the_device_clamp_and_mask(gpu_ctx):
    """counts_dev of -1, 0, 1, K - 1, K, K + 7; the slots past the rows in use hold copies of another image's rows."""
    import torch
    from reconstructor_amd import hamming
    K = 40
    by, counts = hr.counts_case(K)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    want, wn = hr.match_grid({i: (by[i], counts[i]) for i in range(6)}, pairs, stride=K)
    hamming.clear(gpu_ctx)
    hamming.upload_batch_device(gpu_ctx, 0, torch.from_numpy(by).cuda(), torch.from_numpy(counts).cuda())
    assert hamming.count(gpu_ctx) == 6
    out, n = hamming.match_grid(gpu_ctx, pairs, K)
    knn = hamming.knn2(gpu_ctx, pairs, K)
    hamming.clear(gpu_ctx)
    assert np.array_equal(out, want) and np.array_equal(n, wn) and wn.sum() > 40
    for p, (a, b) in enumerate(pairs):
        ra, rb = hr.rows_of(counts[a], K), hr.rows_of(counts[b], K)
        ref = hr.knn2(by[a, :ra], by[b, :rb])
        assert np.array_equal(knn[p, :ra], ref) and (knn[p, ra:] == -1).all()
        assert knn[p, :, 0].max() < max(rb, 1) and knn[p, :, 2].max() < max(rb, 1)          # a row past rows_i is never a neighbour
    # counts_dev == NULL: K rows each, the garbage takes part
    hamming.upload_batch_device(gpu_ctx, 0, torch.from_numpy(by).cuda(), None)
    out2, n2 = hamming.match_grid(gpu_ctx, pairs, K)
    hamming.clear(gpu_ctx)
    want2, wn2 = hr.match_grid({i: (by[i], None) for i in range(6)}, pairs, stride=K)
    assert np.array_equal(out2, want2) and np.array_equal(n2, wn2) and not np.array_equal(out2, out)


def test_grid_forms_and_chunking(gpu_ctx):
    """Six ragged images: pairs = NULL against the explicit list, a list with (j, i) and a repeated pair, out_stride > K, the host and
    the device form, and a forced small workspace (several chunks): the same bits as one chunk and as match_pair per pair."""
    from reconstructor_amd import hamming
    ims = hr.ragged_images()
    ids = sorted(ims)
    canon = [(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]]
    mixed = canon + [(b, a) for a, b in canon[::2]] + [canon[3], canon[3], (ids[1], ids[5]), (ids[5], ids[1])]
    stride = 300
    want, wn = hr.match_grid({i: (b, None) for i, b in ims.items()}, mixed, stride=stride)
    assert wn.sum() > 200
    hamming.clear(gpu_ctx)
    try:
        for i in ids[::-1]:
            hamming.upload(gpu_ctx, i, ims[i])
        a, an = hamming.match_grid(gpu_ctx, None, stride, n_pairs=len(canon))
        b, bn = hamming.match_grid(gpu_ctx, canon, stride)
        assert np.array_equal(a, want[:len(canon)]) and np.array_equal(an, wn[:len(canon)]) and np.array_equal(a, b) and np.array_equal(an, bn)
        m, mn = hamming.match_grid(gpu_ctx, mixed, stride)
        assert np.array_equal(m, want) and np.array_equal(mn, wn)
        w, wnn = hamming.match_grid(gpu_ctx, mixed, stride + 77)                           # out_stride > K
        assert np.array_equal(w[:, :stride], want) and (w[:, stride:] == -1).all() and np.array_equal(wnn, wn)
        d, dn = hamming.match_grid_device(gpu_ctx, mixed, stride)
        gpu_ctx.check(gpu_ctx.lib.rcn_synchronize(gpu_ctx.h))
        assert np.array_equal(d.cpu().numpy(), want) and np.array_equal(dn.cpu().numpy(), wn)
        knn_one = hamming.knn2(gpu_ctx, mixed, stride)
        for rows in (300, 700, 2000):                                                      # 1, 2 and 6 pairs per chunk
            hamming.set_workspace_rows(gpu_ctx, rows)
            c, cn = hamming.match_grid(gpu_ctx, mixed, stride)
            assert np.array_equal(c, want) and np.array_equal(cn, wn), rows
            assert np.array_equal(hamming.knn2(gpu_ctx, mixed, stride), knn_one), rows
        hamming.set_workspace_rows(gpu_ctx, 0)
        for p, (x, y) in enumerate(mixed[:len(canon)]):
            assert np.array_equal(hamming.match_pair(gpu_ctx, ims[x], ims[y]), want[p, :len(ims[x])])
        # remove: the canonical grid shrinks to the images left
        hamming.remove(gpu_ctx, ids[0])
        left = [(x, y) for x, y in canon if ids[0] not in (x, y)]
        r, rn = hamming.match_grid(gpu_ctx, None, stride, n_pairs=len(left))
        keep = [p for p, pr in enumerate(canon) if pr in left]
        assert hamming.count(gpu_ctx) == 5 and np.array_equal(r, want[keep]) and np.array_equal(rn, wn[keep])
    finally:
        hamming.set_workspace_rows(gpu_ctx, 0)
        hamming.clear(gpu_ctx)


def test_binary_and_float_residencies_do_not_touch_each_other(gpu_ctx):
    from reconstructor_amd import hamming, synth
    from reconstructor_amd.matcher import HipL2Matcher, all_pairs
    m = HipL2Matcher(ctx=gpu_ctx)
    m.clear()
    hamming.clear(gpu_ctx)
    fl = synth.descriptor_set("superpoint", 3, [200, 130, 257], n_world=400, seed=5)
    for i, im in enumerate(fl):
        m.upload(i, im)
    pairs = all_pairs(3)
    f0, fn0 = m.match_grid(pairs, 257)
    ims = hr.ragged_images()
    ids = sorted(ims)[3:]
    for i in ids:
        hamming.upload(gpu_ctx, i, ims[i])
    bp = [(ids[0], ids[1]), (ids[1], ids[2]), (ids[2], ids[0])]
    b0, bn0 = hamming.match_grid(gpu_ctx, bp, 300)
    f1, fn1 = m.match_grid(pairs, 257)                       # the float grid with binary rows resident
    assert gpu_ctx.lib.rcn_desc_count(gpu_ctx.h) == 3 and hamming.count(gpu_ctx) == 3
    m.clear()                                                # rcn_desc_clear
    assert gpu_ctx.lib.rcn_desc_count(gpu_ctx.h) == 0 and hamming.count(gpu_ctx) == 3
    b1, bn1 = hamming.match_grid(gpu_ctx, bp, 300)
    for i, im in enumerate(fl):
        m.upload(i, im)
    hamming.clear(gpu_ctx)
    assert gpu_ctx.lib.rcn_desc_count(gpu_ctx.h) == 3 and hamming.count(gpu_ctx) == 0
    f2, fn2 = m.match_grid(pairs, 257)                       # ... and after the binary rows are gone
    m.clear()
    assert fn0.sum() > 0 and bn0.sum() > 0
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2) and np.array_equal(fn0, fn1) and np.array_equal(fn0, fn2)
    assert np.array_equal(b0, b1) and np.array_equal(bn0, bn1)
    want, wn = hr.match_grid({i: (ims[i], None) for i in ids}, bp, stride=300)
    assert np.array_equal(b0, want) and np.array_equal(bn0, wn)


def test_chain_from_orb_to_lists(gpu_ctx):
    """Images -> rcn_orb_detect_and_compute_device with bytes_out_dev -> rcn_bits_upload_batch_device with ORB's own counts_dev -> the
    grid -> rcn_match_compact_begin: the lists equal hamming_ref on the copied bytes."""
    import torch
    import orb_ref
    from reconstructor_amd import hamming, orb
    from reconstructor_amd.matcher import HipL2Matcher
    imgs = np.stack([orb_ref.corner_image(128, 160, s, n_rect=70) for s in (31, 31, 32)])
    imgs[1] = np.clip(imgs[1].astype(np.int32) + np.random.default_rng(2).integers(-3, 4, imgs[1].shape), 0, 255).astype(np.uint8)      # image 0 again, other noise
    K = 100                                                  # ORB finds 124, 132 and 87 keypoints: counts above and below K
    r = orb.detect_and_compute(gpu_ctx, torch.from_numpy(imgs).cuda(), K)
    hamming.clear(gpu_ctx)
    hamming.upload_batch_device(gpu_ctx, 0, r["packed"], r["counts"])
    pairs = [(0, 1), (0, 2), (1, 2)]
    table, counts = hamming.match_grid_device(gpu_ctx, None, K, n_pairs=3)
    offsets = np.zeros(4, np.int64)
    qt = np.zeros((3 * K, 2), np.int32)
    total = C.c_int64()
    gpu_ctx.check(gpu_ctx.lib.rcn_match_compact_begin(gpu_ctx.h, table.data_ptr(), K, counts.data_ptr(), 3, offsets.ctypes.data, qt.ctypes.data,
                                                      len(qt), C.byref(total)))
    gpu_ctx.check(gpu_ctx.lib.rcn_match_compact_wait(gpu_ctx.h))
    hamming.clear(gpu_ctx)
    by, cn = r["packed"].cpu().numpy(), r["counts"].cpu().numpy()
    assert cn.max() > K > cn.min() >= 2
    want, wn = hr.match_grid({i: (by[i], cn[i]) for i in range(3)}, pairs, stride=K)
    assert total.value == offsets[-1] == wn.sum() and wn[0] > 20
    for p in range(3):
        got = [(int(a), int(b)) for a, b in qt[offsets[p]:offsets[p + 1]]]
        assert got == [(i, int(want[p, i])) for i in range(K) if want[p, i] >= 0]
    # how far the L2-on-bytes-as-floats grid is from it on the same images (printed, not asserted)
    m = HipL2Matcher(ctx=gpu_ctx)
    m.clear()
    rows = r["rows"].cpu().numpy()
    for i in range(3):
        m.upload(i, rows[i, :hr.rows_of(cn[i], K)])
    l2, _ = m.match_grid(pairs, K)
    m.clear()
    differ = sum(int(not np.array_equal(l2[p], want[p])) for p in range(3))
    print("Hamming against L2 on the byte values: %d of 3 lists differ, %d of %d query rows" % (differ, int((l2 != want).sum()), 3 * K))


def test_argument_errors(gpu_ctx):
    import torch
    from reconstructor_amd import hamming
    lib, h = gpu_ctx.lib, gpu_ctx.h
    hamming.clear(gpu_ctx)
    rows = hr.random_rows(np.random.default_rng(0), 8)
    out = np.zeros(64, np.int32)
    cnt = C.c_int32()
    dev = torch.zeros(8 * 64, dtype=torch.uint8).cuda()
    for nb in (16, 64, 0, 31):
        assert lib.rcn_bits_upload(h, 0, rows.ctypes.data, 4, nb) == -1
        assert lib.rcn_bits_upload_batch_device(h, 0, 1, dev.data_ptr(), None, 4, nb) == -1
        assert lib.rcn_match_pair_hamming(h, rows.ctypes.data, 4, rows.ctypes.data, 4, nb, 0.7, out.ctypes.data, C.byref(cnt)) == -1
    free0 = torch.cuda.mem_get_info()[0]
    assert lib.rcn_bits_upload(h, 0, rows.ctypes.data, 32769, 32) == -1                      # refused before anything is allocated
    assert lib.rcn_bits_upload_batch_device(h, 0, 1, dev.data_ptr(), None, 32769, 32) == -1
    assert lib.rcn_match_pair_hamming(h, rows.ctypes.data, 4, rows.ctypes.data, 32769, 32, 0.7, out.ctypes.data, C.byref(cnt)) == -1
    assert torch.cuda.mem_get_info()[0] == free0 and hamming.count(gpu_ctx) == 0
    assert lib.rcn_bits_upload(h, 0, rows.ctypes.data, -1, 32) == -1 and lib.rcn_bits_upload(h, 0, None, 4, 32) == -1
    assert lib.rcn_bits_upload_batch_device(h, 0, 2, None, None, 4, 32) == -1 and lib.rcn_bits_upload_batch_device(h, 0, -1, dev.data_ptr(), None, 4, 32) == -1
    assert lib.rcn_match_pair_hamming(h, None, 4, rows.ctypes.data, 4, 32, 0.7, out.ctypes.data, C.byref(cnt)) == -1
    assert lib.rcn_match_pair_hamming(h, rows.ctypes.data, 4, None, 4, 32, 0.7, out.ctypes.data, C.byref(cnt)) == -1
    assert lib.rcn_match_pair_hamming(h, rows.ctypes.data, 4, rows.ctypes.data, 4, 32, 0.7, None, C.byref(cnt)) == -1
    assert lib.rcn_match_pair_hamming(h, rows.ctypes.data, 4, rows.ctypes.data, 4, 32, 0.7, out.ctypes.data, None) == -1
    hamming.upload(gpu_ctx, 1, rows)
    hamming.upload(gpu_ctx, 2, rows[:5])
    pr = np.array([[1, 2]], np.int32)
    bad = np.array([[1, 3]], np.int32)
    tab = torch.zeros(64, dtype=torch.int32).cuda()
    for fn, o, c in ((lib.rcn_match_grid_hamming, out.ctypes.data, out.ctypes.data), (lib.rcn_match_grid_hamming_device, tab.data_ptr(), tab.data_ptr())):
        assert fn(h, bad.ctypes.data, 1, 0.7, o, 8, c) == -5                                 # unknown id
        assert fn(h, pr.ctypes.data, 1, 0.7, o, 7, c) == -1                                  # out_stride < K
        assert fn(h, pr.ctypes.data, 1, 0.7, None, 8, c) == -1 and fn(h, pr.ctypes.data, 1, 0.7, o, 8, None) == -1
        assert fn(h, pr.ctypes.data, -1, 0.7, o, 8, c) == -1
        assert fn(h, None, 2, 0.7, o, 8, c) == -1                                            # two residents: the canonical grid has one pair
        assert fn(h, pr.ctypes.data, 0, 0.7, None, 8, None) == 0
    assert b"RCN_" not in lib.rcn_last_error(h)
    assert lib.rcn_hamming_knn2_device(h, bad.ctypes.data, 1, tab.data_ptr(), 8) == -5
    assert lib.rcn_hamming_knn2_device(h, pr.ctypes.data, 1, tab.data_ptr(), 7) == -1
    assert lib.rcn_hamming_knn2_device(h, pr.ctypes.data, 1, None, 8) == -1
    assert lib.rcn_bits_remove(h, 99) == 0 and hamming.count(gpu_ctx) == 2                   # a no-op, as rcn_desc_remove
    assert lib.rcn_bits_count(None) == -1 and lib.rcn_bits_clear(None) == -1
    got, n = hamming.match_grid(gpu_ctx, pr, 8)                                              # the ctx still works
    assert np.array_equal(got[0], hr.match_pair(rows, rows[:5])[0])
    hamming.clear(gpu_ctx)
