"""GPU: tbdk_connected_components (opencv_amd.imgproc.connected_components[_with_stats]) against the outputs
recorded from the real reference (tests/golden/reference_cc.npz): labels, N, stats and centroids, bit for bit (a NaN
centroid as NaN, no other exemption); a stats capacity below N; stats and centroids left out; pitched images and
labels; one 1080p frame and a frame whose coordinate sums pass 2^32, against the numpy restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cc_cases as LC
import _cc_oracle as CO
import _oracle as O
import _reference_cases as RC
import _views as V

pytestmark = pytest.mark.gpu

CASES = LC.cases()
SENT_I, SENT_F = -123456789, -7.25  # what unwritten stats / centroid rows must still hold


def IP():
    from opencv_amd import imgproc

    return imgproc


@pytest.fixture(scope="module")
def fx():
    return RC.fixture("cc")


def run(gpu, img, conn, t, cap, labels=None):
    dev = img.device if isinstance(img, torch.Tensor) else "cuda"
    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).cuda()
    stats = torch.full((cap, 5), SENT_I, dtype=torch.int32, device=dev)
    cent = torch.full((cap, 2), SENT_F, dtype=torch.float64, device=dev)
    n, labels, stats, cent = IP().connected_components_with_stats(src, labels, stats, cent, conn, t, cap, ctx=gpu)
    return int(n.item()), labels, stats.cpu().numpy(), cent.cpu().numpy()


def untouched(stats, cent, frm):
    return bool((stats[frm:] == SENT_I).all() and (cent[frm:] == SENT_F).all())


@pytest.mark.parametrize("i", range(len(CASES)), ids=lambda i: LC.label(i).replace(" ", "_"))
def test_equals_the_recorded_reference(gpu, fx, i):
    content, w, h, conn, t = CASES[i]
    rn, rstats, rcent = LC.unpack_stats(fx[f"{i}_s"])
    cap = rn + 3
    n, labels, stats, cent = run(gpu, LC.image(content, w, h), conn, t, cap)
    assert n == rn, LC.label(i)
    got, want = LC.stored_labels(labels.cpu().numpy()), fx[f"{i}_labels"]
    assert got.shape == want.shape and np.array_equal(got, want), LC.label(i)
    assert np.array_equal(stats[:n], rstats), LC.label(i)
    assert CO.same_centroids(cent[:n], rcent), LC.label(i)
    assert untouched(stats, cent, n), LC.label(i)


@pytest.fixture(scope="module")
def noisy():
    img = LC.image("noise0.6", 130, 121)
    return img, {(conn, t): CO.connected_components_with_stats(img, conn, t)
                 for conn, t in ((4, LC.CCL_WU), (8, LC.CCL_GRANA))}


@pytest.mark.parametrize("conn,t", [(4, LC.CCL_WU), (8, LC.CCL_GRANA)])
def test_a_capacity_below_n(gpu, noisy, conn, t):
    img, refs = noisy
    rn, rlabels, rstats, rcent = refs[conn, t]
    for cap in (1, 2, rn // 2, rn - 1, rn):
        n, labels, stats, cent = run(gpu, img, conn, t, cap)
        assert n == rn > 8 and np.array_equal(labels.cpu().numpy(), rlabels), cap  # N is true, the labels complete
        k = min(cap, rn)
        assert np.array_equal(stats[:k], rstats[:k]) and CO.same_centroids(cent[:k], rcent[:k]), cap
    # and with room to spare the rows from N on stay as they were
    n, _, stats, cent = run(gpu, img, conn, t, rn + 100)
    assert n == rn and np.array_equal(stats[:n], rstats) and untouched(stats, cent, n)


def test_stats_and_centroids_left_out(gpu, noisy):
    from opencv_amd import _lib

    img, refs = noisy
    rn, rlabels, rstats, rcent = refs[8, LC.CCL_GRANA]
    src = torch.from_numpy(img).cuda()
    n, labels = IP().connected_components(src, ctx=gpu)
    assert int(n.item()) == rn and np.array_equal(labels.cpu().numpy(), rlabels)
    # one of the two
    h, w = img.shape
    lab = torch.empty((h, w), dtype=torch.int32, device="cuda")
    nd = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats = torch.full((rn, 5), SENT_I, dtype=torch.int32, device="cuda")
    cent = torch.full((rn, 2), SENT_F, dtype=torch.float64, device="cuda")

    def raw(s, c, cap, conn=8, t=-1, ww=w, lp=w * 4):
        return gpu.lib.tbdk_connected_components(gpu.handle, C.c_void_p(src.data_ptr()), ww, h, w,
                                                 C.c_void_p(lab.data_ptr()), lp, conn, t,
                                                 None if s is None else C.c_void_p(s.data_ptr()),
                                                 None if c is None else C.c_void_p(c.data_ptr()), cap,
                                                 C.c_void_p(nd.data_ptr()), None)

    assert raw(stats, None, rn) == _lib.TBDK_OK
    assert np.array_equal(stats.cpu().numpy(), rstats) and bool((cent == SENT_F).all())
    stats.fill_(SENT_I)
    assert raw(None, cent, rn) == _lib.TBDK_OK
    assert CO.same_centroids(cent.cpu().numpy(), rcent) and bool((stats == SENT_I).all())
    assert int(nd.item()) == rn and np.array_equal(lab.cpu().numpy(), rlabels)
    # argument checks: nothing enqueued, nothing written
    lab.fill_(-5)
    nd.fill_(-5)
    for kw in (dict(conn=6), dict(t=2), dict(t=-2), dict(cap=0), dict(cap=-1), dict(ww=0), dict(ww=w + 1), dict(lp=w * 4 - 4),
               dict(lp=w * 4 + 2)):
        args = dict(s=stats, c=cent, cap=rn)
        args.update(kw)
        assert raw(**args) == _lib.TBDK_EINVAL, kw
    torch.cuda.synchronize()
    assert bool((lab == -5).all()) and int(nd.item()) == -5


@pytest.mark.parametrize("layout", ["odd_both", "odd_pitch"])
def test_pitched_image_and_labels(gpu, noisy, layout):
    img, refs = noisy
    rn, rlabels, rstats, rcent = refs[8, LC.CCL_GRANA]
    sp, sv = V.window(img, layout, seed=3, device="cuda")
    wide = torch.full((img.shape[0] + 2, img.shape[1] + 7), -9, dtype=torch.int32, device="cuda")
    lv = wide[1:-1, 3:3 + img.shape[1]]
    n, labels, stats, cent = run(gpu, sv, 8, LC.CCL_GRANA, rn, labels=lv)
    assert labels is lv and n == rn and np.array_equal(lv.cpu().numpy(), rlabels)
    assert np.array_equal(stats, rstats) and CO.same_centroids(cent, rcent)
    wide[1:-1, 3:3 + img.shape[1]] = -9
    assert bool((wide == -9).all())  # nothing beside the window was written


def test_a_1080p_frame_of_the_benchmark_sequence(gpu):
    """64 x 4 pixel workgroups in the thousands and a component of 1.5 M pixels.  Connectivity 8 with CCL_DEFAULT is
    the Grana numbering, whose keys are 2 x 2 blocks: 960 x 540 keys in 507 scan tiles of 1024, so the tile scan's
    loop takes one turn here; test_the_wu_numbering_above_1024_scan_tiles takes the second"""
    from opencv_amd import klt

    frames, _ = klt.synth_render(20261015, 1920, 1080, 128, 0, 1, ctx=gpu)
    mask = ((frames[0] > 96) * 255).to(torch.uint8)
    host = mask.cpu().numpy()
    assert np.array_equal(host, ((O.synth(20261015, 1920, 1080, 128, 0, 1)[0][0] > 96) * 255).astype(np.uint8))
    rn, rlabels, rstats, rcent = CO.connected_components_with_stats(host, 8, LC.CCL_DEFAULT)
    assert rn > 100 and rstats[1:, 4].max() > 1 << 20
    n, labels, stats, cent = run(gpu, mask, 8, LC.CCL_DEFAULT, rn)
    assert n == rn and np.array_equal(labels.cpu().numpy(), rlabels)
    assert np.array_equal(stats, rstats) and CO.same_centroids(cent, rcent)


@pytest.mark.parametrize("conn,content", [(4, "noise0.5"), (8, "noise0.3")])
def test_the_wu_numbering_above_1024_scan_tiles(gpu, conn, content):
    """The Wu numbering keys every pixel, and the scan of the tile sums (cc_scan_tiles_kernel) takes 1024 tiles of
    1024 keys a turn, carrying the running total into the next: 1100 x 960 = 1,056,000 pixels are 1032 tiles, the
    smallest frame of this shape whose last tiles are numbered in the second turn.  Noise keeps the components small
    (the numpy restatement labels it in a few seconds; at connectivity 8 only below the percolation density) and
    their number, tens of thousands, far above one turn's: labels, N, stats and centroids bit for bit"""
    w, h = 1100, 960
    ntiles = (w * h + 1023) // 1024  # ccl.hip: nkeys = width * height unless Grana, kScanTile = 1024
    assert w * h > 1 << 20 and ntiles > 1024
    img = LC.image(content, w, h)
    rn, rlabels, rstats, rcent = CO.connected_components_with_stats(img, conn, LC.CCL_WU)
    assert rn > 30000 and rlabels[h - 1].max() > rlabels[:h - 8].max()  # labels first met in the last tiles
    n, labels, stats, cent = run(gpu, img, conn, LC.CCL_WU, rn)
    assert n == rn and np.array_equal(labels.cpu().numpy(), rlabels)
    assert np.array_equal(stats, rstats) and CO.same_centroids(cent, rcent)


def test_coordinate_sums_above_32_bits(gpu):
    """65535 x 40, all foreground but one column: sum x is 8.6e10, and the one component is 65534 pixels wide"""
    img = np.full((40, 65535), 255, np.uint8)
    img[:, 65534] = 0
    rn, rlabels, rstats, rcent = CO.connected_components_with_stats(img, 4, LC.CCL_WU)
    assert rn == 2 and rcent[1, 0] * rstats[1, 4] > 2.0 ** 36
    n, labels, stats, cent = run(gpu, img, 4, LC.CCL_WU, 2)
    assert n == 2 and np.array_equal(labels.cpu().numpy(), rlabels)
    assert np.array_equal(stats, rstats) and CO.same_centroids(cent, rcent)
