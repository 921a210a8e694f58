"""GPU: tbdk_morph_u8 and tbdk_connected_components under the rules of tests/test_gpu_dirty_state.py (no result may
depend on what the library's device memory held before the call: the context's scratch filled with 0xFF / 0x7F, a
larger call with other parameters in between, a context whose every allocation is born dirty) and of
tests/_streams.py (on a side stream behind a late producer, outputs consumed on that stream, the call returning
while the stream is still blocked)."""
import numpy as np
import pytest
import torch

import _cc_cases as LC
import _cc_oracle as CO
import _morph_cases as BC
import _morph_oracle as MO
import _streams as ST
from test_gpu_dirty_state import BYTES, byte_param, cached, dirty_twice, fresh_context  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 130, 121
BIG_W, BIG_H = 300, 211
CAP = 2048


def IP():
    from opencv_amd import imgproc

    return imgproc


def small():
    return cached("blobs_small", lambda: LC.image("noise0.6", W, H))


def big():
    return cached("blobs_big", lambda: LC.noise(BIG_W, BIG_H, 0.45, 77, (255, 127)))


def small_gray():
    return cached("blobs_small_gray", lambda: BC.image(W, H, "noise"))


def big_gray():
    return cached("blobs_big_gray", lambda: BC.image(BIG_W, BIG_H, "noise"))


MORPH = {"open_rect3": (BC.OPEN, "rect3x3", 1, BC.CONSTANT), "close_arb_x2": (BC.CLOSE, "arb5x4", 2, BC.REFLECT_101),
         "erode_ellipse15": (BC.ERODE, "ellipse15x15", 1, BC.REPLICATE)}


def morph_ref(img, key):
    op, name, it, border = MORPH[key]
    return cached(("morph", img.shape, key), lambda: MO.morphology_ex(img, op, BC.elements()[name], iterations=it,
                                                                      border=border))


def morph_call(ctx, img, key, stream=None):
    op, name, it, border = MORPH[key]
    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).cuda()
    return IP().morphology_ex(src, op, BC.elements()[name], iterations=it, borderType=border, ctx=ctx, stream=stream)


def cc_ref(img, conn, t):
    return cached(("cc", img.shape, conn, t), lambda: CO.connected_components_with_stats(img, conn, t))


def cc_call(ctx, img, conn, t, stream=None, cap=CAP):
    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).cuda()
    return IP().connected_components_with_stats(src, connectivity=conn, ccltype=t, max_labels=cap, ctx=ctx,
                                                stream=stream)


def cc_same(got, ref, what):
    n, labels, stats, cent = ref
    gn = int(np.asarray(got[0].cpu() if isinstance(got[0], torch.Tensor) else got[0]).reshape(-1)[0])
    g = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in got[1:]]
    assert gn == n and n <= CAP, (what, gn, n)
    assert np.array_equal(g[0], labels), what
    assert np.array_equal(g[1][:n], stats) and CO.same_centroids(g[2][:n], cent), what


@byte_param
@pytest.mark.parametrize("key", list(MORPH))
def test_scratch_morph(gpu, key, byte):
    img = small_gray()
    # four passes go through two scratch planes; the single 2-D pass of the ellipse through none
    dirty_twice(gpu, byte, lambda: morph_call(gpu, img, key).cpu().numpy(),
                lambda g, what: np.testing.assert_array_equal(g, morph_ref(img, key), what),
                0 if key == "erode_ellipse15" else 2 * W * H, f"morph {key}")


@byte_param
@pytest.mark.parametrize("conn,t", [(4, LC.CCL_DEFAULT), (8, LC.CCL_WU), (8, LC.CCL_GRANA)])
def test_scratch_connected_components(gpu, conn, t, byte):
    img = small()
    dirty_twice(gpu, byte, lambda: cc_call(gpu, img, conn, t), lambda g, what: cc_same(g, cc_ref(img, conn, t), what),
                W * H * 8, f"connected components {conn} {t}")


def test_history_morph(gpu):
    for key in MORPH:
        other = {"open_rect3": "erode_ellipse15", "close_arb_x2": "open_rect3", "erode_ellipse15": "close_arb_x2"}[key]
        for k, img in ((other, big_gray()), (key, small_gray()), (other, big_gray())):
            np.testing.assert_array_equal(morph_call(gpu, img, k).cpu().numpy(), morph_ref(img, k), f"{key}: {k}")


def test_history_connected_components(gpu):
    wide = big()
    for (conn, t), (oc, ot) in (((8, LC.CCL_GRANA), (4, LC.CCL_WU)), ((4, LC.CCL_WU), (8, LC.CCL_GRANA)),
                                ((8, LC.CCL_WU), (8, LC.CCL_GRANA))):
        cc_call(gpu, wide, oc, ot, cap=4 * CAP)
        cc_same(cc_call(gpu, small(), conn, t), cc_ref(small(), conn, t), f"{conn} {t} after {oc} {ot} on a larger image")
        n, labels, _, _ = cc_call(gpu, wide, oc, ot, cap=4 * CAP)
        ref = cc_ref(wide, oc, ot)
        assert int(n.item()) == ref[0] and np.array_equal(labels.cpu().numpy(), ref[1])


@byte_param
def test_fresh_context(byte):
    img = small()
    with fresh_context(byte) as ctx:
        for key in MORPH:
            np.testing.assert_array_equal(morph_call(ctx, small_gray(), key).cpu().numpy(),
                                          morph_ref(small_gray(), key), key)
        for conn, t in ((8, LC.CCL_GRANA), (4, LC.CCL_WU), (8, LC.CCL_WU)):
            cc_same(cc_call(ctx, img, conn, t), cc_ref(img, conn, t), f"fresh context {conn} {t}")


# ---- a side stream behind a late producer ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def side():
    """The protocol's stream for this module alone.  The session's own one (_streams.side_stream) is created by
    the first test that asks for it, and tests/test_gpu_streams.py's self-tests depend on where it falls among the
    streams the session creates (streams share a few hardware queues, dealt as they are created): this module,
    which runs earlier, must not be the one that creates it."""
    prev = ST._cal.pop("S", None)
    ST._cal["S"] = torch.cuda.Stream()
    yield ST._cal["S"]
    ST._cal.pop("S").synchronize()
    if prev is not None:
        ST._cal["S"] = prev


def flipped(img):
    return np.ascontiguousarray(img[::-1, ::-1])


def morph_job(gpu, key):
    img = small_gray()
    other = MO.morphology_ex(flipped(img), MORPH[key][0], BC.elements()[MORPH[key][1]], iterations=MORPH[key][2],
                             border=MORPH[key][3])
    assert (morph_ref(img, key) != other).mean() > 0.5  # the decoy gives another answer
    return ST.Job({"src": img}, {"src": flipped(img)},
                  call=lambda S, b, o: IP().morphology_ex(b["src"], MORPH[key][0], BC.elements()[MORPH[key][1]], o["dst"],
                                                          iterations=MORPH[key][2], borderType=MORPH[key][3], ctx=gpu,
                                                          stream=S),
                  check=lambda got, what: np.testing.assert_array_equal(got, morph_ref(img, key), what),
                  outs={"dst": ((H, W), torch.uint8)})


def cc_job(gpu, conn, t):
    img = small()
    ref = cc_ref(img, conn, t)
    assert ref[0] != CO.connected_components_with_stats(flipped(img), conn, t)[0] or not np.array_equal(
        ref[1], CO.connected_components_with_stats(flipped(img), conn, t)[1])

    def call(S, b, o):
        with torch.cuda.stream(S):  # the N tensor is allocated inside
            return IP().connected_components_with_stats(b["src"], o["labels"], o["stats"], o["cent"], conn, t, CAP,
                                                        ctx=gpu, stream=S)

    return ST.Job({"src": img}, {"src": flipped(img)}, call=call,
                  check=lambda got, what: cc_same(got, ref, what),
                  outs={"labels": ((H, W), torch.int32), "stats": ((CAP, 5), torch.int32),
                        "cent": ((CAP, 2), torch.float64)})


@pytest.mark.parametrize("key", list(MORPH))
def test_morph_on_a_side_stream_behind_a_late_producer(gpu, side, key):
    ST.side_stream()
    ST.late(morph_job(gpu, key), 1.0, False, f"morph {key}, warm-up")  # the scratch may grow here
    ST.late(morph_job(gpu, key), ST.ORDER_MS, False, f"morph {key}")
    ST.late(morph_job(gpu, key), ST.ASYNC_MS, True, f"morph {key}")
    ST.side_stream().synchronize()


@pytest.mark.parametrize("conn,t", [(4, LC.CCL_WU), (8, LC.CCL_GRANA)])
def test_connected_components_on_a_side_stream_behind_a_late_producer(gpu, side, conn, t):
    ST.side_stream()
    ST.late(cc_job(gpu, conn, t), 1.0, False, f"connected components {conn} {t}, warm-up")
    ST.late(cc_job(gpu, conn, t), ST.ORDER_MS, False, f"connected components {conn} {t}")
    ST.late(cc_job(gpu, conn, t), ST.ASYNC_MS, True, f"connected components {conn} {t}")
    ST.side_stream().synchronize()


def test_both_behind_one_spin(gpu, side):
    ST.side_stream()
    ST.late([morph_job(gpu, "close_arb_x2"), cc_job(gpu, 8, LC.CCL_GRANA), morph_job(gpu, "open_rect3"),
             cc_job(gpu, 4, LC.CCL_WU)], ST.ORDER_MS, False, "morph and connected components behind one spin")
    ST.side_stream().synchronize()
