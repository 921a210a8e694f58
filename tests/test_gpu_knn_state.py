"""GPU: tbdk_knn_* under the rules of tests/test_gpu_dirty_state.py (no result may depend on what the library's
device memory held before the call: the context's scratch filled with 0xFF / 0x7F, a larger call with other
parameters in between, a context whose every allocation is born dirty, the model's own among them) and of
tests/_streams.py (on a side stream behind a late producer, outputs consumed on that stream, the calls returning
while the stream is still blocked).  What is compared is everything: masks, the background image, the model, the
counters and the RNG state."""
import numpy as np
import pytest
import torch

import _knn_cases as KC
import _knn_oracle as KO
import _streams as ST
from test_gpu_dirty_state import BYTES, byte_param, cached, dirty_twice, fresh_context  # noqa: F401
from test_gpu_knn import assert_model, model_of, run, subtractor

pytestmark = pytest.mark.gpu

N = 10
SMALL = dict(w=130, h=121, cn=3, params=dict(rng_state=KC.SECOND_SEED))
GRAY = dict(w=67, h=23, cn=1, params=dict(nsamples=3, knn_samples=1, history=30))
BIG = dict(w=300, h=211, cn=1, params=dict(nsamples=16, dist2_threshold=900.0, shadow_value=33, rng_state=5))


def frames_of(c, n=N):
    return cached(("knn_frames", c["w"], c["h"], c["cn"], n), lambda: KC.GC.frames(c["w"], c["h"], n, c["cn"]))


def reference(c, n=N):
    def make():
        case = dict(n=n, rates=np.full(n, -1.0), bg=(n,))
        masks, bgs, m = KO.run_case(case, dict(KC.DEFAULTS, **c["params"]), frames_of(c, n))
        return masks, bgs[n], m.model()

    return cached(("knn_ref", c["w"], c["h"], c["cn"], n), make)


def whole_run(ctx, c, n=N):
    m = subtractor(c["params"], ctx)
    masks, bgs = run(m, frames_of(c, n), bg=(n,))
    return masks, bgs[n], model_of(m)


def same(got, c, what, n=N):
    wm, wb, wmodel = reference(c, n)
    assert np.array_equal(got[0], wm), (what, "masks")
    assert np.array_equal(got[1], wb), (what, "background")
    assert_model(got[2], wmodel, what)


@byte_param
@pytest.mark.parametrize("c", [SMALL, GRAY], ids=["bgr_130x121", "gray_67x23"])
def test_scratch(gpu, c, byte):
    # the subtractor owns its memory; whatever the context's scratch holds is none of its business
    dirty_twice(gpu, byte, lambda: whole_run(gpu, c), lambda g, what: same(g, c, what), 0, "knn")


def test_history(gpu):
    """a larger subtractor with other parameters works between the frames of a smaller one, and the other way round"""
    ms, mb = subtractor(SMALL["params"], gpu), subtractor(BIG["params"], gpu)
    fs, fb = frames_of(SMALL), frames_of(BIG, 4)
    small_masks, big_masks = [], []
    for t in range(N):
        small_masks.append(ms.apply(torch.from_numpy(fs[t]).cuda()))
        if t % 3 == 0:
            big_masks.append(mb.apply(torch.from_numpy(fb[t // 3]).cuda()))
    bgs, bgb = ms.getBackgroundImage(), mb.getBackgroundImage()
    torch.cuda.synchronize()
    same((np.stack([x.cpu().numpy() for x in small_masks]), bgs.cpu().numpy(), model_of(ms)), SMALL, "small among big")
    same((np.stack([x.cpu().numpy() for x in big_masks]), bgb.cpu().numpy(), model_of(mb)), BIG, "big among small", 4)


@byte_param
def test_fresh_context(byte):
    with fresh_context(byte) as ctx:
        for c in (SMALL, GRAY):
            same(whole_run(ctx, c), c, f"fresh context {c['w']}x{c['h']}")
        # before any frame the getters see an empty model, whatever the allocation held
        m = subtractor(GRAY["params"], ctx)
        masks, _ = run(m, frames_of(GRAY)[:2])
        m.reset()
        got = model_of(m)
        assert not got[0].any() and not got[1].any() and not got[2].any() and not got[3].any()
        assert not m.getBackgroundImage().cpu().numpy().any()
        del m


# ---- a side stream behind a late producer ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def side():
    """The protocol's stream for this module alone (see tests/test_gpu_blobs_state.py: the session's own stream
    must not be created by a module that runs before tests/test_gpu_streams.py)."""
    prev = ST._cal.pop("S", None)
    ST._cal["S"] = torch.cuda.Stream()
    yield ST._cal["S"]
    ST._cal.pop("S").synchronize()
    if prev is not None:
        ST._cal["S"] = prev


SIDE_N = 6


def jobs(gpu, c):
    """one job per frame of a fresh subtractor; the decoy frames are the sequence's later ones"""
    m = subtractor(c["params"], gpu)
    fr = frames_of(c, 2 * SIDE_N)
    wm, wb, wmodel = reference(c, SIDE_N)
    decoy_masks = KO.run_case(dict(n=SIDE_N, rates=np.full(SIDE_N, -1.0), bg=()), dict(KC.DEFAULTS, **c["params"]),
                              fr[SIDE_N:])[0]
    assert not np.array_equal(decoy_masks[1:], wm[1:])  # the decoy gives another answer
    out = []
    for t in range(SIDE_N):
        def call(S, b, o, t=t):
            with torch.cuda.stream(S):  # the model's tensors are allocated inside
                res = {"mask": m.apply(b["frame"], o["mask"], -1.0, stream=S)}
                if t == SIDE_N - 1:
                    res.update(bg=m.getBackgroundImage(stream=S), model=m.model(stream=S))
                return res

        def check(got, what, t=t):
            assert np.array_equal(got["mask"], wm[t]), (what, "mask", t)
            if t == SIDE_N - 1:
                assert np.array_equal(got["bg"], wb), (what, "background")
                s, i, n, cnt, r = got["model"]
                assert_model((s, i, n, cnt, int(r.view(np.uint64)[0])), wmodel, what)

        out.append(ST.Job({"frame": fr[t]}, {"frame": fr[SIDE_N + t]}, call=call, check=check,
                          outs={"mask": ((c["h"], c["w"]), torch.uint8)}))
    return m, out


@pytest.mark.parametrize("c", [SMALL, GRAY], ids=["bgr_130x121", "gray_67x23"])
def test_on_a_side_stream_behind_a_late_producer(gpu, side, c):
    ST.side_stream()
    for spin, expect_async, what in ((1.0, False, "warm-up"), (ST.ORDER_MS, False, "ordering"),
                                     (ST.ASYNC_MS, True, "asynchrony")):
        m, js = jobs(gpu, c)
        for t, j in enumerate(js):
            # the long spins sit in front of the first frame (the allocation, the clear) and of the last (the getters)
            ends = t in (0, SIDE_N - 1)
            ST.late(j, spin if ends else 1.0, expect_async and ends, f"knn {c['w']}x{c['h']} {what}, frame {t}")
        ST.side_stream().synchronize()
        del m


def test_all_frames_behind_one_spin(gpu, side):
    ST.side_stream()
    m, js = jobs(gpu, SMALL)
    ST.late(js, ST.ORDER_MS, False, "knn, all frames behind one spin", sequence=True)
    ST.side_stream().synchronize()
    del m
