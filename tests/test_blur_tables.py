"""The side-stream and far-view cases of tbdk_gaussian_blur_u8 and tbdk_threshold, registered with
tests/_streams_table.py and tests/_far_table.py.

tests/test_streams_cases.py requires a case (or an exclusion) in the streams table for every entry point of
include/tbdk.h that takes a `void* stream`, tests/test_far_cases.py one in the far table for every `*pitch`
parameter; tests/test_gpu_streams.py and tests/test_gpu_far_views.py run every case of them: ordering behind a late
producer, pairs behind one spin, the return while the stream is still blocked, images whose rows span 2 GiB and
4 GiB.  This module adds the two new entry points' cases through the tables' own add() when it is imported.  pytest
imports every test module of a run before it runs a test, and this file sorts before those four, so in a run of the
suite their parametrisation and their symbol-by-symbol checks see these cases like any other.  (A run of one of
those files on its own does not import this module and reports the new symbols as uncovered: run them with the
suite, or name this file too.)

The blur case is bgsegm.smooth_mask's call, 11 x 11 at sigma 3.5 with the threshold fused in, on the 0 / 127 / 255
runs image; the threshold case is THRESH_OTSU, whose histogram, scan and apply launches all follow the stream.

The CPU tests below hold what the registration must give: the cases are in the tables once, every new
stream-taking symbol and pitch parameter of the header has one, and the decoy inputs give another answer."""
import numpy as np

import _blur_cases as UC
import _blur_oracle as BO
import _far_table as FT
import _streams_table as T
import test_bgknn_tables  # noqa: F401  (registers its cases, so that the whole-header checks below hold in a run of this file alone)

SIZES = ((130, 121), (300, 5))
SYMBOLS = ("tbdk_gaussian_blur_u8", "tbdk_threshold")
PAIRS = [("blur_smooth_300x5", "blur_smooth_130x121"), ("threshold_otsu_300x5", "threshold_otsu_130x121")]
PITCHES = {("tbdk_gaussian_blur_u8", "src_pitch"), ("tbdk_gaussian_blur_u8", "dst_pitch"),
           ("tbdk_threshold", "src_pitch"), ("tbdk_threshold", "dst_pitch")}
FUSED = (10.0, 255.0, BO.BINARY)
OTSU = BO.TOZERO_INV | BO.OTSU


def _imgproc():
    from opencv_amd import imgproc

    return imgproc


def _blur_ref(i):
    return BO.gaussian_blur(i["src"], (11, 11), 3.5, 3.5, BO.REFLECT_101, threshold=FUSED)


def _blur_run(ctx, st, S, b, o, i):
    return _imgproc().gaussian_blur(b["src"], (11, 11), 3.5, o["dst"], 3.5, BO.REFLECT_101, S, FUSED, ctx=ctx)


def _thresh_ref(i):
    t, out = BO.threshold_u8(i["src"], 0.0, 255.0, OTSU)
    return np.array([int(t)], np.int32), out


def _thresh_run(ctx, st, S, b, o, i):
    return _imgproc().threshold(b["src"], 0.0, 255.0, OTSU, o["dst"], S, ctx=ctx)


def _blur_in_place(ctx, st, b, o, i):
    return _imgproc().gaussian_blur(b["src"], (11, 11), 3.5, b["src"], 3.5, BO.REFLECT_101, None, FUSED, ctx=ctx)


def _thresh_in_place(ctx, st, b, o, i):
    return _imgproc().threshold(b["src"], 0.0, 255.0, OTSU, b["src"], ctx=ctx)


def register():
    """adds the cases once, however often this module is imported or reloaded"""
    if "blur_smooth_130x121" in T.BY_NAME:
        return
    for sz in SIZES:
        outs = lambda i, s=sz: {"dst": ((s[1], s[0]), "uint8")}  # noqa: E731
        T.add(T.Case(f"blur_smooth_{sz[0]}x{sz[1]}", SYMBOLS[:1], T.one(lambda s=sz: {"src": UC.image(s[0], s[1], "runs")}),
                     T.single(_blur_ref), _blur_run, outs=outs))
        T.add(T.Case(f"threshold_otsu_{sz[0]}x{sz[1]}", SYMBOLS[1:],
                     T.one(lambda s=sz: {"src": UC.image(s[0], s[1], "noise")},
                           lambda s=sz: {"src": (UC.image(s[0], s[1], "noise") >> 1) + 90}),
                     T.single(_thresh_ref), _thresh_run, outs=outs))
    T.BY_NAME.update({c.name: c for c in T.CASES})
    T.PAIRS.extend(PAIRS)
    FT.add("blur_src", "blur_smooth_130x121", ("src",), ("tbdk_gaussian_blur_u8", "src_pitch"))
    FT.add("blur_dst", "blur_smooth_130x121", ("dst",), ("tbdk_gaussian_blur_u8", "dst_pitch"))
    FT.add("blur_in_place", "blur_smooth_130x121", ("src",),
           (("tbdk_gaussian_blur_u8", "src_pitch"), ("tbdk_gaussian_blur_u8", "dst_pitch")), run=_blur_in_place,
           share={"src": "io"})  # one image under both pitch parameters
    FT.add("threshold_src", "threshold_otsu_130x121", ("src",), ("tbdk_threshold", "src_pitch"))
    FT.add("threshold_dst", "threshold_otsu_130x121", ("dst",), ("tbdk_threshold", "dst_pitch"))
    FT.add("threshold_in_place", "threshold_otsu_130x121", ("src",),
           (("tbdk_threshold", "src_pitch"), ("tbdk_threshold", "dst_pitch")), run=_thresh_in_place,
           share={"src": "io"})
    FT.BY_NAME.update({c.name: c for c in FT.CASES})


register()


def test_the_cases_are_in_the_tables_once():
    names, far = [c.name for c in T.CASES], [c.name for c in FT.CASES]
    for a, b in PAIRS:
        for name in (a, b):
            assert names.count(name) == 1 and T.BY_NAME[name].sync is None, name  # asynchronous: both checks run
    assert all(T.PAIRS.count(p) == 1 for p in PAIRS)
    assert sum(n.startswith(("blur_", "threshold_")) for n in far) == 6
    register()
    assert [c.name for c in T.CASES] == names and [c.name for c in FT.CASES] == far


def test_every_new_symbol_and_pitch_parameter_has_a_case():
    from test_far_cases import pitch_parameters
    from test_streams_cases import stream_symbols

    cased = {s for c in T.CASES for s in c.symbols}
    assert set(SYMBOLS) <= set(stream_symbols()) and set(SYMBOLS) <= cased
    assert not set(stream_symbols()) - cased - set(T.EXCLUDED)
    pitches = {p for p in pitch_parameters() if p[0] in SYMBOLS}
    covered = {p for c in FT.CASES for p in c.covers}
    assert pitches == PITCHES and PITCHES <= covered
    assert not set(pitch_parameters()) - covered - set(FT.EXCLUDED)


def test_the_decoys_give_another_answer():
    for name in [n for p in PAIRS for n in p]:
        case = T.BY_NAME[name]
        want, other = T.refs(case, "real"), T.refs(case, "decoy")
        assert case.differs(want[0], other[0]) and T.nonempty(want), name
        out = T.flat(want[0])[-1]
        assert 0.05 < (out != 0).mean() < 0.95, name  # the output has both kinds of pixel
        if name.startswith("threshold"):
            assert int(want[0][0][0]) != int(other[0][0][0]) and 0 < int(want[0][0][0]) < 255, name
    for a, b in PAIRS:
        assert T.differs_any(T.refs(T.BY_NAME[a], "real"), T.refs(T.BY_NAME[b], "real"))
