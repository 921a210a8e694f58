"""The side-stream cases of tbdk_morph_u8 and tbdk_connected_components, registered with tests/_streams_table.py.

tests/test_streams_cases.py requires a case (or an exclusion) in that table for every entry point of include/tbdk.h
that takes a `void* stream`, and tests/test_gpu_streams.py runs every case of it behind a late producer: ordering,
pairs behind one spin, and the return while the stream is still blocked.  This module adds the two new entry
points' cases through the table's own add() when it is imported.  pytest imports every test module of a run before
it runs a test, and this file sorts before both of those, so in a run of the suite their parametrisation and
their symbol-by-symbol checks see these cases like any other.  (A run of one of those two files on its own does not
import this module and reports the two symbols as uncovered: run them with the suite, or name this file too.)

The CPU tests below hold what the registration must give: the cases are in the table once, every new stream-taking
symbol of the header has one, and the decoy inputs give another answer than the real ones."""
import numpy as np

import _cc_oracle as CCO
import _morph_cases as BC
import _morph_oracle as MPO
import _streams_table as T
from _streams import POISON
from test_gpu_extreme import same_bits

CC_CAP = 512
SIZES = ((130, 121), (300, 5))
SYMBOLS = ("tbdk_morph_u8", "tbdk_connected_components")
PAIRS = [("morph_open_300x5", "morph_open_130x121"), ("connected_components_300x5", "connected_components_130x121")]


def _imgproc():
    from opencv_amd import imgproc

    return imgproc


def _cc_run(ctx, st, S, b, o, i):
    return _imgproc().connected_components_with_stats(b["src"], o["labels"], o["stats"], o["cent"], 8, -1, CC_CAP,
                                                      ctx=ctx, stream=S)


def _cc_check(g, ref, what):
    n, labels, stats, cent = ref
    assert 2 < n <= CC_CAP and int(g[0][0]) == n, (what, int(g[0][0]), n)
    same_bits(g[1], labels, f"{what}: labels")
    same_bits(g[2][:n], stats, f"{what}: stats")
    assert CCO.same_centroids(g[3][:n], cent), f"{what}: centroids"
    assert (g[2][n:].view(np.uint8) == POISON).all() and (g[3][n:].view(np.uint8) == POISON).all(), \
        f"{what}: rows from N on were written"


def register():
    """adds the cases once, however often this module is imported or reloaded"""
    if "morph_open_130x121" in T.BY_NAME:
        return
    for sz in SIZES:
        T.add(T.Case(f"morph_open_{sz[0]}x{sz[1]}", ("tbdk_morph_u8",),
                     T.one(lambda s=sz: {"src": BC.image(s[0], s[1], "mask")}),
                     T.single(lambda i: MPO.morphology_ex(i["src"], MPO.OPEN, BC.elements()["ellipse5x5"])),
                     lambda ctx, st, S, b, o, i: _imgproc().morphology_ex(b["src"], MPO.OPEN,
                                                                         BC.elements()["ellipse5x5"], dst=o["dst"],
                                                                         ctx=ctx, stream=S),
                     outs=lambda i, s=sz: {"dst": ((s[1], s[0]), "uint8")}))
        T.add(T.Case(f"connected_components_{sz[0]}x{sz[1]}", ("tbdk_connected_components",),
                     T.one(lambda s=sz: {"src": BC.image(s[0], s[1], "mask")}),
                     T.single(lambda i: CCO.connected_components_with_stats(i["src"], 8, -1)), _cc_run, _cc_check,
                     outs=lambda i, s=sz: {"labels": ((s[1], s[0]), "int32"), "stats": ((CC_CAP, 5), "int32"),
                                           "cent": ((CC_CAP, 2), "float64")}))
    T.BY_NAME.update({c.name: c for c in T.CASES})
    T.PAIRS.extend(PAIRS)


register()


def test_the_cases_are_in_the_table_once():
    names = [c.name for c in T.CASES]
    for sz in SIZES:
        for stem in ("morph_open", "connected_components"):
            name = f"{stem}_{sz[0]}x{sz[1]}"
            assert names.count(name) == 1 and T.BY_NAME[name].sync is None, name  # asynchronous: both checks run
    assert all(T.PAIRS.count(p) == 1 for p in PAIRS)
    register()
    assert [c.name for c in T.CASES] == names


def test_every_new_stream_taking_symbol_has_a_case():
    from test_streams_cases import stream_symbols

    cased = {s for c in T.CASES for s in c.symbols}
    assert set(SYMBOLS) <= set(stream_symbols()) and set(SYMBOLS) <= cased
    assert not set(stream_symbols()) - cased - set(T.EXCLUDED)


def test_the_decoys_give_another_answer():
    for name in [n for p in PAIRS for n in p]:
        case = T.BY_NAME[name]
        want, other = T.refs(case, "real"), T.refs(case, "decoy")
        assert case.differs(want[0], other[0]) and T.nonempty(want), name
        if "connected" in name:
            assert 2 < want[0][0] <= CC_CAP, name
    for a, b in PAIRS:
        assert T.differs_any(T.refs(T.BY_NAME[a], "real"), T.refs(T.BY_NAME[b], "real"))
