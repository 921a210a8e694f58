"""The side-stream and far-view cases of tbdk_knn_apply, tbdk_knn_get_background and tbdk_knn_get_model, registered
with tests/_streams_table.py and tests/_far_table.py.

tests/test_streams_cases.py requires a case (or an exclusion) in the streams table for every entry point of
include/tbdk.h that takes a `void* stream`, tests/test_far_cases.py one in the far table for every `*pitch`
parameter; tests/test_gpu_streams.py and tests/test_gpu_far_views.py run every case of them.  This module adds the
three new entry points' cases through the tables' own add() when it is imported.  pytest imports every test module
of a run before it runs a test, and this file sorts before those four, so in a run of the suite their
parametrisation and their symbol-by-symbol checks see these cases like any other.  (A run of one of those files on
its own does not import this module and reports the new symbols as uncovered: run them with the suite, or name
this file too.)

A case is six frames through one subtractor: every frame's mask, and after the last the background image, the
model, the counters and the RNG state.  At the automatic rate the short and mid periods are 1 in these frames, so
every frame is followed by fills, whose order on the stream the final RNG state and the next-update planes show.
The decoy is the same sequence twenty frames later.

The CPU tests below hold what the registration must give: the cases are in the tables once, every new
stream-taking symbol and pitch parameter of the header has one, and the decoy inputs give another answer than the
real ones."""
import numpy as np

import _far_table as FT
import _knn_cases as KC
import _knn_oracle as KO
import _streams_table as T
from test_gpu_extreme import same_bits

KNN_FRAMES = 6
SIZES = {"knn_8UC3_130x121": (130, 121, 3), "knn_8UC1_300x5": (300, 5, 1)}
SYMBOLS = ("tbdk_knn_apply", "tbdk_knn_get_background", "tbdk_knn_get_model")
PAIRS = [("knn_8UC1_300x5", "knn_8UC3_130x121")]
FAR_BASE = "knn_8UC3_130x121"  # the far arena wants at least 32 rows
PITCHES = {("tbdk_knn_apply", "pitch"), ("tbdk_knn_apply", "mask_pitch"), ("tbdk_knn_get_background", "pitch")}
PARAMS = dict(KC.DEFAULTS, rng_state=KC.SECOND_SEED)


def _case(name):
    w, h, cn = SIZES[name]
    return dict(name=name, w=w, h=h, cn=cn, n=KNN_FRAMES, rates=np.full(KNN_FRAMES, -1.0), bg=(KNN_FRAMES,))


def _inputs(name):
    def inputs(which):
        w, h, cn = SIZES[name]
        fr = KC.GC.frames(w, h, 20 + KNN_FRAMES, cn)
        sel = range(KNN_FRAMES) if which == "real" else range(20, 20 + KNN_FRAMES)  # the decoy: later frames
        return [{"frame": np.ascontiguousarray(fr[t])} for t in sel]

    return inputs


def _oracle(name):
    def f(ins):
        masks, bgs, m = KO.run_case(_case(name), PARAMS, [i["frame"] for i in ins])
        out = [{"mask": masks[t]} for t in range(KNN_FRAMES)]
        s, i, n, c, state = m.model()
        out[-1].update(bg=bgs[KNN_FRAMES], model=(s, i, n, c, np.array([state], np.uint64).view(np.int64)))
        return out

    return f


def _setup(name):
    def setup(ctx):
        from test_gpu_knn import subtractor

        return subtractor(PARAMS, ctx)

    return setup


def _run(ctx, m, S, b, o, i):
    out = {"mask": m.apply(b["frame"], o["mask"], -1.0, stream=S)}
    if i == KNN_FRAMES - 1:
        out.update(bg=m.getBackgroundImage(stream=S), model=m.model(stream=S))
    return out


def _check(g, ref, what):
    same_bits(g["mask"], ref["mask"], f"{what}: mask")
    if "bg" in ref:
        same_bits(g["bg"], ref["bg"], f"{what}: background image")
        for name, x, y in zip(("samples", "index", "next", "counters", "rng state"), g["model"], ref["model"]):
            same_bits(x, y, f"{what}: model {name}")


def _active(name):
    """some mask has background and foreground, fills were made, and every single frame matters: the first
    frame's mask does not depend on its pixels (the model is empty), so a frame read too early shows in what is
    compared later; with frame t alone replaced by the decoy's, a later mask or the final model differs"""
    def active(r):
        real, decoy = _inputs(name)("real"), _inputs(name)("decoy")
        for t in range(KNN_FRAMES):
            mixed = _oracle(name)(real[:t] + [decoy[t]] + real[t + 1:])
            if not T.differs_any(mixed[t:], r[t:]):
                return False
        state = int(r[-1]["model"][4].view(np.uint64)[0])
        return state != PARAMS["rng_state"] and r[-1]["model"][2].any() and \
            any(0 < (x["mask"] == 0).mean() < 1 for x in r[1:])

    return active


def _far_background(ctx, m, b, o, i):
    out = {"mask": m.apply(b["frame"], o["mask"], -1.0)}
    if i == KNN_FRAMES - 1:
        out.update(bg=m.getBackgroundImage(o["bg"]), model=m.model())
    return out


def _far_outs(i):
    w, h, cn = SIZES[FAR_BASE]
    o = {"mask": ((h, w), "uint8")}
    if i == KNN_FRAMES - 1:
        o["bg"] = ((h, w, cn), "uint8")
    return o


def register():
    """adds the cases once, however often this module is imported or reloaded"""
    if FAR_BASE in T.BY_NAME:
        return
    for name, (w, h, cn) in SIZES.items():
        T.add(T.Case(name, SYMBOLS, _inputs(name), _oracle(name), _run, _check, setup=_setup(name), active=_active(name),
                     called=lambda i: SYMBOLS[:1] + (SYMBOLS[1:] if i == KNN_FRAMES - 1 else ()),
                     differs=lambda a, b: "bg" not in a or T.differs_any(a, b),  # per frame: see _active
                     outs=lambda i, w=w, h=h: {"mask": ((h, w), "uint8")}))
    T.BY_NAME.update({c.name: c for c in T.CASES})
    T.PAIRS.extend(PAIRS)
    T.SEQUENCES.append(FAR_BASE)  # its frames also queued behind one spin, as MOG2's are
    FT.add(f"{FAR_BASE}_frame", FAR_BASE, ("frame",), ("tbdk_knn_apply", "pitch"))
    FT.add(f"{FAR_BASE}_mask", FAR_BASE, ("mask",), ("tbdk_knn_apply", "mask_pitch"))
    FT.add(f"{FAR_BASE}_background", FAR_BASE, ("bg",), ("tbdk_knn_get_background", "pitch"), run=_far_background,
           outs=_far_outs)
    FT.BY_NAME.update({c.name: c for c in FT.CASES})


register()


def test_the_cases_are_in_the_tables_once():
    names, far = [c.name for c in T.CASES], [c.name for c in FT.CASES]
    for name in SIZES:
        assert names.count(name) == 1 and T.BY_NAME[name].sync is None, name  # asynchronous: both checks run
    assert all(T.PAIRS.count(p) == 1 for p in PAIRS) and T.SEQUENCES.count(FAR_BASE) == 1
    assert sum(n.startswith(FAR_BASE) for n in far) == 3
    register()
    assert [c.name for c in T.CASES] == names and [c.name for c in FT.CASES] == far
    assert all(FT.BY_NAME[n].base is T.BY_NAME[FAR_BASE] for n in far if n.startswith(FAR_BASE))


def test_every_new_symbol_and_pitch_parameter_has_a_case():
    from test_far_cases import pitch_parameters
    from test_streams_cases import stream_symbols

    cased = {s for c in T.CASES for s in c.symbols}
    assert set(SYMBOLS) <= set(stream_symbols()) and set(SYMBOLS) <= cased
    assert not set(stream_symbols()) - cased - set(T.EXCLUDED)
    pitches = {p for p in pitch_parameters() if p[0].startswith("tbdk_knn_")}
    covered = {p for c in FT.CASES for p in c.covers}
    assert pitches == PITCHES and PITCHES <= covered
    assert not set(pitch_parameters()) - covered - set(FT.EXCLUDED)


def test_the_decoys_give_another_answer():
    for name in SIZES:
        case = T.BY_NAME[name]
        real, decoy = case.inputs("real"), case.inputs("decoy")
        assert all(not np.array_equal(r["frame"], d["frame"]) for r, d in zip(real, decoy)), name
        want, other = T.refs(case, "real"), T.refs(case, "decoy")
        assert all(case.differs(a, b) for a, b in zip(want, other)) and T.differs_any(want[1:], other[1:]), name
        assert case.active(want), name
    for a, b in PAIRS:
        assert T.differs_any(T.refs(T.BY_NAME[a], "real"), T.refs(T.BY_NAME[b], "real"))
