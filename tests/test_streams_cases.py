"""The conditions of tests/test_gpu_streams.py's case table, from the oracle alone (no GPU).

A case proves nothing if the decoy gives the same answer as the real inputs: a
call that read its inputs too early would still pass.  So for every case, and
every call of it: oracle(decoy) != oracle(real) in the compared outputs (corner
lists differ, flows differ in at least 1 % of the pixels, masks differ, tracks
differ); the real case is active (non-empty corner / hit / track sets); the two
cases of a pair give different results.  And the table names every `tbdk_*`
symbol of include/tbdk.h that takes a `void* stream`, so that a new entry point
cannot arrive without a case."""
import os
import re

import pytest

import _streams_table as T

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tbdk.h")


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_decoy_gives_another_answer_and_the_case_is_active(name):
    case = T.BY_NAME[name]
    real, decoy = case.inputs("real"), case.inputs("decoy")
    assert len(real) == len(decoy) > 0
    for r, d in zip(real, decoy):
        assert r.keys() == d.keys()
        for k in r:
            assert r[k].shape == d[k].shape and r[k].dtype == d[k].dtype, (name, k)
    want, other = T.refs(case, "real"), T.refs(case, "decoy")
    assert len(want) == len(other) == len(real)
    for i, (a, b) in enumerate(zip(want, other)):
        assert case.differs(a, b), f"{name}, call {i}: the decoy's result equals the real inputs'"
    assert (case.active or T.nonempty)(want), f"{name}: the oracle finds nothing on the real inputs"
    assert set(case.keep) <= set(real[0]), name
    assert case.symbols and all(s.startswith("tbdk_") for s in case.symbols)
    reached = {s for i in range(len(real)) for s in case.symbols_of(i)}
    assert reached == set(case.symbols), f"{name}: no call reaches {sorted(set(case.symbols) - reached)}"


@pytest.mark.parametrize("pair", T.PAIRS, ids=lambda p: "+".join(p))
def test_pair_results_differ(pair):
    a, b = (T.BY_NAME[n] for n in pair)
    assert a.name != b.name and set(a.symbols) & set(b.symbols), pair
    ra, rb = T.refs(a, "real"), T.refs(b, "real")
    assert T.differs_any(ra, rb), f"{pair}: the two calls give the same result"
    # other inputs and another size
    ia, ib = a.inputs("real")[0], b.inputs("real")[0]
    assert any(ia[k].shape != ib[k].shape for k in ia if k in ib) or T.differs_any(list(ia.values()), list(ib.values()))


def stream_symbols():
    """every function of the header with a `void* stream` parameter"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = []
    for m in re.finditer(r"\bint\s+(tbdk_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_every_stream_taking_symbol_is_in_the_table():
    syms = stream_symbols()
    assert len(syms) >= 50 and "tbdk_pyr_build" in syms and "tbdk_mog2_apply" in syms and "tbdk_ctx_create" not in syms
    cased = {s for c in T.CASES for s in c.symbols}
    named = cased | set(T.EXCLUDED)
    assert not set(syms) - named, f"stream-taking entry points with neither a case nor an exclusion: {sorted(set(syms) - named)}"
    assert not named - set(syms), f"the table names symbols the header does not have: {sorted(named - set(syms))}"
    assert not cased & set(T.EXCLUDED), "a symbol is both a case and an exclusion"
    assert all(len(r) > 20 for r in T.EXCLUDED.values()), "an exclusion needs its reason"


def test_synchronising_cases_cite_their_line():
    for c in T.CASES:
        if c.sync is not None:
            assert "\"" in c.sync and ("tbdk.h" in c.sync or "opencv_amd/" in c.sync), c.name
        for line in c.keep.values():
            assert "tbdk.h" in line and "\"" in line, c.name
    # what the header quotes say is in the header
    text = " ".join(re.sub(r"^\s*/?\*+/?", "", ln).strip() for ln in open(HEADER).read().splitlines())
    for c in T.CASES:
        for line in [c.sync] * (c.sync is not None and c.sync.startswith("tbdk.h")) + list(c.keep.values()):
            quotes = re.findall(r"\"(.*?)\"", line)
            assert quotes, (c.name, line)
            for quote in quotes:
                assert re.sub(r"\s+", " ", quote) in re.sub(r"\s+", " ", text), (c.name, quote)
