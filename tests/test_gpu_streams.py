"""Every entry point on a side stream behind a late producer (tests/_streams.py's
protocol over tests/_streams_table.py's cases).

Ordering: each case runs with its inputs produced on the stream behind a ~50 ms
spin, every library call carries stream=S, the outputs are consumed on S with no
host synchronisation in between, and the existing oracle comparison of the entry
point runs on what the consumer saw, bit for bit.  Pairs queue two different
calls of one entry point behind one spin; the frames of MOG2 and of the KLT
tracker are also queued behind one spin, with nothing between the frames.
Asynchrony: every call the header does not document as synchronising, every call
of a sequence included, must return while a ~200 ms spin still blocks the stream;
the file ends by asserting that symbol by symbol against the header.  The three
harness self-tests show that a violation is seen.

DESIGN.md (test strategy, "Streams") has the per-entry-point audit."""
import pytest
import torch

import _streams as ST
import _streams_table as T
from test_gpu_dirty_state import DEFAULTS, options

pytestmark = pytest.mark.gpu

ran = {"ordering": set(), "pairs": set(), "asynchrony": set(), "sequences": set()}
returned_early = set()  # the symbols reached by a call that passed the asynchrony check


def jobs_of(gpu, case, state):
    """one job per call of the case, every call of it"""
    real, decoy, want = case.inputs("real"), case.inputs("decoy"), T.refs(case, "real")
    for i in range(len(real)):
        yield ST.Job(real[i], decoy[i],
                     call=lambda S, b, o, i=i: case.run(gpu, state, S, b, o, i),
                     check=lambda got, what, i=i: case.check(got, want[i], what),
                     outs=case.outs(i) if case.outs else {}, keep=tuple(case.keep), poison_results=case.poison,
                     prefill=(lambda: case.prefill(state)) if case.prefill else None)


def run_case(gpu, case, spin_ms, expect_async=False, record=None):
    ST.side_stream()  # after the context (the gpu fixture), as tbdk.h's note on side streams asks
    with options(gpu, case.options, DEFAULTS):
        state = case.setup(gpu) if case.setup else None
        for i, job in enumerate(jobs_of(gpu, case, state)):
            ST.late(job, spin_ms, expect_async, f"{case.name}, call {i}")
            if record is not None:
                record.update(case.symbols_of(i))
        ST.side_stream().synchronize()
        del state


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_ordering(gpu, name):
    run_case(gpu, T.BY_NAME[name], ST.ORDER_MS)
    ran["ordering"].add(name)


@pytest.mark.parametrize("pair", T.PAIRS, ids=lambda p: "+".join(p))
def test_pair_behind_one_spin(gpu, pair):
    """two different calls of one entry point queued behind one spin: what the second call's
    host code does to a context-owned table or scratch must not reach the first call's kernels"""
    a, b = (T.BY_NAME[n] for n in pair)
    ST.side_stream()
    with options(gpu, dict(a.options, **b.options), DEFAULTS):
        sa, sb = (c.setup(gpu) if c.setup else None for c in (a, b))
        ja, jb = list(jobs_of(gpu, a, sa)), list(jobs_of(gpu, b, sb))
        for i in range(max(len(ja), len(jb))):
            ST.late([j[i] for j in (ja, jb) if i < len(j)], ST.ORDER_MS, False, f"{a.name} then {b.name}, step {i}")
        ST.side_stream().synchronize()
        del sa, sb
    ran["pairs"].add(pair)


ASYNC = [c.name for c in T.CASES if c.sync is None]


@pytest.mark.parametrize("name", ASYNC)
def test_asynchrony(gpu, name):
    """the call returns while the stream is still blocked.  A warm-up run first: scratch growth
    and lazy stream or table creation may legitimately block"""
    case = T.BY_NAME[name]
    run_case(gpu, case, 1.0)
    reached = set()
    run_case(gpu, case, ST.ASYNC_MS, expect_async=True, record=reached)  # every call of the case, each behind its spin
    assert reached == set(case.symbols), f"{name}: the asynchrony run never called {sorted(set(case.symbols) - reached)}"
    returned_early.update(reached)
    ran["asynchrony"].add(name)


SEQUENCES = T.SEQUENCES


@pytest.mark.parametrize("name", SEQUENCES)
def test_sequence_behind_one_spin(gpu, name):
    """the frames of one object (MOG2, the KLT tracker) queued behind ONE spin, every frame produced late and
    consumed on the stream: no synchronisation of any kind sits between frame f and frame f + 1, so an edge
    missing between two frames shows.  (Sequences whose calls synchronise, the loops, cannot be queued so.)"""
    case = T.BY_NAME[name]
    ST.side_stream()
    with options(gpu, case.options, DEFAULTS):
        state = case.setup(gpu) if case.setup else None
        ST.late(list(jobs_of(gpu, case, state)), ST.ORDER_MS, False, f"{name}, all frames behind one spin", sequence=True)
        ST.side_stream().synchronize()
        del state
    ran["sequences"].add(name)


def test_every_case_ran():
    assert ran["ordering"] == {c.name for c in T.CASES} and len(ran["ordering"]) == len(T.CASES)
    assert len(ran["pairs"]) == len(T.PAIRS)
    assert ran["asynchrony"] == set(ASYNC) and len(ASYNC) == len([c for c in T.CASES if c.sync is None])
    assert ran["sequences"] == set(SEQUENCES) and len(SEQUENCES) >= 3
    # symbol by symbol: every stream-taking entry point of the header was reached by a call that returned while
    # the stream was blocked, unless it is excluded or every case that reaches it cites the line that documents
    # it as synchronising
    from test_streams_cases import stream_symbols

    documented = {s for c in T.CASES if c.sync is not None for s in c.symbols} - \
        {s for c in T.CASES if c.sync is None for s in c.symbols}
    need = set(stream_symbols()) - set(T.EXCLUDED) - documented
    assert need <= returned_early, f"no asynchrony check reached {sorted(need - returned_early)}"
    assert len(need) >= 35


# ---- the harness sees a violation (torch only; data races on benign buffers, nothing faults) -----------------

def _stand_in(call):
    import numpy as np

    real = {"inp": np.arange(4096, dtype=np.float32)}
    decoy = {"inp": -real["inp"] - 1}

    def check(got, what):
        assert np.array_equal(got[0], real["inp"]), f"{what}: the consumer saw other data than the real input's copy"

    return ST.Job(real, decoy, call, check, outs={"out": ((4096,), torch.float32)})


def test_harness_sees_a_call_on_another_stream():
    other = torch.cuda.Stream()

    def call(S, b, o):
        with torch.cuda.stream(other):  # not ordered behind S: reads the decoy while S still spins
            o["out"].copy_(b["inp"])
        return (o["out"],)

    with pytest.raises(AssertionError, match="the consumer saw other data"):
        ST.late(_stand_in(call), ST.ORDER_MS, False, "stand-in on a second stream")
    other.synchronize()


def test_harness_sees_a_call_that_waits_for_the_stream():
    def call(S, b, o):
        o["out"].copy_(b["inp"])
        S.synchronize()
        return (o["out"],)

    with pytest.raises(AssertionError, match="the call waited for the stream"):
        ST.late(_stand_in(call), ST.ASYNC_MS, True, "stand-in that synchronises")


def test_harness_passes_a_call_on_the_stream():
    def call(S, b, o):
        o["out"].copy_(b["inp"])
        return (o["out"],)

    assert ST.late(_stand_in(call), ST.ORDER_MS, False, "stand-in on the stream")
    assert ST.late(_stand_in(call), ST.ASYNC_MS, True, "stand-in on the stream")
