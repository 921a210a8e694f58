"""Every entry point on a side stream behind a late producer: the harness.

The library's contract (include/tbdk.h, top): "every call is asynchronous on the
given HIP stream ... no hidden host sync".  The rest of the suite calls on the
legacy default stream with inputs that were complete long before the call; there
a kernel launched on stream 0 instead of `s`, a blocking copy that was meant to
go on the stream, or a side stream without its fork edge all read the right data
anyway.  `late` creates the one calling condition that shows them.

Protocol, on a torch.cuda.Stream() S (torch creates it non-blocking; it is
created after the context, as tbdk.h's note on side streams asks):

  1. the input buffers hold a DECOY, the real inputs wait in separate device
     tensors, caller-owned output buffers hold a poison byte; one
     torch.cuda.synchronize(), here only;
  2. on S: torch.cuda._sleep(cycles), an event `gate`, then the real inputs are
     copied device-to-device over the decoy;
  3. the library call with stream=S, from the host, while the spin still runs;
  4. still on S and with no host synchronisation, every output is cloned (the
     consumer), then the decoy is written back over the inputs and the poison
     over the outputs: a kernel the library deferred past the end of its call
     reads the decoy or loses its output.  A buffer the header says must outlive
     the call (`keep`) is not overwritten;
  5. S.synchronize() -- not a device synchronise -- and the checker runs on the
     clones.

By construction this catches any read of an input on a stream not ordered behind
S (the null stream, a blocking copy, a side stream without its fork edge) and any
host read of device results before S got there.  It probably also catches a side
stream not joined back into S, whose work starts only after the spin; that is
not guaranteed: with few hardware queues streams share one and can be ordered by
accident.  No queue setting is touched here.

Pairs: several jobs queued behind one spin catch a context-owned table or
scratch that the second call's host code rewrites while the first call's kernels
still wait behind the spin.

Sequences (sequence=True): the frames of one object whose calls do not
synchronise (MOG2, the KLT tracker) queued behind one spin, each frame produced
late and its outputs consumed, then overwritten, before the next call: run frame
by frame the protocol drains the device between two frames (step 1), which would
hide an edge missing across frames.

Library-owned outputs (a pyramid's storage) are poisoned in step 1 too
(Job.prefill), so a recycled allocation cannot show an earlier run's answer.

Asynchrony (expect_async): right after the calls return, `gate` must not have
completed: the call came back while the stream was still blocked, so it waited
for nothing.  Only for calls the header does not document as synchronising, and
after a warm-up run (scratch growth and lazy creation may block).

The spin is a bounded cycle count: nothing here waits on an event that was not
recorded, loops on query() or retries."""
from dataclasses import dataclass, field

import numpy as np

ORDER_MS = 50.0    # ordering cases: a misplaced kernel of these sizes runs in microseconds
ASYNC_MS = 200.0   # asynchrony cases: three orders of magnitude above a whole frame of the loop (0.163 ms)
CALIBRATION_CYCLES = 20_000_000
POISON = 0xA5

_cal = {}


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, measured once per session with a
    pair of torch events (the device against itself)"""
    import torch

    if "cpm" not in _cal:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # the first launch pays the module load
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(CALIBRATION_CYCLES)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0
        _cal["cpm"] = CALIBRATION_CYCLES / ms
        print(f"streams: torch.cuda._sleep runs {_cal['cpm']:.0f} cycles per ms "
              f"({CALIBRATION_CYCLES} cycles took {ms:.2f} ms)")
    return _cal["cpm"]


def side_stream():
    """one non-blocking stream per session, created after the context"""
    import torch

    if "S" not in _cal:
        _cal["S"] = torch.cuda.Stream()
    return _cal["S"]


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:  # torch has no uint16 arithmetic; the kernels only take the pointer
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def to_host(v):
    """a clone (or a nest of them) as numpy; host values pass through"""
    import torch

    if isinstance(v, torch.Tensor):
        if v.dtype == torch.uint16:
            return v.view(torch.int16).cpu().numpy().view(np.uint16)
        return v.cpu().numpy()
    if isinstance(v, (tuple, list)):
        return type(v)(to_host(x) for x in v)
    if isinstance(v, dict):
        return {k: to_host(x) for k, x in v.items()}
    return v


def _bytes_of(t):
    import torch

    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def _poison(t):
    """the poison byte over a device tensor, on the current stream"""
    if t.numel() == 0:
        return
    if t.is_contiguous() and (t.dim() == 0 or t.stride(-1) == 1):
        _bytes_of(t.reshape(-1)).fill_(POISON)
    else:  # a strided view (a field of a record, a permuted plane): any other value will do
        t.zero_()


def _map_tensors(v, fn):
    import torch

    if isinstance(v, torch.Tensor):
        return fn(v)
    if isinstance(v, (tuple, list)):
        return type(v)(_map_tensors(x, fn) for x in v)
    if isinstance(v, dict):
        return {k: _map_tensors(x, fn) for k, x in v.items()}
    return v


@dataclass
class Job:
    """one library call of the protocol
    real, decoy  {name: numpy array}, the same names, shapes and types
    call         (S, bufs, outs) -> the outputs: device tensors (in any nest of tuples / lists /
                 dicts) and host values; bufs: {name: device tensor} of the inputs, outs:
                 {name: device tensor} of the caller-owned outputs (poisoned)
    check        (outputs as numpy, what) raises AssertionError
    outs         {name: (shape, torch dtype)} caller-owned output buffers
    keep         names of inputs that must outlive the call (not overwritten in step 4)"""
    real: dict
    decoy: dict
    call: object
    check: object
    outs: dict = field(default_factory=dict)
    keep: tuple = ()
    poison_results: bool = True  # False: the call returns views of memory the library (or an input) owns
    prefill: object = None       # () -> None, in step 1: poisons library-owned output memory (pyramid storage)


def late(jobs, spin_ms=ORDER_MS, expect_async=False, what="", sequence=False):
    """the protocol of the module docstring over one job or several behind one spin (a pair, or with
    `sequence` the frames of one object: every frame produced late, no synchronisation of any kind
    between the frames); raises AssertionError when a checker does, or (expect_async) when a call
    waited for the stream"""
    import torch

    if isinstance(jobs, Job):
        jobs = [jobs]
    S = side_stream()
    cycles = int(cycles_per_ms() * spin_ms)
    state = []
    for j in jobs:
        assert j.real.keys() == j.decoy.keys()
        for k in j.real:
            assert j.real[k].shape == j.decoy[k].shape and j.real[k].dtype == j.decoy[k].dtype, k
        decoy = {k: to_dev(v) for k, v in j.decoy.items()}
        bufs = {k: v.clone() for k, v in decoy.items()}
        staged = {k: to_dev(v) for k, v in j.real.items()}
        outs = {k: torch.empty(shape, dtype=getattr(torch, dt) if isinstance(dt, str) else dt, device="cuda")
                for k, (shape, dt) in j.outs.items()}
        for o in outs.values():
            _poison(o)
        if j.prefill is not None:
            j.prefill()
        state.append((decoy, bufs, staged, outs))
    torch.cuda.synchronize()  # step 1; the only device-wide synchronise
    gate = torch.cuda.Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        gate.record(S)
        for _, bufs, staged, _ in state:
            for k in bufs:
                bufs[k].copy_(staged[k], non_blocking=True)
        def consume(res):
            return _map_tensors(res, lambda t: t.clone())

        def write_back(j, decoy, bufs, outs, res):
            for k in bufs:
                if k not in j.keep:
                    bufs[k].copy_(decoy[k], non_blocking=True)
            if j.poison_results:
                _map_tensors(res, _poison)
            for o in outs.values():
                _poison(o)

        if sequence:  # the frames of one object: call f's outputs are consumed before call f + 1 replaces them
            clones = []
            for j, (decoy, bufs, _, outs) in zip(jobs, state):
                res = j.call(S, bufs, outs)
                clones.append(consume(res))
                write_back(j, decoy, bufs, outs, res)
            returned_early = not gate.query()
        else:
            results = [j.call(S, bufs, outs) for j, (_, bufs, _, outs) in zip(jobs, state)]
            returned_early = not gate.query()
            clones = [consume(res) for res in results]
            for j, (decoy, bufs, _, outs), res in zip(jobs, state, results):
                write_back(j, decoy, bufs, outs, res)
    S.synchronize()
    for i, (j, c) in enumerate(zip(jobs, clones)):
        j.check(to_host(c), f"{what}{f', call {i}' if len(jobs) > 1 else ''} (side stream, inputs produced late)")
    if expect_async:
        assert returned_early, (f"{what}: the stream's earlier work ({spin_ms:.0f} ms) had finished when the call "
                                "returned: the call waited for the stream")
    return returned_early
