"""Every image entry point on small views whose rows span 2 GiB and 4 GiB
(tests/_far.py's arena and protocol over tests/_far_table.py's cases).

include/tbdk.h ("image layout") takes any pitch >= a row; a pitch is an int, and
no entry point bounds pitch * height except the ones the header lists under
"Extents".  Each case runs under three layouts of its far images: `under_2g`
(the extent fits 31 bits, pitch * height does not), `over_2g` and `over_4g` (the
last 8 rows start at or beyond 2^31 / 2^32).  The result must equal the entry
point's oracle, bit for bit where its own test is, and no byte of the arena
outside the images may change.  A case with a documented bound runs twice under a
layout beyond it: at the largest accepted pitch (results equal the oracle) and at
the smallest rejected one (TBDK_EINVAL, every output and the arena untouched).

The arena (a 4 GiB guard below the images, 1 MiB above) keeps every address a
32-bit offset can wrap to inside one allocation, so a defect is a wrong result or
a changed poison byte; the two stand-in kernels at the end show both are seen.
DESIGN.md (test strategy, "Extents") has the audit and the measured wall time."""
import numpy as np
import pytest
import torch

import _far as F
import _far_table as FT
import _streams as ST
from test_gpu_dirty_state import options

pytestmark = pytest.mark.gpu

ran = set()


@pytest.fixture(scope="module", autouse=True)
def far_arena(gpu):
    F.arena()  # skips the module, with the figure, where the device has too little free memory
    yield
    F.release()


def torch_dtype(dt):
    return {"uint8": torch.uint8, "uint16": torch.uint16, "float16": torch.float16, "float32": torch.float32,
            "int32": torch.int32, "float64": torch.float64}[np.dtype(dt).name]


def rects_of(fc, i, layout, pitch=None, taken=()):
    imgs = fc.images(i)
    rects = F.place([(n, s[0], int(np.prod(s[1:])) * dt.itemsize, u) for n, s, dt, u in imgs], layout, pitches=fc.share,
                    taken=list(taken))
    if pitch is not None:
        rects = [F.with_pitch(r, pitch) for r in rects]
        assert F.separated(list(taken) + rects) and all(r.extent <= F.SPAN for r in rects)
    return {r.name: (r, s, dt) for r, (n, s, dt, u) in zip(rects, imgs)}


def run_far(gpu, fc, layout, pitch=None, expect_einval=False):
    """the protocol of tests/_far.py over every call of the case"""
    from opencv_amd import _lib

    base = fc.base
    ins, want = base.inputs("real"), FT.T.refs(base, "real")
    keep = set(base.keep)
    kept = {}  # name -> rect of an input that must outlive its call
    with options(gpu, dict(base.options, **fc.options), FT.OPTION_DEFAULTS):
        state = base.setup(gpu) if base.setup else None
        for i, inp in enumerate(ins):
            what = f"{fc.name}, {layout}{'' if pitch is None else f', pitch {pitch}'}, call {i}"
            placed = rects_of(fc, i, layout, pitch, taken=list(kept.values()))
            bufs = {k: ST.to_dev(v) for k, v in inp.items()}
            outs = {}
            for k, (shape, dt) in fc.outs_of(i).items():
                if k not in placed:
                    outs[k] = torch.empty(tuple(shape), dtype=torch_dtype(dt), device="cuda")
                    ST._poison(outs[k])
            for name, (r, shape, dt) in placed.items():
                v = F.view(r, shape, torch_dtype(dt))
                if name in bufs:
                    F.put(r, bufs[name])
                    bufs[name] = v
                else:
                    outs[name] = v
            torch.cuda.synchronize()
            rects = [r for r, _, _ in placed.values()]
            try:
                res = fc.run(gpu, state, bufs, outs, i) if fc.run else base.run(gpu, state, None, bufs, outs, i)
            except _lib.TbdkError as e:
                torch.cuda.synchronize()
                assert expect_einval and "EINVAL" in str(e), f"{what}: {e}"
                for name, (r, _, _) in placed.items():
                    if name in bufs:
                        F.poison(r)  # the inputs; a far output must still be all poison: the scan holds that
                for r in kept.values():
                    F.poison(r)
                F.scan(rects, f"{what} (rejected)")
                for k, o in outs.items():
                    if k not in placed:
                        assert bool((ST._bytes_of(o.reshape(-1)) == ST.POISON).all()), f"{what}: output {k} was written"
                return "rejected"
            torch.cuda.synchronize()
            assert not expect_einval, f"{what}: accepted, TBDK_EINVAL expected"
            got = ST.to_host(ST._map_tensors(res, lambda t: t.clone()))
            saved = {}
            for k in [k for k in kept if k[0] not in fc.hold]:
                F.poison(kept.pop(k))  # an input of the call before, which this call had to see unchanged
            for name, (r, _, _) in placed.items():
                if name in keep:
                    kept[name, i] = r
                else:
                    F.poison(r)
            for k, r in kept.items():
                saved[k] = F.get(r)
                F.poison(r)
            F.scan(rects + list(kept.values()), what)
            for k, r in kept.items():
                F.put(r, saved[k])
            base.check(got, want[i], what)
        torch.cuda.synchronize()
        del state
    for r in kept.values():
        F.poison(r)
    return "ran"


@pytest.mark.parametrize("layout", F.LAYOUTS)
@pytest.mark.parametrize("name", [c.name for c in FT.CASES])
def test_far(gpu, name, layout):
    fc = FT.BY_NAME[name]
    _, shape, dt, unit = next(im for i in range(fc.ncalls()) for im in fc.images(i))
    h, row = shape[0], int(np.prod(shape[1:])) * dt.itemsize
    nominal = F.pitch_of(layout, h, row, unit)
    if fc.bound is None or fc.bound.accepts(h, nominal, row):
        assert run_far(gpu, fc, layout) == "ran"
    else:
        last = fc.bound.last_accepted(h, row, unit)
        assert fc.bound.accepts(h, last, row) and not fc.bound.accepts(h, last + unit, row) and last + unit <= nominal
        assert run_far(gpu, fc, layout, pitch=last) == "ran"
        assert run_far(gpu, fc, layout, pitch=last + unit, expect_einval=True) == "rejected"
    ran.add((name, layout))


def test_every_case_ran():
    assert ran == {(c.name, lay) for c in FT.CASES for lay in F.LAYOUTS}


# ---- the harness sees a defect (stand-in kernels in torch; every address stays inside the arena) ---------------------

def _stand_in():
    img = np.random.default_rng(97040).integers(0, 256, (40, 97), dtype=np.uint8)
    (r,) = F.place([("src", 40, 97, 1)], "over_4g")
    assert (r.h - 1) * r.pitch >= 1 << 32
    return img, r


def test_harness_sees_rows_read_at_a_wrapped_offset():
    """a "kernel" that reads source row y at (y * pitch) mod 2^32: its last 8 rows are the image's first 8 again
    (8 pitches past 2^32 the offsets start over); the oracle comparison (here: the image itself) catches it"""
    img, r = _stand_in()
    F.put(r, torch.from_numpy(img).cuda())
    a = F.arena()
    got = torch.stack([a[F.LOW_GUARD + r.col + (y * r.pitch) % (1 << 32):][:r.row] for y in range(r.h)]).cpu().numpy()
    F.poison(r)
    F.scan([r], "stand-in reader")  # it wrote nothing
    assert np.array_equal(got[:r.h - F.EDGE_ROWS], img[:r.h - F.EDGE_ROWS])
    with pytest.raises(AssertionError, match="differs"):
        assert np.array_equal(got, img), "the copy differs from the source"


def test_harness_sees_a_row_written_2_32_bytes_low():
    """a "kernel" that writes a row 2^32 bytes below where it belongs (its first row: the others' wrapped places lie
    among the image's own rows, where the comparison sees them): inside the arena, in the low guard; the scan names the
    stray bytes by their offset from the image base, and leaves the arena clean"""
    img, r = _stand_in()
    a = F.arena()
    low = F.LOW_GUARD + r.col - (1 << 32)
    assert 0 <= low < F.LOW_GUARD - r.row
    a[low:low + r.row].copy_(torch.from_numpy(img[0]).cuda())
    stray = int((img[0] != F.POISON).sum())
    with pytest.raises(AssertionError, match=rf"{stray} byte\(s\) outside every image changed.*mod 2\^32"):
        F.scan([r], "stand-in writer")
    F.scan([r], "after the failed scan")  # all poison again
