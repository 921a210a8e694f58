"""The forward-backward check composed from the oracle alone (tests/_fb_oracle.py)
on the inputs of the GPU tests: no GPU.  A GPU test of the check must not pass
by having nothing to reject, so on every sequence and configuration those tests
use the oracle shows at least one point of each kind -- lost by the forward
pass, lost on the way back, and tracked back too far from its start -- and the
checked loop's predictions differ from the plain loop's by more than 0.01 px.

Measured from the oracle (forward lost / backward lost / too far):
  loop, 640x480, 16 objects, 8 frames, seed 20261022 at 1.0 px: 12 / 2 / 302 of
  28,075 points entering (largest prediction change 0.50 px); window 9: 52 / 6 /
  525; window 5, max_level 1: 65 / 17 / 640 (4.2 px); max_level 0: 11 / 2 / 307;
  max_tracks 10: 9 / 1 / 287; seed 20261023 at 0.25 px: 2 / 2 / 836 of 27,211.
  standalone, 616 points, frames 0 and 3 of 320x240: (21, 2) 3 / 2 / 66 at 1.0 px
  and 3 / 2 / 149 at 0.25 px; (5, 1) 19 / 21 / 197 and 19 / 21 / 214."""
import numpy as np
import pytest

import _fb_oracle as F

O = F.O


@pytest.mark.parametrize("win,max_level", F.LK_CASES)
def test_standalone_inputs_have_every_kind(win, max_level):
    assert len(F.lk_inputs()[2]) == 616
    for thr in F.LK_THRS:
        fl, bl, far, kept = F.kinds(F.lk_reference(win, max_level, thr))
        print(f"win {win} levels {max_level} thr {thr}: {fl} forward lost, {bl} backward lost, {far} too far, {kept} kept")
        assert fl >= 1 and bl >= 1 and far >= 1 and kept >= 100


def test_outputs_where_undefined():
    c = F.lk_reference(21, 2, 1.0)
    pts = F.lk_inputs()[2]
    lost = c.fwd_status == 0
    assert np.array_equal(c.back_pts[lost], pts[lost]) and np.all(np.isinf(c.fb_err[lost]))
    assert np.all(np.isinf(c.fb_err[(c.fwd_status == 1) & (c.back_status == 0)]))
    both = (c.fwd_status == 1) & (c.back_status == 1)
    assert np.all(np.isfinite(c.fb_err[both]))
    assert np.array_equal(c.status == 1, both & (c.fb_err < np.float32(1.0)))


def test_infinite_threshold_is_the_status_rule():
    """thr = +inf: only the two statuses gate; where no point is lost on the way
    back the result is the plain forward pass's"""
    Pa, Pb = F.lk_pyramids(21, 2)
    pts = F.lk_inputs()[2]
    c = F.checked_trace(Pa, Pb, pts, 21, 2, F.LK_ITERS, F.LK_EPS, F.LK_MIN_EIG, np.inf, O.ACCUM_EXACT)
    nxt, st, err, it = O.lk(Pa, Pb, pts, (21, 21), 2, F.LK_ITERS, F.LK_EPS, 0, F.LK_MIN_EIG, O.ACCUM_EXACT)
    assert np.array_equal(c.next_pts, nxt) and np.array_equal(c.err, err) and np.array_equal(c.iters, it)
    assert np.array_equal(c.status == 1, (st == 1) & (c.back_status == 1))
    sub = (c.back_status == 1) | (st == 0)  # the points with no backward loss
    c2 = F.checked_trace(Pa, Pb, pts[sub], 21, 2, F.LK_ITERS, F.LK_EPS, F.LK_MIN_EIG, np.inf, O.ACCUM_EXACT)
    assert np.array_equal(c2.status, st[sub]) and np.array_equal(c2.next_pts, nxt[sub])


def test_keep_mask_is_monotone_in_the_threshold():
    Pa, Pb = F.lk_pyramids(9, 2)
    pts = F.lk_inputs()[2]
    masks = [F.checked_trace(Pa, Pb, pts, 9, 2, F.LK_ITERS, F.LK_EPS, F.LK_MIN_EIG, thr, O.ACCUM_EXACT).status == 1
             for thr in (0.05, 0.25, 1.0, 4.0, np.inf)]
    for lo, hi in zip(masks, masks[1:]):
        assert np.all(hi[lo])
    assert masks[0].sum() < masks[2].sum() < masks[-1].sum()


@pytest.mark.parametrize("cid", sorted({c.id for c in F.LOOP_CASES if not c.options}))
def test_loop_inputs_have_every_kind_and_move_predictions(cid):
    """(the cases that differ by context options only share the default case's oracle run)"""
    c = F.LOOP_BY_ID[cid]
    run = F.loop_oracle(c.seed, c.opt, c.cfg, c.ransac)
    plain = F.loop_oracle(c.seed, 0, c.cfg, c.ransac)
    tot = {k: sum(x[k] for x in run.log) for k in run.log[0]}
    change = F.largest_change(run, plain)
    print(f"{cid}: {tot}, largest prediction change {change:.4f} px")
    assert tot["fwd_lost"] >= 1 and tot["back_lost"] >= 1 and tot["too_far"] >= 1
    assert change > 0.01
    # the metrics' bookkeeping: lk_points enter, klt_points are the kept pairs
    assert sum(m["lk_points"] for m in run.metrics) == tot["pairs"] + tot["fwd_lost"]
    assert sum(m["klt_points"] for m in run.metrics) == tot["kept"]
    assert sum(m["klt_points"] for m in run.metrics) < sum(m["klt_points"] for m in plain.metrics)


def test_every_option_case_shares_an_oracle_run_checked_above():
    plain_ids = {(c.seed, c.opt, tuple(sorted(c.cfg.items())), c.ransac) for c in F.LOOP_CASES if not c.options}
    for c in F.LOOP_CASES:
        assert (c.seed, c.opt, tuple(sorted(c.cfg.items())), c.ransac) in plain_ids, c.id
