"""The numpy restatement of cv::estimateRigidTransform's point-set branch
(tests/_rigid_oracle.py) vs outputs recorded from the real function
(tests/golden/rigid_transform_cases.npz, recorded by tools/record_rigid_cases.py):
the same sets get a transform, and the matrices agree within the project's fit
tolerance 64 eps cond(A_inliers) max(1, |M|) (the restatement's eigen solve is
LAPACK's, the reference's is Jacobi).  No GPU."""
import os

import numpy as np
import pytest

import _rigid_oracle as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rigid_transform_cases.npz")


@pytest.fixture(scope="module")
def cases():
    z = np.load(GOLDEN)
    o = z["offsets"]
    return [(z["a"][o[i]:o[i + 1]], z["b"][o[i]:o[i + 1]], int(z["max_iters"][i]), float(z["good_ratio"][i]),
             bool(z["found"][i]), z["M"][i].reshape(2, 3)) for i in range(len(o) - 1)]


def test_rng_first_draws_match_recorded():
    # cv::RNG((uint64)-1): next() x 8 and uniform(0, 37) x 12, recorded from the reference
    r = R.RNG()
    assert [r.next() for _ in range(8)] == [130063605, 3133359004, 2578348940, 925327173, 1080261831, 2946015512,
                                            94037301, 2298661280]
    r = R.RNG()
    assert [r.uniform(0, 37) for _ in range(12)] == [21, 18, 18, 19, 26, 32, 25, 20, 4, 1, 2, 17]


def test_fixture_covers_the_edge_cases(cases):
    ns = [len(c[0]) for c in cases]
    assert {0, 1, 2, 3, 256} <= set(ns) and max(ns) == 256
    assert any(c[4] for c in cases) and any(not c[4] for c in cases)
    assert os.path.getsize(GOLDEN) <= 256 * 1024


def test_restatement_matches_recorded_reference(cases):
    nfound = 0
    for i, (a, b, mi, gr, found, M) in enumerate(cases):
        r = R.estimate(a, b, mi, gr)
        assert r.found == found, (i, len(a), mi, gr)
        assert (r.k >= 0) == found and r.inliers.any() == found
        if not found:
            continue
        nfound += 1
        tol = R.tolerance(a[r.inliers], b[r.inliers], M)
        assert np.all(np.abs(r.M - M) <= tol), (i, r.M - M, tol)
    assert nfound >= 30


def test_closed_form_hypotheses_change_no_decision(cases):
    # the kernel solves the 3-point hypotheses in closed form: same rounds, same masks
    for i, (a, b, mi, gr, found, _) in enumerate(cases):
        if len(a) > 64 and not found:
            continue  # the long no-consensus searches are covered by the test above
        r0, r1 = R.estimate(a, b, mi, gr), R.estimate(a, b, mi, gr, solve=R.closed_form)
        assert r0.k == r1.k and r0.rounds == r1.rounds and np.array_equal(r0.inliers, r1.inliers), i
