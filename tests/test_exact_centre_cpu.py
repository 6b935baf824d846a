"""CPU checks of the reference tests/_exact_centre.py gives the GPU test of the general
solver's actions on non-unique minimisers (tests/test_gpu_exact_centre.py).

The centre from its definition must be the limit of the documented central path (a 60-digit
path to μ = 1e-14), every face must be what its construction says (centre and a second point
both optimal by HiGHS and feasible), and the two points must lie far apart: the GPU test's
bar is 1e-6, so an answer at the second point — the closed form's vertex, a simplex vertex, a
far point of an interpolation face — misses it by five decades (two for the near-bound
cases)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import _exact_centre as C
from tests._scipy_solvers import lp_solve, objective

SMALL = [d for d in C.DIMS if d <= 8]


@pytest.mark.parametrize("name", sorted(C.NONUNIQUE))
@pytest.mark.parametrize("d", SMALL)
def test_centre_is_the_central_paths_limit(name, d):
    """d <= 8: the definition's centre against the 60-digit path of F_μ at μ = 1e-14, to 1e-9
    (the path is O(μ) from its limit)."""
    case = C.NONUNIQUE[name](d)
    assert case["prefixes"]
    for n in case["prefixes"]:
        x = C.mp_central_path(case["z"][:n], case["y"][:n], case["norm"])
        dev = np.abs(x - case["centre"][n]).max()
        print(f"{name} d={d} n={n}: |path(1e-14) - centre| = {dev:.2e}")
        assert dev <= 1e-9, (name, n, dev)


def test_asymmetric_l1_centre_value():
    """a = 4: x_p = 0.3950806… (the root of −4/(1 − x) + 4/(½ + ½x) + 1/x − 1/(1 − x))."""
    c = C.l1_tie_asymmetric(5)
    x = c["centre"][12][0]
    assert abs(x - 0.3950806) < 5e-8
    assert abs(-4 / (1 - x) + 4 / (0.5 + 0.5 * x) + 1 / x - 1 / (1 - x)) < 1e-10


def _min_separation(name):
    return 1e-4 if name in C.NEAR_BOUND else 0.1


@pytest.mark.parametrize("name", sorted(C.NONUNIQUE))
@pytest.mark.parametrize("d", C.DIMS)
def test_faces_are_optimal_and_wide(name, d):
    """Every non-unique case at every d: the centre and the second point both attain HiGHS's
    optimum to 1e-9·(1 + f) (l2: the optimum 0 of an interpolation face), both are feasible,
    and they are >= 0.1 apart in the ∞-norm (>= 1e-4 for the near-bound cases)."""
    case = C.NONUNIQUE[name](d)
    norm = case["norm"]
    assert case["prefixes"]
    for n in case["prefixes"]:
        z, y = case["z"][:n], case["y"][:n]
        f = 0.0 if norm == "l2" else lp_solve(z, y, norm)[1]
        for x in (case["centre"][n], case["other"][n]):
            assert C.ball_norm(x, norm) <= 1.0 + 1e-12, (name, n)
            assert abs(objective(z, y, x) - f) <= 1e-9 * (1.0 + f), (name, n, objective(z, y, x), f)
        sep = np.abs(case["centre"][n] - case["other"][n]).max()
        assert sep >= _min_separation(name), (name, n, sep)


@pytest.mark.parametrize("name", C.NEAR_BOUND)
def test_near_bound_centres_are_near_the_bound(name):
    """One free coordinate of the centre in [1e-4, 5e-4]: inside the polish's coarsest kZero."""
    for d in C.DIMS:
        case = C.NONUNIQUE[name](d)
        x = case["centre"][case["prefixes"][0]]
        small = np.abs(x)[(np.abs(x) > 0.0) & (np.abs(x) < 0.5)]
        assert small.size == 1 and 1e-4 <= small[0] <= 5e-4, (d, small)


@pytest.mark.parametrize("name", C.TIE_FAMILIES)
@pytest.mark.parametrize("d", [5, 65])
def test_poly_tie_flags_exactly_the_tied_prefixes(name, d):
    """The oracle's tie test (what takes a sequence out of the closed form's regime) flags
    exactly the prefixes the construction ties, and every checked prefix is one of them."""
    case = C.NONUNIQUE[name](d)
    z, y, norm = case["z"], case["y"], case["norm"]
    theta = np.zeros(d)
    touched = np.zeros(d, dtype=bool)
    flagged = []
    for t in range(z.shape[0]):
        touched |= z[t] != 0.0
        theta = theta + (-y[t]) * z[t]
        if O._poly_tie(theta, touched, norm):
            flagged.append(t + 1)
    assert flagged == case["tied"]
    assert set(case["prefixes"]) <= set(flagged)


@pytest.mark.parametrize("norm", ["l2", "linf", "l1"])
@pytest.mark.parametrize("d", C.DIMS)
def test_interpolation_checks_half_of_the_short_prefixes(norm, d):
    case = C.interpolation(norm, d)
    assert 2 * len(case["prefixes"]) >= case["eligible"], (len(case["prefixes"]), case["eligible"])
    assert all(n < d and C.ball_norm(case["centre"][n], norm) <= 0.9 for n in case["prefixes"])
    assert min(C.ball_norm(case["centre"][n], norm) for n in case["prefixes"]) <= 0.5


@pytest.mark.parametrize("norm", ["l1", "linf"])
def test_tie_coordinates_cross_the_lane_boundaries(norm):
    """The ties do not all sit in coordinates 0 and 1: 0 and d − 1, and 63 and 64 at d >= 65."""
    for d in C.DIMS:
        case = (C.l1_tie_asymmetric if norm == "l1" else C.linf_tie_asymmetric)(d)
        used = set(np.flatnonzero((case["z"] != 0.0).any(axis=0)))
        assert used == ({63, 64} if d >= 65 else {0, d - 1})
