"""The FTRL/FTL kernels on the branches that g(T)-like rows never take: the FTRL rescale
(s²||θ||² > 1) and the pipelined kernel's shortcut around it, FTL's near-origin re-sum and
its return to θ = 0, horizons shorter than the register ring, the closed form's certificate
broken in one place at the pipelined shapes, and the forms that only the generate-and-simulate
pipelines launch (the lean whole-run kernels and the plain kernel over a group range).

The inputs are the families of tests/_families.py; tests/test_families_cpu.py shows from the
reference arithmetic alone that each input reaches its branch, stays 1e-6 away from every
hinge tie and 1e-9 away from the rescale threshold.  The reference is the C oracle
(fast_algorithms.py:88-115); the bars are those of tests/test_gpu_pipe.py: `close` (1e-12
relative) for the two-pass results, `close_closed` for the closed form, bit for bit wherever
two runs are the same arithmetic."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F
from tests.test_gpu_pipe import SHAPES, close, close_closed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    _lib.load()
    return engine


@functools.lru_cache(maxsize=None)
def family(case):
    return F.make(*case)   # shared between tests: never written to


@functools.lru_cache(maxsize=None)
def oracle(case, flag, T=None):
    """(regret, cum, comp, x_last) of the C oracle on a family case (its first T steps)."""
    f = family(case)
    z, y = (f.z, f.y) if T is None else (f.z[:, :T], f.y[:, :T])
    return O.simulate_alg_batch(z, y, flag, f.eta0, nthreads=4)


def run_both(db, flag, eta0):
    """The two-pass run and the closed-form run of one resident batch:
    (regret2, cum2, regret1, cum1, closed flags) as host arrays of the B sequences."""
    import torch
    B = db.L.B
    closed = torch.full((max(B, 1),), 7, dtype=torch.int32, device=db.device)
    r2 = db.simulate_alg(flag, eta0, closed_comparator=False).clone()
    cum2 = db.cum.clone()
    r1 = db.simulate_alg(flag, eta0, closed_comparator=True, closed_out=closed).clone()
    cum1 = db.cum.clone()
    torch.cuda.synchronize()
    return tuple(a[:B].cpu().numpy() for a in (r2, cum2, r1, cum1, closed))


# ------------------------------------------------------------------ pipelined kernel
@pytest.mark.parametrize("name", F.PIPE_FAMILIES)
@pytest.mark.parametrize("P,d", SHAPES)
def test_pipe_kernel_on_family(eng, P, d, name):
    """Every dispatched (lanes, d) instance on the families that rescale (FTRL) and that stay
    near or return to the origin (FTL): two-pass and closed form against the oracle, every
    sequence certified, and the loop's `cum` the same bits in both runs."""
    case = F.pipe_case(name, d)
    f = family(case)
    B, T = f.y.shape
    ref = oracle(case, f.flag)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    r2, cum2, r1, cum1, closed = run_both(db, f.flag, f.eta0)
    assert close(r2, ref[0]) and close(cum2, ref[1]), (P, d, name)
    assert close_closed(r1, ref[0], T), (P, d, name)
    assert np.all(closed == 1)
    assert np.array_equal(cum1, cum2)


# ------------------------------------------------------------------ plain kernel
@pytest.mark.parametrize("case", F.SPLIT_CASES, ids=lambda c: f"{c[0]}-T{c[2]}-d{c[3]}")
def test_plain_kernel_rescale_all_lane_splits(eng, case):
    """test_batch_all_lane_splits' loop on rows that rescale: with x_last asked for, every
    butterfly layout runs the plain kernel, whose rescale branch sums z·x a second time."""
    f = family(case)
    d = f.z.shape[2]
    ref = oracle(case, 0)
    for P in (1, -1, -2, -4, -8, -16, -32, -64, 2, 4, 8, 16, 32, 64):
        if P != 1 and -(-d // abs(P)) > 64:
            continue
        got = eng.simulate_alg_batch(f.z, f.y, 0, f.eta0, lanes_per_seq=P, return_all=True)
        if P == 1 or P < 0:  # exact modes
            assert all(np.array_equal(g, r) for g, r in zip(got, ref)), P
        else:
            assert all(close(g, r) for g, r in zip(got, ref)), P


# ------------------------------------------------------------------ short horizons
@pytest.mark.parametrize("name", F.SHORT_FAMILIES)
@pytest.mark.parametrize("P,d", SHAPES)
def test_pipe_kernel_short_horizons(eng, P, d, name):
    """Horizons below the ring depth (the prologue's and the look-ahead's clamped loads, the
    tn > 0 guards) and around the 64-step refresh, FTRL and FTL."""
    case = F.short_case(name, d)
    f = family(case)
    B = f.y.shape[0]
    for T in F.SHORT_TS:
        db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z[:, :T], f.y[:, :T])
        assert (db.L.P, db.L.chain) == (P, 0)
        for flag in (0, 1):
            ref = oracle(case, flag, T)
            r2, cum2, r1, cum1, closed = run_both(db, flag, f.eta0)
            assert close(r2, ref[0]) and close(cum2, ref[1]), (P, d, name, T, flag)
            assert close_closed(r1, ref[0], T), (P, d, name, T, flag)
            assert np.all(closed == 1) and np.array_equal(cum1, cum2), (T, flag)
            if T == 0:
                assert np.all(r2 == 0.0) and np.all(r1 == 0.0) and np.all(ref[0] == 0.0)


# ------------------------------------------------------------------ certificate edges
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_pipe_kernel_certificate_edges(eng, P, d):
    """A single violation of the closed form's certificate — a row at 1.5x or at 1 + 1e-9 (at
    t = 0, 63, 64, T - 1), a label of 0.5 (first, last step), an exact tie at t = 0 — sends
    that sequence and no other to the second pass, bit-identical to the two-pass run; the
    sequences that share its wave keep the closed form, with the bits they have in a batch
    without the violations."""
    f, edits, base = F.cert_case(d)
    B, T = f.y.shape
    unclean = sorted(edits)
    ok = np.ones(B, dtype=bool)
    ok[unclean] = False
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    db0 = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(base.z, base.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    for flag in (0, 1):
        ref = O.simulate_alg_batch(f.z, f.y, flag, f.eta0, nthreads=4)
        r2, cum2, r1, cum1, closed = run_both(db, flag, f.eta0)
        assert sorted(np.nonzero(closed == 0)[0]) == unclean and np.all(closed[ok] == 1), (P, flag)
        assert np.array_equal(r1[~ok], r2[~ok])
        assert close(r2, ref[0]) and close(cum2, ref[1]) and close_closed(r1, ref[0], T)
        assert np.array_equal(cum1, cum2)
        clean_r1 = run_both(db0, flag, f.eta0)[2]
        assert np.array_equal(r1[ok], clean_r1[ok])


# ------------------------------------------------------------------ range forms
SENTINEL = -7.25


@pytest.mark.parametrize("name", F.RANGE_FAMILIES)
@pytest.mark.parametrize("d,P", F.RANGE_SHAPES)
def test_range_forms_match_whole_batch_kernel(eng, d, P, name):
    """The pipelines' FTRL launches (ocx_test_alg_range: the lean whole-run forms 8 x 8, 16 x 4,
    8 x 4 and the plain kernel over a group range, 8 x 2) on packed rows: inside the range the
    regrets of the whole-batch kernel bit for bit — the second pass of the two unclean
    sequences included —, outside it nothing written, and the folded maximum the bit pattern
    of max(0, max regret) over the range."""
    import torch
    from online_convex_optimization_amd import _lib
    f = F.range_case(name, d)
    B, T = f.y.shape
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    G, S = db.L.G, db.L.S
    assert B % S != 0 and G >= 3
    ref = O.simulate_alg_batch(f.z, f.y, 0, f.eta0, nthreads=4)[0]
    two = db.simulate_alg(0, f.eta0, closed_comparator=False).clone()
    one = db.simulate_alg(0, f.eta0, closed_comparator=True).clone()
    torch.cuda.synchronize()
    two, one = two[:B].cpu().numpy(), one[:B].cpu().numpy()
    assert close(two, ref) and close_closed(one, ref, T)
    for onepass, want in ((0, two), (1, one)):
        for g0, gn in ((0, G), (1, G - 2), (G - 1, 1)):
            got = torch.full((B,), SENTINEL, dtype=torch.float64, device=db.device)
            gmax = torch.zeros(1, dtype=torch.float64, device=db.device)
            torch.cuda.synchronize()
            _lib.call("ocx_test_alg_range", ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(),
                      f.eta0, onepass, g0, gn, got.data_ptr(), gmax.data_ptr(),
                      db.stream.cuda_stream)
            torch.cuda.synchronize()
            got, gm = got.cpu().numpy(), gmax.cpu().numpy()
            lo, hi = g0 * S, min(B, (g0 + gn) * S)
            inside = np.zeros(B, dtype=bool)
            inside[lo:hi] = True
            key = (d, P, name, onepass, g0, gn)
            assert np.array_equal(got[inside], want[inside]), key
            assert np.all(got[~inside] == SENTINEL), key
            exp = np.array([max(0.0, float(want[inside].max()))])
            assert gm.view(np.uint64)[0] == exp.view(np.uint64)[0], key
            for b in F.RANGE_UNCLEAN:
                if inside[b]:
                    assert got[b] == two[b], key
