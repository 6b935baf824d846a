"""Regret curves (ocx_dev_simulate_alg_curve and the layers above it): FTRL / FTL observed at
checkpoint horizons in one pass.

The reference of every check is the existing code or the C oracle on the TRUNCATED input
(z[:, :t_k], y[:, :t_k]), never the curve code: bit for bit against the oracle in the exact
modes, bit for bit against the existing kernels in the same layout (the layout does not depend
on T, so a truncated run is the same arithmetic), and `close_closed` against the oracle where
the closed form was taken."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F

pytestmark = pytest.mark.gpu

# ring depth, the 64-step boundaries of the pipelined kernel's re-sum and of the FTRL scale
# table, the last step and both ends
CHECKPOINTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257]
CERT_CHECKPOINTS = [1, 63, 64, 65, 129, 130]
B, T = F.PIPE_B, 257
TOL = 1e-12


def close_closed(a, b, T):
    """tests/test_gpu_parity.py's bar for the closed-form comparator against the reference's
    sequential sum of T terms: |diff| <= max(1e-12 * max(1, |ref|), 4 eps T^1.5)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    tol = np.maximum(TOL * np.maximum(1.0, np.abs(b)), 4 * 2.22e-16 * float(T) ** 1.5)
    return np.all(np.abs(a - b) <= tol)


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    _lib.load()
    return engine


@functools.lru_cache(maxsize=None)
def family(name, d, B=B, T=T):
    return F.make(name, B, T, d, 100 + d)   # shared between tests: never written to


@functools.lru_cache(maxsize=None)
def oracle(name, d, t):
    """(regret, cum, comp) of the C oracle (simulate_alg_full per sequence) on the first t
    steps of a family."""
    f = family(name, d)
    return O.simulate_alg_batch(f.z[:, :t], f.y[:, :t], f.flag, f.eta0, nthreads=4)[:3]


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100), (1, 1024)]


@pytest.mark.parametrize("name", ("gt_like", "straddle", "always", "pairs", "small"))
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle_on_every_prefix(eng, P, d, name):
    f = family(name, d)
    reg, cum, comp, closed = eng.simulate_alg_curve_batch(
        f.z, f.y, CHECKPOINTS, f.flag, f.eta0, lanes_per_seq=P, return_all=True)
    assert reg.shape == cum.shape == comp.shape == closed.shape == (B, len(CHECKPOINTS))
    assert np.all(closed == 0)   # streamed comparator for every pair
    for k, t in enumerate(CHECKPOINTS):
        ref = oracle(name, d, t)
        for got, want, what in ((reg, ref[0], "regret"), (cum, ref[1], "cum"),
                                (comp, ref[2], "comp")):
            assert np.array_equal(got[:, k], want), (P, d, name, t, what)


# ------------------------------------------------------------------ 2. every layout vs the existing kernels
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64)]


@pytest.mark.parametrize("name", ("gt_like", "always", "pairs", "small"))
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_columns_equal_the_existing_kernels_on_truncated_input(eng, P, d, name):
    """Column k of the device call against the existing kernels on (z[:, :t_k], y[:, :t_k]) in
    the same layout: flags = 0 against the two-pass run, the closed form requested against
    simulate_alg(closed_comparator=True) — regret, cum, comp and the closed flags, bit for bit.
    The two-pass reference is DeviceBatch.simulate_alg(closed_comparator=False), the same
    dispatch as the curve's (engine.simulate_alg_batch(return_all=True) asks for x_last, which
    sends a butterfly layout to the plain kernel: another summation); its regret is also
    checked against engine.simulate_alg_batch without x_last."""
    import torch
    f = family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    two = host(db.simulate_alg_curve(CHECKPOINTS, f.flag, f.eta0, closed_comparator=False))
    one = host(db.simulate_alg_curve(CHECKPOINTS, f.flag, f.eta0, closed_comparator=True))
    assert np.all(two["closed"] == 0)
    for k, t in enumerate(CHECKPOINTS):
        key = (P, d, name, t)
        dt = eng.DeviceBatch(B, t, d, lanes_per_seq=P).pack(f.z[:, :t], f.y[:, :t])
        assert (dt.L.P, dt.L.C, dt.L.chain) == (db.L.P, db.L.C, db.L.chain)
        dt.simulate_alg(f.flag, f.eta0, closed_comparator=False)
        torch.cuda.synchronize()
        for what, ref in (("regret", dt.regret), ("cum", dt.cum), ("comp", dt.comp)):
            assert np.array_equal(two[what][:, k], ref[:B].cpu().numpy()), key + (what, 0)
        reg_host = eng.simulate_alg_batch(f.z[:, :t], f.y[:, :t], f.flag, f.eta0, lanes_per_seq=P)
        assert np.array_equal(two["regret"][:, k], reg_host), key
        cl = torch.full((B,), 7, dtype=torch.int32, device=dt.device)
        dt.simulate_alg(f.flag, f.eta0, closed_comparator=True, closed_out=cl)
        torch.cuda.synchronize()
        for what, ref in (("regret", dt.regret), ("cum", dt.cum), ("comp", dt.comp),
                          ("closed", cl)):
            assert np.array_equal(one[what][:, k], ref[:B].cpu().numpy()), key + (what, 1)
    if name in ("gt_like", "always", "small"):
        assert np.all(one["closed"] == 1)


# ------------------------------------------------------------------ 3. certificates
@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_certificates_per_prefix(eng, P, d, flag):
    """A sequence whose certificate breaks at step t_e is closed at exactly the checkpoints
    t_k <= t_e (no edit at a step < t_k), streams the others with the bits of the flags = 0
    call, and never takes a wave neighbour with it."""
    f, edits, _ = F.cert_case(d)
    Bc, Tc = f.y.shape
    assert (Bc, Tc) == (37, 130)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    two = host(db.simulate_alg_curve(CERT_CHECKPOINTS, flag, f.eta0, closed_comparator=False))
    one = host(db.simulate_alg_curve(CERT_CHECKPOINTS, flag, f.eta0, closed_comparator=True))
    want = np.ones((Bc, len(CERT_CHECKPOINTS)), dtype=np.int32)
    for b, (_, _, te) in edits.items():
        want[b] = [0 if te < t else 1 for t in CERT_CHECKPOINTS]
    assert np.array_equal(one["closed"], want)
    # unedited sequences sharing a wave with an edited one: closed everywhere (a requirement)
    S = db.L.S
    shared = [b for b in range(Bc) if b not in edits
              and any(e // S == b // S for e in edits)]
    assert shared or S == 1
    assert np.all(one["closed"][shared] == 1)
    assert np.all(two["closed"] == 0)
    op = want == 0
    for what in ("regret", "cum", "comp"):
        assert np.array_equal(one[what][op], two[what][op]), what
    assert np.array_equal(one["cum"], two["cum"])
    for k, t in enumerate(CERT_CHECKPOINTS):
        ref = O.simulate_alg_batch(f.z[:, :t], f.y[:, :t], flag, f.eta0, nthreads=4)
        cl = want[:, k] == 1
        for i, what in enumerate(("regret", "cum", "comp")):
            assert close_closed(one[what][cl, k], ref[i][cl], t), (P, d, flag, t, what)


# ------------------------------------------------------------------ 4. degenerate lists
def test_degenerate_checkpoint_lists(eng):
    f = family("gt_like", 5)
    # K = 1 with [T]: the whole-horizon call
    got = eng.simulate_alg_curve_batch(f.z, f.y, [T], 0, f.eta0, lanes_per_seq=1, return_all=True)
    ref = eng.simulate_alg_batch(f.z, f.y, 0, f.eta0, lanes_per_seq=1, return_all=True)
    for g, r in zip(got[:3], ref[:3]):
        assert g.shape == (B, 1) and np.array_equal(g[:, 0], r)
    # K = 0
    got = eng.simulate_alg_curve_batch(f.z, f.y, [], 0, f.eta0, lanes_per_seq=1, return_all=True)
    assert all(g.shape == (B, 0) for g in got)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    assert all(v.shape == (B, 0) for v in host(db.simulate_alg_curve([])).values())
    # T = 0 with [0]
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    for lanes in (1, 0):
        got = eng.simulate_alg_curve_batch(z0, y0, [0], 0, f.eta0, lanes_per_seq=lanes,
                                           return_all=True)
        assert all(g.shape == (B, 1) and np.all(g[:, :1] == 0.0) for g in got[:3])
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_alg_curve([0]))
    assert all(np.all(out[k] == 0.0) for k in ("regret", "cum", "comp"))


@pytest.mark.parametrize("flag", (0, 1))
def test_every_step_is_a_checkpoint(eng, flag):
    """K = T + 1 at T = 40, d = 5, exact mode: 41 oracle calls per sequence."""
    Ts, Bs = 40, 9
    f = F.make("gt_like" if flag == 0 else "small", Bs, Ts, 5, 77)
    got = eng.simulate_alg_curve_batch(f.z, f.y, list(range(Ts + 1)), flag, f.eta0,
                                       lanes_per_seq=1, return_all=True)
    for b in range(Bs):
        for t in range(Ts + 1):
            ref = O.simulate_alg_full(f.z[b, :t], f.y[b, :t], flag, f.eta0)
            assert (got[0][b, t], got[1][b, t], got[2][b, t]) == tuple(ref[:3]), (b, t)


def test_host_entry_takes_the_closed_form_outside_the_exact_modes(eng):
    f = family("gt_like", 64)
    reg, cum, comp, closed = eng.simulate_alg_curve_batch(
        f.z, f.y, CHECKPOINTS, 0, f.eta0, lanes_per_seq=8, return_all=True)
    assert np.all(closed == 1)
    for k, t in enumerate(CHECKPOINTS):
        ref = oracle("gt_like", 64, t)
        assert close_closed(reg[:, k], ref[0], t) and close_closed(comp[:, k], ref[2], t)


# ------------------------------------------------------------------ 5. g(T) layer
def test_gT_regret_curves_exact(eng):
    cks = [50, 100, 200]
    got = eng.gT_regret_curves(200, 20, cks, d=5, lanes_per_seq=1, batch=8)  # 8 + 8 + 4
    assert got.shape == (20, 3)
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 5)
        for k, t in enumerate(cks):
            assert got[r, k] == O.simulate_alg_full(z[:t], y[:t], 0, eng.SQRT2)[0], (r, t)
    assert np.array_equal(got[:, 2], eng.gT_regrets(200, 20, lanes_per_seq=1))


def test_gT_regret_curves_closed_form(eng):
    cks = [50, 100, 200]
    got, closed = eng.gT_regret_curves(200, 20, cks, d=64, lanes_per_seq=eng.LANES_BEST, batch=8,
                                       return_closed=True)
    assert got.shape == closed.shape == (20, 3) and np.all(closed == 1)
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 64)
        for k, t in enumerate(cks):
            ref = O.simulate_alg_full(z[:t], y[:t], 0, eng.SQRT2)[0]
            assert close_closed(got[r, k], ref, t), (r, t)
