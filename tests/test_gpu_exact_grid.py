"""FTRL-vs-exact-FTL regret grids (ocx_dev_ftrl_vs_exact_curve_etas and the layers above it): M
FTRL step sizes beside one exact-FTL column, observed at K checkpoint horizons per pass over z.

The reference of every check is the CPU oracle on the truncated input, the existing curve call
(DeviceBatch.ftrl_vs_exact_curve, one step size per call) or the existing single-horizon kernel
(DeviceBatch.ftrl_vs_exact) — never the grid code: bit for bit in every output, and
`close_closed` (the project's bar for a closed-form comparator) against the oracle where the
closed form was taken."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _etas_cases as E
from tests import _exact_grid_cases as G
from tests import _families as F

pytestmark = pytest.mark.gpu

ETAS = G.ETAS7
M = len(ETAS)
UNIQUE = sorted({ETAS.index(e) for e in ETAS})     # first column of every distinct step size
TOL = 1e-12
THREE = ("cum_ftrl", "comp_ftl", "ftrl")                                   # [B, M, K]
TWO = ("cum_exact", "comp", "exact", "action", "in_regime", "closed")     # [B, K(, d)]


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


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def column(grid, m):
    """Column m of a grid result in the shape of a curve result."""
    return {k: (v[:, m] if k in THREE else v) for k, v in grid.items()}


def assert_column_equals(grid, m, ref, ctx, keys=None):
    col = column(grid, m)
    for what in (keys or ref.keys()):
        assert np.array_equal(col[what], ref[what]), ctx + (m, what)


# ------------------------------------------------------------------ 1. exact modes vs the oracle
@functools.lru_cache(maxsize=None)
def oracle_grid(name, d, t, B, T, norm="l2"):
    """test_gpu_exact_curve.oracle_exact's recipe on the first t steps of a family, per sequence
    and distinct step size: exact FTL's (cum, comp, action, in_regime) once, FTRL's regret and
    cum against that action and the loss of FTL(theta_ftrl) per eta0."""
    f = G.family(name, d, B, T, norm)
    n = f.z.shape[0]
    cum_e, comp = np.zeros(n), np.zeros(n)
    act, rg = np.zeros((n, d)), np.zeros(n, dtype=bool)
    cum_r, comp_f, ftrl = (np.zeros((n, M)) for _ in range(3))
    for b in range(n):
        zb, yb = f.z[b, :t], f.y[b, :t]
        cum_e[b], comp[b], act[b], rg[b] = O.ftl_exact_closed_form(zb, yb, norm)
        for m in UNIQUE:
            r = O.simulate_alg_full(zb, yb, 0, ETAS[m], comparator=act[b])
            ftrl[b, m], cum_r[b, m] = r[0], r[1]
            comp_f[b, m] = O.simulate_alg_full(zb, yb, 0, ETAS[m])[2]
    for m in range(M):
        u = ETAS.index(ETAS[m])
        ftrl[:, m], cum_r[:, m], comp_f[:, m] = ftrl[:, u], cum_r[:, u], comp_f[:, u]
    return {"cum_exact": cum_e, "comp": comp, "action": act, "in_regime": rg, "cum_ftrl": cum_r,
            "comp_ftl": comp_f, "ftrl": ftrl, "exact": cum_e - comp}


def check_exact_against_oracle(eng, name, P, d, cks, B_, T_, norm="l2"):
    f = G.family(name, d, B_, T_, norm)
    got = eng.ftrl_vs_exact_curve_etas_batch(f.z, f.y, cks, ETAS, norm=norm, lanes_per_seq=P,
                                             check_regime=False, with_ftl_comparator=True)
    K = len(cks)
    assert got["cum_ftrl"].shape == got["comp_ftl"].shape == got["ftrl"].shape == (B_, M, K)
    assert got["cum_exact"].shape == (B_, K) and got["action"].shape == (B_, K, d)
    assert np.all(got["closed"] == 0)   # streamed comparator for every pair
    for k, t in enumerate(cks):
        ref = oracle_grid(name, d, t, B_, T_, norm)
        for what in THREE:
            assert np.array_equal(got[what][:, :, k], ref[what]), (name, P, d, norm, t, what)
        for what in ("cum_exact", "comp", "exact", "action", "in_regime"):
            assert np.array_equal(got[what][:, k], ref[what]), (name, P, d, norm, t, what)
    return got


@pytest.mark.parametrize("name", ("gt_like", "beam"))
@pytest.mark.parametrize("P,d", G.EXACT)
def test_exact_modes_equal_the_oracle_on_every_prefix(eng, P, d, name):
    got = check_exact_against_oracle(eng, name, P, d, G.CHECKPOINTS, G.B, G.T)
    if name == "beam":   # rows of norm ~1.6: outside the l2 regime from the first row on
        assert not got["in_regime"][:, 1:].any()


@pytest.mark.parametrize("d", (100, 1024))
def test_exact_modes_equal_the_oracle_wide(eng, d):
    check_exact_against_oracle(eng, "gt_like", 1, d, G.SHORT_CHECKPOINTS, G.SHORT_B, G.SHORT_T)


@pytest.mark.parametrize("P", (1, -1, -4))
@pytest.mark.parametrize("norm", ("l1", "linf"))
def test_exact_modes_equal_the_oracle_l1_linf(eng, norm, P):
    cks = list(range(G.SHORT_T + 1))
    got = check_exact_against_oracle(eng, "gt_like", P, 5, cks, G.SHORT_B, G.SHORT_T, norm)
    assert got["in_regime"].all()


# ------------------------------------------------------------------ 2. every layout vs the curve call
CASES = [(P, d, name, "l2") for P, d in G.LAYOUTS for name in G.families_for(d)] + \
        [(P, d, "gt_like", norm) for P, d in G.LAYOUTS if d in (5, 64) for norm in ("l1", "linf")]


@pytest.mark.parametrize("P,d,name,norm", CASES)
def test_columns_equal_the_existing_curve_call(eng, P, d, name, norm):
    """[:, m, :] of the grid and its eta-independent outputs against
    DeviceBatch.ftrl_vs_exact_curve(cks, etas[m]) on the same resident batch, with the closed
    comparator off and on, with and without comp_ftl: every output, bit for bit, for every m."""
    f = G.family(name, d, G.B, G.T, norm)
    db = eng.DeviceBatch(G.B, G.T, d, lanes_per_seq=P).pack(f.z, f.y)
    for closed in (False, True):
        for with_f in (False, True):
            kw = dict(norm=norm, closed_comparator=closed, with_ftl_comparator=with_f,
                      with_actions=True)
            got = host(db.ftrl_vs_exact_curve_etas(G.CHECKPOINTS, ETAS, **kw))
            assert got["cum_ftrl"].shape == (G.B, M, len(G.CHECKPOINTS))
            assert ("comp_ftl" in got) == with_f
            for m in UNIQUE:
                ref = host(db.ftrl_vs_exact_curve(G.CHECKPOINTS, ETAS[m], **kw))
                assert set(ref) == set(got)
                assert_column_equals(got, m, ref, (P, d, name, norm, closed, with_f))
            for m in range(M):   # the duplicate columns
                u = ETAS.index(ETAS[m])
                for what in THREE:
                    if what in got:
                        assert np.array_equal(got[what][:, m], got[what][:, u]), (m, what)
            if closed and norm == "l2" and name != "beam":   # rows in the ball, labels +-1
                assert np.all(got["closed"] == 1)
            elif name == "beam":
                assert np.all(got["closed"][:, 1:] == 0)
            else:
                assert np.all(got["closed"] == 0)


# ------------------------------------------------------------------ 3. grouping changes nothing
GROUP_LAYOUTS = [(8, 16), (8, 32), (8, 64), (1, 5), (-4, 16), (-8, 64), (-4, 64), (64, 1024)]


def offers(L, group):
    """Whether the layout has the `group` instance: the argument check of an empty call."""
    from online_convex_optimization_amd import _lib
    buf = ctypes.c_void_p(16)   # never dereferenced: M = 0
    rc = _lib.load().ocx_dev_ftrl_vs_exact_curve_etas(
        ctypes.byref(L), buf, buf, None, 0, None, 0, None, None, None, None, None, None, None,
        0, 0, group, None, 0, None)
    return rc == 0


@pytest.mark.parametrize("P,d", GROUP_LAYOUTS)
def test_forced_groups_equal_the_default(eng, P, d):
    f = G.family("beam", d)
    db = eng.DeviceBatch(G.B, G.T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert offers(db.L, 1)
    ran = []
    for closed in (False, True):
        kw = dict(closed_comparator=closed, with_ftl_comparator=True, with_actions=True)
        want = host(db.ftrl_vs_exact_curve_etas(G.CHECKPOINTS, ETAS, **kw))
        for g in (1, 2, 4):
            if not offers(db.L, g):
                with pytest.raises(Exception):
                    db.ftrl_vs_exact_curve_etas(G.CHECKPOINTS, ETAS, _group=g, **kw)
                continue
            ran.append(g)
            got = host(db.ftrl_vs_exact_curve_etas(G.CHECKPOINTS, ETAS, _group=g, **kw))
            for what, v in want.items():
                assert np.array_equal(got[what], v), (P, d, closed, g, what)
        for what in THREE:   # the two sqrt 2 columns
            assert np.array_equal(want[what][:, 2], want[what][:, 3]), what
    assert 1 in ran


# ------------------------------------------------------------------ 4. certificate per pair
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_certificate_per_pair(eng, P, d):
    """`closed` is 0 exactly at the checkpoints after an edit (a 1.5- or (1 + 1e-9)-norm row, a
    0.5 label, the zero row with label 0), for every step size; those pairs carry the streamed
    call's bits, the certified ones pass the project's bar against the oracle, and a certified
    sequence keeps the closed form whatever shares its wave."""
    f, edits, _ = E.cert_etas_case(d)
    Bc, Tc = f.y.shape
    cks = G.CERT_CHECKPOINTS
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    kw = dict(with_ftl_comparator=True, with_actions=True)
    two = host(db.ftrl_vs_exact_curve_etas(cks, ETAS, closed_comparator=False, **kw))
    one = host(db.ftrl_vs_exact_curve_etas(cks, ETAS, closed_comparator=True, **kw))
    K = len(cks)
    want_rg = np.ones((Bc, K), dtype=np.int32)
    want_cl = np.ones((Bc, K), dtype=np.int32)
    for b, (kind, val, te) in edits.items():
        after = np.array([1 if te < t else 0 for t in cks])
        want_cl[b] = 1 - after
        if not (kind == "row" and val < 1.5):   # the 1 + 1e-9 rows stay in the regime
            want_rg[b] = 1 - after
    assert np.array_equal(one["in_regime"], want_rg) and np.array_equal(two["in_regime"], want_rg)
    assert np.array_equal(one["closed"], want_cl) and np.all(two["closed"] == 0)
    S = db.L.S   # unedited sequences sharing a wave with an edited one: closed everywhere
    shared = [b for b in range(Bc) if b not in edits and any(e // S == b // S for e in edits)]
    assert shared or S == 1
    assert np.all(one["closed"][shared] == 1)
    op = want_cl == 0
    for what in ("cum_exact", "comp", "exact"):
        assert np.array_equal(one[what][op], two[what][op]), what
    for what in THREE:
        for m in range(M):
            assert np.array_equal(one[what][:, m][op], two[what][:, m][op]), (what, m)
    for what in ("cum_ftrl", "cum_exact", "action"):
        assert np.array_equal(one[what], two[what]), what
    for m in UNIQUE:   # and the whole grid is the curve call's, column by column
        ref = host(db.ftrl_vs_exact_curve(cks, ETAS[m], closed_comparator=True, **kw))
        assert_column_equals(one, m, ref, (P, d))
    for k, t in enumerate(cks):   # the certified pairs against the oracle: the project's bar
        ref = [O.ftl_exact_closed_form(f.z[b, :t], f.y[b, :t]) for b in range(Bc)]
        assert np.array_equal(one["in_regime"][:, k], [int(r[3]) for r in ref]), t
        cl = want_cl[:, k] == 1
        assert close_closed(one["comp"][cl, k], np.array([r[1] for r in ref])[cl], t), (P, d, t)
        for m in UNIQUE:
            want = np.array([O.simulate_alg_full(f.z[b, :t], f.y[b, :t], 0, ETAS[m])[2]
                             for b in np.flatnonzero(cl)])
            assert close_closed(one["comp_ftl"][cl, m, k], want, t), (P, d, t, m)


# ------------------------------------------------------------------ 5. sweep form
@pytest.mark.parametrize("P,d,name", [(8, 64, "gt_like"), (8, 64, "beam"), (1, 5, "beam"),
                                      (-4, 64, "beam"), (8, 16, "straddle"), (0, 64, "always")])
def test_sweep_form_equals_the_single_horizon_kernel(eng, P, d, name):
    import torch
    f = G.family(name, d)
    db = eng.DeviceBatch(G.B, G.T, d, lanes_per_seq=P).pack(f.z, f.y)
    for closed in (False, True):
        got = host(db.ftrl_vs_exact_etas(ETAS, closed_comparator=closed, with_ftl_comparator=True,
                                         with_actions=True))
        assert got["cum_ftrl"].shape == (G.B, M) and got["comp"].shape == (G.B,)
        assert got["action"].shape == (G.B, d)
        for m in UNIQUE:
            cf = torch.zeros(G.B, dtype=torch.float64, device=db.device)
            act = torch.zeros((G.B, d), dtype=torch.float64, device=db.device)
            rg = db.ftrl_vs_exact(ETAS[m], comp_ftl=cf, cmp_action=act, closed_comparator=closed)
            torch.cuda.synchronize()
            ref = {"cum_ftrl": db.cum[:G.B], "cum_exact": db.cum_exact[:G.B],
                   "comp": db.comp[:G.B], "in_regime": rg[:G.B], "comp_ftl": cf, "action": act}
            for what, v in ref.items():
                g = got[what][:, m] if what in THREE else got[what]
                assert np.array_equal(g, v.cpu().numpy()), (P, d, name, closed, m, what)


# ------------------------------------------------------------------ 6. general-solver fill
def test_general_fill_equals_the_curve_call_per_step_size(eng):
    """linf on the reference's own rows (un-scaled gt_like: ||z||_1 > 1, outside the regime):
    one general solve, whatever M is, fills what the per-step-size calls fill."""
    import torch
    f = F.make("gt_like", G.SHORT_B, G.SHORT_T, 5, 105)
    cks = G.SHORT_CHECKPOINTS
    db = eng.DeviceBatch(G.SHORT_B, G.SHORT_T, 5).pack(f.z, f.y)
    solves = []
    call = db._call

    def counting(name, *args):
        if name.startswith("ocx_dev_exact_ball_solve"):
            solves.append(name)
        return call(name, *args)

    db._call = counting
    got = host(db.ftrl_vs_exact_curve_etas_general(cks, ETAS, norm="linf", with_actions=True))
    assert len(solves) == 1
    gap = db.exact_gap_max
    assert gap > 0.0 and not got["in_regime"][:, 2:].any()
    # the certificate bar of check_certificates, on the filled pairs
    assert gap <= eng.EXACT_GAP_RTOL * (1.0 + np.abs(got["comp"]).max())
    for m in UNIQUE:
        ref = host(db.ftrl_vs_exact_curve_general(cks, ETAS[m], norm="linf", with_actions=True))
        assert db.exact_gap_max == gap
        assert np.array_equal(got["cum_ftrl"][:, m], ref["cum_ftrl"]), m
        assert_column_equals(got, m, ref, ("general",))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 7. driver
def test_driver_grid_columns_are_the_curve_drivers(eng):
    import torch
    from online_convex_optimization_amd import drivers
    title, grid, runs, reps = "Label flips", [100, 200, 400], 1, 2
    got = drivers.exact_case_regret_grid(title, grid, [1.0, G.SQ2], runs=runs, replicates=reps)
    assert got["FTRL"].shape == (2, 2, 3) and got["FTL (exact)"].shape == (2, 3)
    ref = drivers.exact_case_regret_curves(title, grid, runs=runs, replicates=reps)
    assert np.array_equal(got["FTRL"][:, 1, :], ref["FTRL"])          # that function's sqrt 2
    assert np.array_equal(got["FTL (exact)"], ref["FTL (exact)"])
    # the 1.0 column: the curve call on the same generated batch
    family_, stream0 = drivers.CASE_FAMILIES[title]
    db = eng.DeviceBatch(runs * reps, 400, 5, lanes_per_seq=1)
    run_idx = np.repeat(np.arange(runs), reps)
    db.generate_family(family_, 2025 * (run_idx + 1), stream0 + np.tile(np.arange(reps), runs))
    one = host(db.ftrl_vs_exact_curve_general(grid, 1.0))
    assert np.array_equal(got["FTRL"][:, 0, :], one["ftrl"])
    assert np.array_equal(got["FTL (exact)"], one["exact"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 8. device checkpoints out of contract
@pytest.mark.parametrize("P,d,norm", [(8, 64, "l2"), (1, 5, "l2"), (-4, 5, "linf"), (8, 16, "l2")])
def test_bad_device_checkpoints_write_nothing_outside(eng, P, d, norm):
    """An unordered, repeated, out-of-range DEVICE checkpoint array (the caller's precondition
    broken): the numbers are meaningless, but the clamped, forward-only walk writes nothing
    outside the outputs and the workspace — every buffer sits between guard words that must
    survive, for a grid of three passes (M = 7 at group <= 4, the last one short)."""
    import torch
    from online_convex_optimization_amd import _lib
    lib = _lib.load()
    f = F.cert_case(64)[0] if d == 64 else G.family("gt_like", d, 37, 130)
    Bc, Tc = f.y.shape
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    ck = torch.tensor([300, -5, 7, 7, 2, 1 << 40, Tc, -(1 << 40)], dtype=torch.int64,
                      device=db.device)
    K, GW = int(ck.numel()), 64
    et = np.ascontiguousarray(ETAS, dtype=np.float64)
    need = lib.ocx_ftrl_exact_grid_workspace_bytes(ctypes.byref(db.L), M, K, 1)
    assert need > 0 and need % 8 == 0

    def guarded(n, dtype, fill):
        t = torch.full((n + 2 * GW,), fill, dtype=dtype, device=db.device)
        return t, t[GW:GW + n]

    bufs = {k: guarded(Bc * M * K, torch.float64, -7.25) for k in ("cum_ftrl", "comp_ftl")}
    bufs.update({k: guarded(Bc * K, torch.float64, -7.25) for k in ("cum_exact", "comp")})
    bufs["action"] = guarded(Bc * K * d, torch.float64, -7.25)
    bufs["regime"] = guarded(Bc * K, torch.int32, -77)
    bufs["closed"] = guarded(Bc * K, torch.int32, -77)
    bufs["ws"] = guarded(need // 8, torch.float64, -7.25)
    for flags in (0, _lib.OCX_ALG_CLOSED_COMPARATOR):
        rc = lib.ocx_dev_ftrl_vs_exact_curve_etas(
            ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), et.ctypes.data_as(_lib.c_dp), M,
            ck.data_ptr(), K, bufs["cum_ftrl"][1].data_ptr(), bufs["cum_exact"][1].data_ptr(),
            bufs["comp"][1].data_ptr(), bufs["comp_ftl"][1].data_ptr(),
            bufs["action"][1].data_ptr(), bufs["regime"][1].data_ptr(),
            bufs["closed"][1].data_ptr(), eng._norm_code(norm), flags, 0,
            bufs["ws"][1].data_ptr(), need,
            ctypes.c_void_p(torch.cuda.current_stream(db.device).cuda_stream))
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        for name, (whole, _) in bufs.items():
            fill = -77 if whole.dtype == torch.int32 else -7.25
            assert bool((whole[:GW] == fill).all()) and bool((whole[-GW:] == fill).all()), name
    # every output word was written (K emissions per sequence and column whatever the list holds)
    assert not bool((bufs["regime"][1] == -77).any()) and not bool((bufs["closed"][1] == -77).any())
    assert not bool((bufs["cum_ftrl"][1] == -7.25).any())
    assert not bool((bufs["cum_exact"][1] == -7.25).any())


def test_degenerate_shapes(eng):
    f = G.family("gt_like", 5)
    db = eng.DeviceBatch(G.B, G.T, 5, lanes_per_seq=1).pack(f.z, f.y)
    out = host(db.ftrl_vs_exact_curve_etas([], ETAS, with_ftl_comparator=True))
    assert out["cum_ftrl"].shape == out["comp_ftl"].shape == (G.B, M, 0)
    assert out["comp"].shape == (G.B, 0)
    out = host(db.ftrl_vs_exact_curve_etas([1, 5], []))
    assert out["cum_ftrl"].shape == out["ftrl"].shape == (G.B, 0, 2)
    assert out["exact"].shape == (G.B, 2)
    out = host(eng.DeviceBatch(G.B, 0, 64, lanes_per_seq=8).ftrl_vs_exact_curve_etas([0], ETAS))
    assert all(np.all(out[k] == 0.0) for k in ("ftrl", "exact", "cum_ftrl", "cum_exact", "comp"))
    assert out["in_regime"].all()
