"""FTRL-vs-exact-FTL regret curves (ocx_dev_ftrl_vs_exact_curve and the layers above it): both
loops of ocx_dev_ftrl_vs_exact_ex observed at checkpoint horizons in one pass.

The reference of every check is the existing kernel or the CPU oracle on the TRUNCATED input
(z[:, :t_k], y[:, :t_k]), never the curve code: bit for bit against the oracle in the exact
modes, bit for bit against the existing kernel in the same layout (the layout does not depend
on T, so a truncated run is the same arithmetic), and `close_closed` against the oracle where
the closed form was taken."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F

pytestmark = pytest.mark.gpu

# ring depth (NB <= 8), the 64-step boundaries of the FTRL scale table, the last step, both ends
CHECKPOINTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257]
CERT_CHECKPOINTS = [0, 1, 63, 64, 65, 129, 130]
SHORT_CHECKPOINTS = [0, 1, 2, 7, 8, 9, 39, 40]
B, T = F.PIPE_B, 257
TOL = 1e-12
KEYS = ("cum_ftrl", "cum_exact", "comp", "comp_ftl", "action", "in_regime")


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


@functools.lru_cache(maxsize=6)
def family(name, d, B=B, T=T, norm="l2"):
    """Shared between tests: never written to.  l1 / linf: rows scaled into the dual ball
    (||z||_inf <= 1, resp. ||z||_1 <= 1), so every prefix is in the closed form's regime."""
    f = F.make(name, B, T, d, 100 + d)
    if norm == "linf":
        z = f.z / np.maximum(1.0, np.abs(f.z).sum(axis=2, keepdims=True))
        f = F.Family(z, f.y, f.eta0, f.flag)
    return f


@functools.lru_cache(maxsize=None)
def oracle_exact(name, d, t, B=B, T=T, norm="l2"):
    """The oracle on the first t steps of a family, per sequence: exact FTL's (cum, comp,
    action, in_regime), FTRL's cum against that action, and the loss of FTL(theta_ftrl)."""
    f = family(name, d, B, T, norm)
    n = f.z.shape[0]
    cum_e, comp, cum_r, comp_f, ftrl = (np.zeros(n) for _ in range(5))
    act, rg = np.zeros((n, d)), np.zeros(n, dtype=bool)
    for b in range(n):
        zb, yb = f.z[b, :t], f.y[b, :t]
        cum_e[b], comp[b], act[b], rg[b] = O.ftl_exact_closed_form(zb, yb, norm)
        r = O.simulate_alg_full(zb, yb, 0, f.eta0, comparator=act[b])
        ftrl[b], cum_r[b] = r[0], r[1]
        comp_f[b] = O.simulate_alg_full(zb, yb, 0, f.eta0)[2]
    return {"cum_exact": cum_e, "comp": comp, "action": act, "in_regime": rg, "cum_ftrl": cum_r,
            "comp_ftl": comp_f, "ftrl": ftrl}


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def truncated_batch(eng, f, t, P, d):
    n = f.z.shape[0]
    return eng.DeviceBatch(n, t, d, lanes_per_seq=P).pack(f.z[:, :t], f.y[:, :t])


def truncated(dt, f, norm, closed, with_f):
    """The existing kernel (DeviceBatch.ftrl_vs_exact) on a batch truncated at t."""
    import torch
    n, d = f.z.shape[0], f.z.shape[2]
    cf = torch.zeros(n, dtype=torch.float64, device=dt.device) if with_f else None
    act = torch.zeros((n, d), dtype=torch.float64, device=dt.device)
    rg = dt.ftrl_vs_exact(f.eta0, comp_ftl=cf, cmp_action=act, closed_comparator=closed, norm=norm)
    torch.cuda.synchronize()
    out = {"cum_ftrl": dt.cum[:n], "cum_exact": dt.cum_exact[:n], "comp": dt.comp[:n],
           "action": act, "in_regime": rg[:n]}
    if with_f:
        out["comp_ftl"] = cf
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)]


def check_exact_against_oracle(eng, name, P, d, cks, B_, T_, norm="l2"):
    f = family(name, d, B_, T_, norm)
    got = eng.ftrl_vs_exact_curve_batch(f.z, f.y, cks, f.eta0, norm=norm, lanes_per_seq=P,
                                        check_regime=False, with_ftl_comparator=True)
    assert got["cum_ftrl"].shape == (B_, len(cks)) and got["action"].shape == (B_, len(cks), d)
    assert np.all(got["closed"] == 0)   # streamed comparator for every pair
    for k, t in enumerate(cks):
        ref = oracle_exact(name, d, t, B_, T_, norm)
        for what in KEYS:
            assert np.array_equal(got[what][:, k], ref[what]), (P, d, norm, t, what)
        assert np.array_equal(got["ftrl"][:, k], ref["ftrl"]), (P, d, norm, t)
        assert np.array_equal(got["exact"][:, k], ref["cum_exact"] - ref["comp"]), (P, d, norm, t)


@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle_on_every_prefix(eng, P, d):
    check_exact_against_oracle(eng, "gt_like", P, d, CHECKPOINTS, B, T)


@pytest.mark.parametrize("d", (100, 1024))
def test_exact_modes_equal_the_oracle_wide(eng, d):
    check_exact_against_oracle(eng, "gt_like", 1, d, SHORT_CHECKPOINTS, 6, 40)


@pytest.mark.parametrize("P", (1, -1, -4))
@pytest.mark.parametrize("norm", ("l1", "linf"))
def test_exact_modes_equal_the_oracle_l1_linf(eng, norm, P):
    check_exact_against_oracle(eng, "gt_like", P, 5, list(range(41)), 6, 40, norm)
    assert all(oracle_exact("gt_like", 5, t, 6, 40, norm)["in_regime"].all() for t in range(41))


# ------------------------------------------------------------------ 2. every layout vs the existing kernel
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 64), (-4, 64)]
CASES = [(P, d, name, "l2") for P, d in LAYOUTS for name in ("gt_like", "straddle", "always")] + \
        [(P, d, "gt_like", norm) for P, d in LAYOUTS if d in (5, 64) for norm in ("l1", "linf")]


@pytest.mark.parametrize("P,d,name,norm", CASES)
def test_columns_equal_the_existing_kernel_on_truncated_input(eng, P, d, name, norm):
    """Column k of the device call against DeviceBatch.ftrl_vs_exact on (z[:, :t_k], y[:, :t_k])
    in the same layout, with the closed comparator off and on, with and without comp_ftl:
    cum, cum_exact, comp, comp_ftl, cmp_action and regime, bit for bit."""
    f = family(name, d, B, T, norm)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    variants = [(closed, with_f) for closed in (False, True) for with_f in (False, True)]
    got = {v: host(db.ftrl_vs_exact_curve(CHECKPOINTS, f.eta0, norm=norm, closed_comparator=v[0],
                                          with_ftl_comparator=v[1], with_actions=True))
           for v in variants}
    for v in variants:
        if not v[0] or norm != "l2":
            assert np.all(got[v]["closed"] == 0)
        else:   # rows inside the ball, labels +-1: every prefix certified
            assert np.all(got[v]["closed"] == 1)
    for k, t in enumerate(CHECKPOINTS):
        dt = truncated_batch(eng, f, t, P, d)
        assert (dt.L.P, dt.L.C, dt.L.chain) == (db.L.P, db.L.C, db.L.chain)
        for v in variants:
            ref = truncated(dt, f, norm, v[0], v[1])
            for what, want in ref.items():
                assert np.array_equal(got[v][what][:, k], want), (P, d, name, norm, t, v, what)
            assert np.array_equal(got[v]["ftrl"][:, k], ref["cum_ftrl"] - ref["comp"])
            assert np.array_equal(got[v]["exact"][:, k], ref["cum_exact"] - ref["comp"])
        if norm == "l2":   # the closed form against the oracle's streamed sum: the project's bar
            want = oracle_exact(name, d, t)["comp"]
            assert close_closed(got[(True, False)]["comp"][:, k], want, t), (P, d, name, t)


# ------------------------------------------------------------------ 3. regime and certificate per prefix
@pytest.mark.parametrize("P,d,closed", [(P, d, True) for P, d in F.CERT_SHAPES] + [(1, 64, False)])
def test_regime_and_certificate_per_prefix(eng, P, d, closed):
    """A sequence leaves the regime at the checkpoints after a 1.5-norm row, a 0.5 label or the
    zero row with label 0; a (1 + 1e-9)-norm row only breaks the closed form's certificate.
    A pair is closed exactly where no edit lies before t_k, never takes a wave neighbour with
    it, and the streamed pairs carry the bits of the flags = 0 call."""
    f, edits, _ = F.cert_case(d)
    Bc, Tc = f.y.shape
    assert (Bc, Tc) == (37, 130)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    two = host(db.ftrl_vs_exact_curve(CERT_CHECKPOINTS, f.eta0, closed_comparator=False,
                                      with_ftl_comparator=True, with_actions=True))
    one = host(db.ftrl_vs_exact_curve(CERT_CHECKPOINTS, f.eta0, closed_comparator=closed,
                                      with_ftl_comparator=True, with_actions=True))
    K = len(CERT_CHECKPOINTS)
    want_rg = np.ones((Bc, K), dtype=np.int32)
    want_cl = np.ones((Bc, K), dtype=np.int32)
    for b, (kind, val, te) in edits.items():
        after = np.array([1 if te < t else 0 for t in CERT_CHECKPOINTS])
        want_cl[b] = 1 - after
        if not (kind == "row" and val < 1.5):   # the 1 + 1e-9 rows stay in the regime
            want_rg[b] = 1 - after
    if not closed:
        want_cl[:] = 0
    assert np.array_equal(one["in_regime"], want_rg)
    assert np.array_equal(two["in_regime"], want_rg)
    assert np.array_equal(one["closed"], want_cl) and np.all(two["closed"] == 0)
    if closed:   # unedited sequences sharing a wave with an edited one: closed everywhere
        S = db.L.S
        shared = [b for b in range(Bc) if b not in edits and any(e // S == b // S for e in edits)]
        assert shared or S == 1
        assert np.all(one["closed"][shared] == 1)
    op = want_cl == 0
    for what in ("cum_ftrl", "cum_exact", "comp", "comp_ftl", "ftrl", "exact"):
        assert np.array_equal(one[what][op], two[what][op]), what
    for what in ("cum_ftrl", "cum_exact", "action"):
        assert np.array_equal(one[what], two[what]), what
    # the oracle on the truncated input: the regime flags, and the closed pairs within the bar
    for k, t in enumerate(CERT_CHECKPOINTS):
        ref = [O.ftl_exact_closed_form(f.z[b, :t], f.y[b, :t]) for b in range(Bc)]
        assert np.array_equal(one["in_regime"][:, k], [int(r[3]) for r in ref]), t
        cl = want_cl[:, k] == 1
        assert close_closed(one["comp"][cl, k], np.array([r[1] for r in ref])[cl], t), (P, d, t)


# ------------------------------------------------------------------ 4. ties
def test_ties_leave_the_regime_at_the_prefix_they_occur(eng):
    """l1: the dyadic sequence whose two leading coordinates tie at prefix 6 (and the regime
    stays left); linf: the label-flip family, where S_0 returns to 0 at every even prefix.
    The regime columns are the oracle's on the truncated input."""
    d, Tt = 5, 12
    z = np.zeros((2, Tt, d))
    z[:, :, 0] = 0.5
    z[:, 3:, 0] = 0.0
    z[:, 3:, 1] = 0.5
    z[1] *= 0.5                       # a second sequence, same pattern at half the size
    y = np.ones((2, Tt))
    cks = list(range(Tt + 1))
    got = eng.ftrl_vs_exact_curve_batch(z, y, cks, norm="l1", lanes_per_seq=1, check_regime=False)
    want = np.array([[O.ftl_exact_poly(z[b, :t], y[b, :t], "l1")[3] for t in cks]
                     for b in range(2)])
    assert np.array_equal(got["in_regime"], want)
    assert list(want[0]) == [True] * 6 + [False] * 7
    zf, yf, _ = O.flip_sequence(Tt, d)
    zf = np.asarray(zf, dtype=np.float64)[None]
    yf = np.asarray(yf, dtype=np.float64)[None]
    for lanes in (1, -4):
        got = eng.ftrl_vs_exact_curve_batch(zf, yf, cks, norm="linf", lanes_per_seq=lanes,
                                            check_regime=False)
        want = np.array([[O.ftl_exact_poly(zf[0, :t], yf[0, :t], "linf")[3] for t in cks]])
        assert np.array_equal(got["in_regime"], want)
        assert not want[0, 2:].any() and want[0, :2].all()


# ------------------------------------------------------------------ 5. general-solver fill
GEN_CKS = [0, 1, 7, 40]
GEN_KEYS = ("ftrl", "exact", "cum_exact", "comp", "action")


def general_case(half):
    f = F.make("gt_like", 6, 40, 3, 4242)
    z = f.z.copy()
    if half:
        z[::2] *= 2.0
    else:
        z *= 2.0
    return z, f.y


@pytest.mark.parametrize("norm", ("l2", "linf"))
def test_general_fill_equals_truncated_calls(eng, norm):
    import torch
    z, y = general_case(False)
    got = eng.ftrl_vs_exact_curve_batch(z, y, GEN_CKS, norm=norm)
    assert got["exact_gap_max"] > 0.0 and not got["in_regime"][:, 2:].any()
    db = eng.DeviceBatch(6, 40, 3).pack(z, y)
    dev = host(db.ftrl_vs_exact_curve_general(GEN_CKS, norm=norm, with_actions=True))
    assert db.exact_gap_max > 0.0
    for k, t in enumerate(GEN_CKS):
        ref = eng.ftrl_vs_exact_batch(z[:, :t], y[:, :t], norm=norm)
        for key in GEN_KEYS:
            assert np.array_equal(got[key][:, k], ref[key]), (norm, t, key)
            assert np.array_equal(dev[key][:, k], ref[key]), (norm, t, key, "device")
        assert np.array_equal(got["in_regime"][:, k], ref["in_regime"])
    torch.cuda.synchronize()


def test_general_fill_changes_only_the_pairs_outside_the_regime(eng):
    z, y = general_case(True)
    raw = eng.ftrl_vs_exact_curve_batch(z, y, GEN_CKS, check_regime=False)
    got = eng.ftrl_vs_exact_curve_batch(z, y, GEN_CKS)
    assert np.array_equal(raw["in_regime"], got["in_regime"])
    ok = got["in_regime"]
    assert ok[1::2].all() and not ok[::2, 2:].any() and ok[:, 0].all()
    for key in GEN_KEYS + ("cum_ftrl",):
        assert np.array_equal(raw[key][ok], got[key][ok]), key
    assert not np.array_equal(raw["comp"][~ok], got["comp"][~ok])
    for k, t in enumerate(GEN_CKS):
        ref = eng.ftrl_vs_exact_batch(z[:, :t], y[:, :t])
        for key in GEN_KEYS:
            assert np.array_equal(got[key][:, k], ref[key]), (t, key)


# ------------------------------------------------------------------ 6. drivers
@pytest.mark.parametrize("norm", ("l2", "linf"))
@pytest.mark.parametrize("title", ("Label flips", "Switching leaders"))
def test_driver_curves_are_the_reference_numbers_for_deterministic_families(eng, title, norm):
    from online_convex_optimization_amd import drivers
    grid = [10, 20, 40]
    got = drivers.exact_case_regret_curves(title, grid, runs=1, replicates=1, norm=norm)
    for k, t in enumerate(grid):
        ref = drivers.exact_case_regrets(title, t, runs=1, replicates=1, norm=norm)
        for key in drivers.EXACT_ALGOS:
            assert got[key].shape == (1, 3)
            assert np.array_equal(got[key][:, k], ref[key]), (title, norm, t, key)


def test_driver_curve_of_a_random_family_is_the_anytime_regret(eng):
    import torch
    from online_convex_optimization_amd import drivers
    title, grid, runs, reps = "Random i.i.d. (separable)", [10, 20, 40], 2, 2
    got = drivers.exact_case_regret_curves(title, grid, runs=runs, replicates=reps)
    family_, stream0 = drivers.CASE_FAMILIES[title]
    n = runs * reps
    db = eng.DeviceBatch(n, 40, 5, lanes_per_seq=1)
    run_idx = np.repeat(np.arange(runs), reps)
    db.generate_family(family_, 2025 * (run_idx + 1), stream0 + np.tile(np.arange(reps), runs))
    zz, yy = db.rows_of(torch.arange(n, device=db.device))
    z, y = zz.cpu().numpy(), yy.cpu().numpy()
    for k, t in enumerate(grid):
        ref = eng.ftrl_vs_exact_batch(z[:, :t], y[:, :t], lanes_per_seq=1)
        assert np.array_equal(got["FTRL"][:, k], ref["ftrl"]), t
        assert np.array_equal(got["FTL (exact)"][:, k], ref["exact"]), t
    cur = host(db.ftrl_vs_exact_curve(grid))
    cmp_ = host(db.exact_comparison_curves(grid))
    assert sorted(cmp_) == ["FTL (exact)", "FTRL"]
    assert np.array_equal(cmp_["FTRL"], cur["ftrl"])
    assert np.array_equal(cmp_["FTL (exact)"], cur["exact"])


# ------------------------------------------------------------------ 7. misc
@pytest.mark.parametrize("P,d,norm", [(8, 64, "l2"), (1, 5, "l2"), (-4, 5, "linf")])
def test_bad_device_checkpoints_write_nothing_outside(eng, P, d, norm):
    """An unordered, repeated, out-of-range DEVICE checkpoint array (the caller's precondition
    broken): the numbers are meaningless, but nothing outside the outputs and the workspace is
    written — every buffer sits between guard words that must survive."""
    import torch
    from online_convex_optimization_amd import _lib
    lib = _lib.load()
    f, _, _ = F.cert_case(64) if d == 64 else (family("gt_like", 5, 37, 130), None, None)
    Bc, Tc = f.y.shape
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    ck = torch.tensor([300, -5, 7, 7, 2, 1 << 40, Tc, -(1 << 40)], dtype=torch.int64,
                      device=db.device)
    K, G = int(ck.numel()), 64
    need = lib.ocx_ftrl_exact_curve_workspace_bytes(ctypes.byref(db.L), K, 1)
    assert need > 0 and need % 8 == 0

    def guarded(n, dtype, fill):
        t = torch.full((n + 2 * G,), fill, dtype=dtype, device=db.device)
        return t, t[G:G + n]

    bufs = {k: guarded(Bc * K, torch.float64, -7.25)
            for k in ("cum_ftrl", "cum_exact", "comp", "comp_ftl")}
    bufs["action"] = guarded(Bc * K * d, torch.float64, -7.25)
    bufs["regime"] = guarded(Bc * K, torch.int32, -77)
    bufs["closed"] = guarded(Bc * K, torch.int32, -77)
    bufs["ws"] = guarded(need // 8, torch.float64, -7.25)
    for flags in (0, _lib.OCX_ALG_CLOSED_COMPARATOR):
        rc = lib.ocx_dev_ftrl_vs_exact_curve(
            ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), f.eta0, ck.data_ptr(), K,
            bufs["cum_ftrl"][1].data_ptr(), bufs["cum_exact"][1].data_ptr(),
            bufs["comp"][1].data_ptr(), bufs["comp_ftl"][1].data_ptr(),
            bufs["action"][1].data_ptr(), bufs["regime"][1].data_ptr(),
            bufs["closed"][1].data_ptr(), eng._norm_code(norm), flags, bufs["ws"][1].data_ptr(),
            need, ctypes.c_void_p(torch.cuda.current_stream(db.device).cuda_stream))
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        for name, (whole, _) in bufs.items():
            fill = -77 if whole.dtype == torch.int32 else -7.25
            assert bool((whole[:G] == fill).all()) and bool((whole[-G:] == fill).all()), name
    # every output word was written (K emissions per sequence whatever the list holds)
    assert not bool((bufs["regime"][1] == -77).any()) and not bool((bufs["closed"][1] == -77).any())
    assert not bool((bufs["cum_ftrl"][1] == -7.25).any())


def test_degenerate_horizons(eng):
    f = family("gt_like", 5)
    # K = 1 with [T]: the whole-horizon call, in an exact and in the default layout
    for lanes in (1, eng.LANES_BEST):
        got = eng.ftrl_vs_exact_curve_batch(f.z, f.y, [T], f.eta0, lanes_per_seq=lanes,
                                            with_ftl_comparator=True)
        ref = eng.ftrl_vs_exact_batch(f.z, f.y, f.eta0, lanes_per_seq=lanes,
                                      with_ftl_comparator=True)
        for key in KEYS + ("ftrl", "exact"):
            assert np.array_equal(got[key][:, 0], ref[key]), (lanes, key)
        assert np.all(got["closed"] == (0 if lanes == 1 else 1))
    # T = 0 with [0]
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    for lanes in (1, 0):
        for norm in ("l2", "l1", "linf"):
            got = eng.ftrl_vs_exact_curve_batch(z0, y0, [0], lanes_per_seq=lanes, norm=norm,
                                                with_ftl_comparator=True)
            for key in ("ftrl", "exact", "cum_ftrl", "cum_exact", "comp", "comp_ftl", "action"):
                assert np.all(got[key] == 0.0), (lanes, norm, key)
            assert got["in_regime"].all() and got["exact_gap_max"] == 0.0
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).ftrl_vs_exact_curve([0]))
    assert all(np.all(out[k] == 0.0) for k in ("ftrl", "exact", "cum_ftrl", "cum_exact", "comp"))
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    assert all(v.shape[:2] == (B, 0) for v in host(db.ftrl_vs_exact_curve([])).values())
