"""The one-wave-per-sequence form of the two SMART sweeps (ocx_smart_wave_cols_kernel, through
ocx_test_simulate_smart_wave_cols = DeviceBatch.simulate_smart_thresholds / simulate_smart_curve
with ``_wave=group``, and through the product dispatch in the exact layouts), and the
single-threshold call on the kernel it was written from (ocx_smart_wave_kernel, under
OCX_SMART_KERNEL=wave), with which it shares its ordered adder (csrc/ocx_smart_wave.h).

The kernel adds in the reference's order whatever the layout, so every comparison is
np.array_equal on regrets and switch steps against the C oracle (or, where a case says so,
against the existing single-threshold call): this mode is bit-exact or wrong, there are no
tolerances.  Inputs: tests/_thresholds_cases.py, tests/_smart_curve_cases.py,
tests/_smart_wave_cols_cases.py and tests/_smart_wave_single_cases.py (conditions asserted in
tests/test_smart_wave_cols_cpu.py)."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import _smart_curve_cases as CC
from tests import _smart_wave_cols_cases as W
from tests import _smart_wave_single_cases as S
from tests import _thresholds_cases as C

pytestmark = pytest.mark.gpu

B, T, SQ2 = C.B, C.T, C.SQ2
TH7, M7 = C.TH7, len(C.TH7)
CK7, TH7C = CC.CK7, CC.TH7C
GROUPS = (1, 2, 4, 8)     # 7 columns: tail launches at 2 and 4, a spare column at 8
EXACT_LAYOUTS = (1, -1, -4)


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    _lib.load()
    return engine


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def new_stats(db):
    import torch
    return torch.zeros(2, dtype=torch.int64, device=db.device)


def packed(eng, z, y, P):
    Bn, Tn, d = z.shape
    db = eng.DeviceBatch(Bn, Tn, d, lanes_per_seq=P)
    return db.pack(z, y) if Tn else db


def assert_columns(got, want_reg, want_sw, what):
    assert got["regret"].shape == got["switch_step"].shape == want_reg.shape, what
    for m in range(want_reg.shape[1]):
        assert np.array_equal(got["switch_step"][:, m], want_sw[:, m]), (*what, m, "switch_step")
        assert np.array_equal(got["regret"][:, m], want_reg[:, m]), (*what, m, "regret")


def single_wave(db, th, monkeypatch):
    """(regret [B], switch_step [B]) of the single-threshold call on ocx_smart_wave_kernel."""
    import torch
    Bn = int(db.L.B)
    sw = torch.full((Bn,), -7, dtype=torch.int64, device=db.device)
    with monkeypatch.context() as mp:
        mp.setenv("OCX_SMART_KERNEL", "wave")   # read at every call
        reg = db.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=False,
                                closed_comparator=False)
        torch.cuda.synchronize()
    return reg[:Bn].cpu().numpy().copy(), sw.cpu().numpy()


# ------------------------------------------------------------------ 1. thresholds vs the oracle
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("d", W.DIMS)
@pytest.mark.parametrize("P", EXACT_LAYOUTS)
def test_thresholds_equal_the_oracle(eng, P, d, name):
    f = C.family(name, d)
    want_reg, want_sw = C.oracle_columns(name, d)
    ftl = O.simulate_alg_batch(f.z, f.y, 1, SQ2, nthreads=4)[0]
    db = packed(eng, f.z, f.y, P)
    for group in GROUPS:
        got = host(db.simulate_smart_thresholds(TH7, SQ2, _wave=group))
        assert got["switch_step"].dtype == np.int64
        assert_columns(got, want_reg, want_sw, (P, d, name, group))
        # +inf never switches: FTL's regret, the same adds and the same comparator
        assert np.array_equal(got["regret"][:, C.INF_COL], ftl), (P, d, name, group)
        assert np.all(got["switch_step"][:, C.INF_COL] == -1)
        for k in ("regret", "switch_step"):
            assert np.array_equal(got[k][:, C.DUP_COLS[0]], got[k][:, C.DUP_COLS[1]])
            # the columns are different runs
            assert len({got[k][:, m].tobytes() for m in range(M7)}) == 6, (P, d, name, group, k)


# ------------------------------------------------------------------ 2. curves on truncated rows
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("d", W.DIMS)
@pytest.mark.parametrize("P", EXACT_LAYOUTS)
def test_curves_equal_the_oracle_on_truncated_rows(eng, P, d, name):
    f = C.family(name, d)
    db = packed(eng, f.z, f.y, P)
    for hz, th, (want_reg, want_sw) in ((CK7, TH7C, CC.oracle_curve(name, d)),
                                        (W.HZ9, W.TH9, W.oracle_curve9(name, d))):
        for group in GROUPS:
            got = host(db.simulate_smart_curve(hz, th, SQ2, _wave=group))
            assert_columns(got, want_reg, want_sw, (P, d, name, group, len(hz)))
            sw = got["switch_step"]
            assert np.all((sw == -1) | ((sw >= 0) & (sw < np.array(hz)[None, :])))
    # h = 0: regret 0.0 and no switch, whatever the threshold
    assert np.all(got["regret"][:, 0] == 0.0) and np.all(got["switch_step"][:, 0] == -1)


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-4, 16), (-1, 64)])
def test_equal_horizons_are_the_threshold_sweep(eng, P, d, name):
    f = C.family(name, d)
    db = packed(eng, f.z, f.y, P)
    for group in GROUPS:
        want = host(db.simulate_smart_thresholds(TH7, SQ2, _wave=group))
        got = host(db.simulate_smart_curve([T] * M7, TH7, SQ2, _wave=group))
        assert np.array_equal(got["switch_step"], want["switch_step"]), (P, d, name, group)
        assert np.array_equal(got["regret"], want["regret"]), (P, d, name, group)
    assert_columns(got, *C.oracle_columns(name, d), (P, d, name))


# ------------------------------------------------------------------ 3. batch edges
@pytest.mark.parametrize("Bn,Tn,d", [(19, 120, 12), (70, 200, 5), (5, 130, 64), (3, 0, 4),
                                     (9, 65, 1)])
def test_batch_edges(eng, Bn, Tn, d):
    """The inputs of tests/test_gpu_parity.py test_smart_batch_splits (its generator and seed
    rule) with a per-sequence threshold matrix: B not a multiple of the four waves of a block,
    T = 0, d = 1."""
    rng = np.random.default_rng(5 + d)
    z = rng.standard_normal((Bn, Tn, d))
    z /= np.maximum(1.0, np.linalg.norm(z, axis=2, keepdims=True))
    y = np.where(rng.random((Bn, Tn)) < 0.5, -1.0, 1.0)
    th = rng.uniform(-1.0, 6.0, size=(Bn, 5))
    cols = [O.simulate_smart_batch(z, y, th[:, m].copy(), SQ2, nthreads=4) for m in range(5)]
    want_reg = np.stack([c[0] for c in cols], axis=1)
    want_sw = np.stack([c[1] for c in cols], axis=1)
    assert Tn == 0 or len(set(want_sw.ravel().tolist())) > 5   # a mix of switch steps
    for P in EXACT_LAYOUTS:
        db = packed(eng, z, y, P)
        for group in GROUPS:
            got = host(db.simulate_smart_thresholds(th, SQ2, _wave=group))
            assert_columns(got, want_reg, want_sw, (Bn, Tn, d, P, group))
    if Tn == 0:
        assert np.all(got["regret"] == 0.0) and np.all(got["switch_step"] == -1)


# ------------------------------------------------------------------ 4. butterfly layout
@pytest.mark.parametrize("name", C.FAMILIES)
def test_butterfly_layout_sums_in_the_reference_order(eng, monkeypatch, name):
    d = 64
    f = C.family(name, d)
    db = packed(eng, f.z, f.y, 8)
    assert (db.L.P, db.L.C, db.L.chain) == (8, 8, 0) and not db.exact
    want_reg, want_sw = C.oracle_columns(name, d)
    singles = [single_wave(db, th, monkeypatch) for th in TH7]
    for group in GROUPS:
        got = host(db.simulate_smart_thresholds(TH7, SQ2, _wave=group))
        assert_columns(got, want_reg, want_sw, (name, group))
        for m in range(M7):
            assert np.array_equal(got["regret"][:, m], singles[m][0]), (name, group, m)
            assert np.array_equal(got["switch_step"][:, m], singles[m][1]), (name, group, m)
        got = host(db.simulate_smart_curve(CK7, TH7C, SQ2, _wave=group))
        assert_columns(got, *CC.oracle_curve(name, d), (name, group, "curve"))


# ------------------------------------------------------------------ 5. the re-scan is shared
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-4, 16), (8, 64)])
def test_one_switch_test_per_step_serves_every_column(eng, P, d, name):
    f = C.family(name, d)
    db = packed(eng, f.z, f.y, P)
    th_sw = C.oracle_columns(name, d)[1]
    cv_sw = CC.oracle_curve(name, d)[1]
    pre_th = C.pre_switch_steps(th_sw, T)       # [B, 7]
    pre_cv = CC.pre_switch_steps(cv_sw, CK7)    # [B, 7]
    for group in GROUPS:
        for what, pre, want_sw, run in (
                ("thresholds", pre_th, th_sw,
                 lambda st: db.simulate_smart_thresholds(TH7, SQ2, stats=st, _wave=group)),
                ("curve", pre_cv, cv_sw,
                 lambda st: db.simulate_smart_curve(CK7, TH7C, SQ2, stats=st, _wave=group))):
            st = new_stats(db)
            got = host(run(st))
            assert np.array_equal(got["switch_step"], want_sw), (P, d, name, group, what)
            want = sum(int(pre[:, k0:k0 + group].max(axis=1).sum())
                       for k0 in range(0, M7, group))
            stv = st.cpu().numpy()
            print("switch tests", what, P, d, name, group, int(stv[0]), want)
            assert stv[0] == want and stv[1] == 0, (P, d, name, group, what, stv, want)


# ------------------------------------------------------------------ 6. non-finite thresholds
def test_non_finite_thresholds(eng):
    """The inputs of tests/test_gpu_thresholds.py
    test_non_finite_thresholds_decide_without_rescan: the comparison is the single kernel's,
    with no special case."""
    Bn, Tn, d = 4, 300, 8
    th = [np.inf, -np.inf, np.nan, 1e300]
    db = eng.DeviceBatch(Bn, Tn, d, lanes_per_seq=1).generate_gT(base_seed=5)
    for group in GROUPS + (None,):
        got = host(db.simulate_smart_thresholds(th, SQ2, _wave=group))
        for b in range(Bn):
            assert list(got["switch_step"][b]) == [-1, 0, -1, -1], (group, b)
            z, y = O.gT_sample(5, Tn, b, d)
            for m, t in enumerate(th):
                ref, rsw = O.simulate_SMART_like(z, y, float(t), SQ2, return_switch=True)
                assert got["regret"][b, m] == ref and got["switch_step"][b, m] == rsw, \
                    (group, b, m)


# ------------------------------------------------------------------ 7. dispatch
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-1, 9), (-4, 16), (1, 64)])
def test_public_calls_in_exact_layouts(eng, monkeypatch, P, d, name):
    f = C.family(name, d)
    db = packed(eng, f.z, f.y, P)
    assert db.exact
    calls = (("thresholds", lambda **kw: db.simulate_smart_thresholds(TH7, SQ2, **kw)),
             ("curve", lambda **kw: db.simulate_smart_curve(W.HZ9, W.TH9, SQ2, **kw)))
    for what, run in calls:
        pub = host(run())
        for group in GROUPS:
            got = host(run(_wave=group))
            assert all(np.array_equal(pub[k], got[k]) for k in pub), (P, d, name, what, group)
        lanes = host(run(_group=1))   # the lane-group form
        assert all(np.array_equal(pub[k], lanes[k]) for k in pub), (P, d, name, what, "lanes")
        with monkeypatch.context() as mp:
            mp.setenv("OCX_SMART_KERNEL", "lanes")   # read at every call
            held = host(run())
        assert all(np.array_equal(pub[k], held[k]) for k in pub), (P, d, name, what, "env")


# ------------------------------------------------------------------ 8. the single call
@pytest.mark.parametrize("Tn", S.HORIZONS)
@pytest.mark.parametrize("d", S.DIMS)
def test_single_call_equals_the_oracle(eng, monkeypatch, d, Tn):
    """simulate_smart under OCX_SMART_KERNEL=wave (ocx_launch_smart_wave:
    ocx_smart_wave_kernel<8> at d = 8, <0> at d = 9) with per-sequence thresholds, with and
    without a switch_step tensor.  tests/test_smart_wave_cols_cpu.py asserts that the
    oracle's switch steps at T = 67 hit every position of a speculated group, the last group
    and -1."""
    import torch
    z, y, th = S.inputs(d)
    want_reg, want_sw = S.oracle(d, Tn)
    z, y = np.ascontiguousarray(z[:, :Tn]), np.ascontiguousarray(y[:, :Tn])
    monkeypatch.setenv("OCX_SMART_KERNEL", "wave")   # read at every call
    for P in S.LAYOUTS:
        db = packed(eng, z, y, P)
        sw = torch.full((S.B,), -7, dtype=torch.int64, device=db.device)
        for sw_arg in (sw, None):
            db.regret.fill_(7.0)
            reg = db.simulate_smart(th, SQ2, switch_step=sw_arg, closed_prefix=False,
                                    closed_comparator=False)
            torch.cuda.synchronize()
            assert np.array_equal(reg[:S.B].cpu().numpy(), want_reg), (d, Tn, P, sw_arg is None)
        assert np.array_equal(sw.cpu().numpy(), want_sw), (d, Tn, P)


def test_argument_checks(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = C.family("beam", 5)
    db = packed(eng, f.z, f.y, 1)
    for bad in (0, 3, 5, 16, -1):
        with pytest.raises(ValueError, match="group must be 1, 2, 4 or 8"):
            db.simulate_smart_thresholds(TH7, SQ2, _wave=bad)
        with pytest.raises(ValueError, match="group must be 1, 2, 4 or 8"):
            db.simulate_smart_curve(CK7, TH7C, SQ2, _wave=bad)
    # the wave form is the re-scan mode's
    with pytest.raises(ValueError):
        db.simulate_smart_thresholds(TH7, SQ2, closed_prefix=True, _wave=2)
    with pytest.raises(ValueError):
        db.simulate_smart_curve(CK7, TH7C, SQ2, _group=2, _wave=2)
    # d > 64
    f100 = C.family("beam", 100)
    db100 = packed(eng, f100.z, f100.y, 1)
    with pytest.raises(_lib.OCXError, match="unsupported"):
        db100.simulate_smart_thresholds(TH7, SQ2, _wave=4)
    with pytest.raises(_lib.OCXError, match="unsupported"):
        db100.simulate_smart_curve(CK7, TH7C, SQ2, _wave=1)
    # decreasing horizons, in the C call itself; nothing is launched
    hz_bad = np.array([9, 3], dtype=np.int64)
    th = torch.zeros((B, 2), dtype=torch.float64, device=db.device)
    reg = torch.full((B, 2), 7.0, dtype=torch.float64, device=db.device)

    def call(hz, M=2, thp=th.data_ptr(), regp=reg.data_ptr(), group=2):
        with torch.cuda.device(db.device):
            _lib.call("ocx_test_simulate_smart_wave_cols", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), hz.ctypes.data_as(_lib.c_i64p), thp, M, SQ2, regp, None,
                      None, group, db._sp)

    with pytest.raises(ValueError, match="non-decreasing"):
        call(hz_bad)
    with pytest.raises(ValueError, match="outside"):
        call(np.array([3, T + 1], dtype=np.int64))
    with pytest.raises(ValueError, match="M < 0"):
        call(hz_bad, M=-1)
    with pytest.raises(ValueError, match="NULL"):
        call(hz_bad[::-1].copy(), regp=None)
    with pytest.raises(ValueError, match="NULL"):
        call(hz_bad[::-1].copy(), thp=None)
    torch.cuda.synchronize()
    assert bool((reg == 7.0).all())
    call(hz_bad[::-1].copy())       # the same call with legal horizons runs
    torch.cuda.synchronize()
    assert not bool((reg == 7.0).any())
    # M = 0
    out = host(db.simulate_smart_thresholds([], SQ2, _wave=4))
    assert all(v.shape == (B, 0) for v in out.values())
