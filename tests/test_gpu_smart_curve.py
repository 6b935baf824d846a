"""SMART regret curves (ocx_dev_simulate_smart_curve and the layers above it): SMART for K
(horizon, threshold) pairs in passes over z that each serve a group of consecutive pairs and
stop at the group's last horizon.

Bit for bit against the C oracle on truncated rows in the exact modes, and bit for bit per
column against DeviceBatch.simulate_smart(..., stats=...) — the threshold sweep kernel's
one-column instance — on a DeviceBatch packed with the first t_k rows, for every layout, every
forced group size and every flag pair.  CK7 / TH7C (tests/_smart_curve_cases.py, conditions
asserted in tests/test_smart_curve_cpu.py) put every MID column's horizon in the middle of its
switch steps."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F
from tests import _smart_curve_cases as C
from tests import _thresholds_cases as TC

pytestmark = pytest.mark.gpu

B, T = C.B, C.T
SQ2 = C.SQ2
CK7, TH7C = C.CK7, C.TH7C
K7 = len(CK7)


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


def single(db, th, pf, cc):
    """(regret [B], switch_step [B], stats [2]) of the single-threshold call with a stats
    tensor on the packed batch: the sweep kernel's one-column instance in the batch's own
    layout, for every flag pair; th scalar or [B]."""
    import torch
    Bn = int(db.L.B)
    sw = torch.full((Bn,), -7, dtype=torch.int64, device=db.device)
    st = new_stats(db)
    reg = db.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=pf, closed_comparator=cc,
                            stats=st)
    torch.cuda.synchronize()
    return reg[:Bn].cpu().numpy().copy(), sw.cpu().numpy(), st.cpu().numpy()


def truncated(eng, z, y, P, horizons, ths, pf, cc, full=None, dbs=None):
    """[B, K] regret and switch_step, and the summed stats, of K single-threshold calls, call
    k on a DeviceBatch packed with the first horizons[k] rows; ths[k] scalar or [B].  With
    `full`, asserts that every truncated batch has the full batch's layout.  `dbs` (a dict)
    keeps the truncated batches between calls."""
    Bn, _, d = z.shape
    dbs = {} if dbs is None else dbs
    cols = []
    for t, th in zip(horizons, ths):
        if t not in dbs:
            dbs[t] = eng.DeviceBatch(Bn, t, d, lanes_per_seq=P)
            if t:
                dbs[t].pack(z[:, :t], y[:, :t])
            if full is not None:
                assert (dbs[t].L.P, dbs[t].L.C, dbs[t].L.chain) == \
                    (full.L.P, full.L.C, full.L.chain), (P, d, t)
        cols.append(single(dbs[t], th, pf, cc))
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1),
            sum(c[2] for c in cols))


def has_instance(C_lane, group):
    return group == 1 or C_lane <= 8 or (group == 2 and C_lane <= 16)


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100)]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle_on_truncated_rows(eng, P, d, name):
    f = C.family(name, d)
    want_reg, want_sw = C.oracle_curve(name, d)
    reg, sw = eng.simulate_smart_curve_batch(f.z, f.y, CK7, TH7C, lanes_per_seq=P,
                                             return_switch=True)
    assert reg.shape == sw.shape == (B, K7) and sw.dtype == np.int64
    for k in range(K7):
        assert np.array_equal(sw[:, k], want_sw[:, k]), (P, d, name, k, "switch_step")
        assert np.array_equal(reg[:, k], want_reg[:, k]), (P, d, name, k, "regret")
    assert np.array_equal(eng.simulate_smart_curve_batch(f.z, f.y, CK7, TH7C, lanes_per_seq=P),
                          reg)


# ------------------------------------------------------------------ 2. every layout, every group
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 5), (-4, 16), (1, 64)]
FLAG_PAIRS = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_columns_equal_the_existing_kernel_on_truncated_batches(eng, P, d, name):
    from online_convex_optimization_amd import _lib
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    Cl = int(db.L.C)
    dbs = {}
    for pf, cc in FLAG_PAIRS:
        ref_reg, ref_sw, _ = truncated(eng, f.z, f.y, P, CK7, TH7C, pf, cc, full=db, dbs=dbs)
        ok = []
        for group in (1, 2, 4):
            try:
                got = host(db.simulate_smart_curve(CK7, TH7C, SQ2, closed_prefix=pf,
                                                   closed_comparator=cc, _group=group))
            except _lib.OCXError as e:
                assert not has_instance(Cl, group) and "unsupported" in str(e), \
                    (P, d, group, str(e))
                continue
            assert has_instance(Cl, group), (P, d, group)
            ok.append(group)
            for k in range(K7):
                assert np.array_equal(got["switch_step"][:, k], ref_sw[:, k]), \
                    (P, d, name, pf, cc, group, k, "switch_step")
                assert np.array_equal(got["regret"][:, k], ref_reg[:, k]), \
                    (P, d, name, pf, cc, group, k, "regret")
        pub = host(db.simulate_smart_curve(CK7, TH7C, SQ2, closed_prefix=pf, closed_comparator=cc))
        for key, ref in (("regret", ref_reg), ("switch_step", ref_sw)):
            for k in range(K7):
                assert np.array_equal(pub[key][:, k], ref[:, k]), (P, d, name, pf, cc, "public",
                                                                   k, key)
        assert _lib.load().ocx_smart_curve_group(ctypes.byref(db.L), K7) in ok
    sw = pub["switch_step"]
    assert np.all((sw == -1) | ((sw >= 0) & (sw < np.array(CK7)[None, :])))


# ------------------------------------------------------------------ 3. equal horizons
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (8, 64), (0, 5)])
def test_equal_horizons_are_the_threshold_sweep(eng, P, d, name):
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    want = host(db.simulate_smart_thresholds(TC.TH7, SQ2))
    groups = [None] + [g for g in (1, 2, 4) if has_instance(int(db.L.C), g)]
    for group in groups:
        got = host(db.simulate_smart_curve([T] * len(TC.TH7), TC.TH7, SQ2, _group=group))
        assert np.array_equal(got["switch_step"], want["switch_step"]), (P, d, name, group)
        assert np.array_equal(got["regret"], want["regret"]), (P, d, name, group)


# ------------------------------------------------------------------ 4. the re-scan is shared
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-4, 16)])
def test_one_rescan_per_step_stops_at_the_horizon(eng, P, d, name):
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert db.exact   # the oracle's switch steps are the layout's
    want_sw = C.oracle_curve(name, d)[1]
    pre = C.pre_switch_steps(want_sw, CK7)     # [B, K]
    ran = 0
    for group in (1, 2, 4):
        if not has_instance(int(db.L.C), group):
            continue
        ran += 1
        st = new_stats(db)
        got = host(db.simulate_smart_curve(CK7, TH7C, SQ2, closed_prefix=False,
                                           closed_comparator=False, stats=st, _group=group))
        assert np.array_equal(got["switch_step"], want_sw), (P, d, name, group)
        want = sum(int(pre[:, k0:k0 + group].max(axis=1).sum()) for k0 in range(0, K7, group))
        stv = st.cpu().numpy()
        print("rescans", P, d, name, group, int(stv[0]), want)
        assert stv[0] == want and stv[1] == 0, (P, d, name, group, stv, want)
    assert ran >= 2


# ------------------------------------------------------------------ 5. certificates per pair
CERT_HZ = [0, 1, 63, 64, 65, 129, 130]


def test_certificates_are_per_sequence_and_column(eng):
    P, d = 8, 64
    f, edits, _ = F.cert_case(d)
    Bc, Tc = f.y.shape
    assert (Bc, Tc) == (37, 130)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    # the pair (b, k) is clean if no edit of sequence b lies in its first t_k rows
    clean = np.ones((Bc, len(CERT_HZ)), dtype=bool)
    for b, (_, _, te) in edits.items():
        clean[b] = [te >= t for t in CERT_HZ]
    assert 0 < (~clean).sum() < clean.size
    plain = host(db.simulate_smart_curve(CERT_HZ, TH7C, SQ2, closed_prefix=False,
                                         closed_comparator=False))
    # the single-threshold call on the truncated batches: certified pairs keep its closed
    # value whatever shares their wave or group
    ref_reg, ref_sw, ref_st = truncated(eng, f.z, f.y, P, CERT_HZ, TH7C, True, True, full=db)
    assert ref_st[1] == clean.sum()
    for group in (1, 2, 4):
        st = new_stats(db)
        got = host(db.simulate_smart_curve(CERT_HZ, TH7C, SQ2, closed_prefix=True,
                                           closed_comparator=True, stats=st, _group=group))
        assert st.cpu().numpy()[1] == clean.sum(), (group, st.cpu().numpy(), clean.sum())
        assert np.array_equal(got["switch_step"], plain["switch_step"]), group
        # uncertified pairs stream the comparator: the flags-0 bits
        assert np.array_equal(got["regret"][~clean], plain["regret"][~clean]), group
        assert np.array_equal(got["regret"], ref_reg) and np.array_equal(got["switch_step"], ref_sw)
    S = db.L.S
    shared = [b for b in range(Bc) if b not in edits and any(e // S == b // S for e in edits)]
    assert shared
    # a certified pair (T/2 - ||theta||) differs from the streamed sum by rounding only, and on
    # these rows it does differ somewhere: the closed form was taken
    assert not np.array_equal(got["regret"][shared], plain["regret"][shared])
    assert np.allclose(got["regret"], plain["regret"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ 6. guard band
def test_guard_band_ties_keep_the_reference_steps_at_every_horizon(eng):
    z, y, _ = O.flip_sequence(TC.FLIP_T)
    z, y = z.astype(np.float64), y.astype(np.float64)
    pairs = [(h, float(th)) for h, ths in ((100, TC.FLIP_TH[53:57]), (200, TC.FLIP_TH[72:76]),
                                           (300, TC.FLIP_TH[76:80]), (400, TC.FLIP_TH[80:84]))
             for th in ths]
    hz = [p[0] for p in pairs]
    th = [p[1] for p in pairs]
    ref_reg, ref_sw = [], []
    for h, t in pairs:
        r, s = O.simulate_SMART_like(z[:h], y[:h], t, SQ2, return_switch=True)
        ref_reg.append(r)
        ref_sw.append(s)
    Bn = 3
    Z, Y = np.repeat(z[None], Bn, axis=0), np.repeat(y[None], Bn, axis=0)
    for lanes, pf in ((1, False), (1, True), (eng.LANES_BEST, True)):
        db = eng.DeviceBatch(Bn, TC.FLIP_T, z.shape[1], lanes_per_seq=lanes).pack(Z, Y)
        got = host(db.simulate_smart_curve(hz, th, SQ2, closed_prefix=pf,
                                           closed_comparator=False))
        for b in range(Bn):
            assert np.array_equal(got["switch_step"][b], ref_sw), (lanes, pf, b)
            if lanes == 1:
                assert np.array_equal(got["regret"][b], ref_reg), (lanes, pf, b)
    # the thresholds of horizon 100 straddle it: two switch before it, two would switch after
    assert ref_sw[:4].count(-1) == 2 and len(set(ref_sw)) >= 12


# ------------------------------------------------------------------ 7. degenerate cases
def test_degenerate_cases(eng):
    f = C.family("beam", 5)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    # K = 0, host and device
    reg, sw = eng.simulate_smart_curve_batch(f.z, f.y, [], [], lanes_per_seq=1, return_switch=True)
    assert reg.shape == sw.shape == (B, 0)
    assert all(v.shape == (B, 0) for v in host(db.simulate_smart_curve([], [])).values())
    # t_k = 0: zeros and -1, whatever the threshold; duplicates of it
    for lanes in (1, 0):
        reg, sw = eng.simulate_smart_curve_batch(f.z, f.y, [0, 0, 0, 5], [-1.0, 0.0, 2.0, -1.0],
                                                 lanes_per_seq=lanes, return_switch=True)
        assert np.all(reg[:, :3] == 0.0) and np.all(sw[:, :3] == -1) and np.all(sw[:, 3] == 0)
    # T = 0
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    reg, sw = eng.simulate_smart_curve_batch(z0, y0, [0, 0], [1.0, -1.0], lanes_per_seq=1,
                                             return_switch=True)
    assert reg.shape == (B, 2) and np.all(reg == 0.0) and np.all(sw == -1)
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_smart_curve([0] * 3))
    assert np.all(out["regret"] == 0.0) and np.all(out["switch_step"] == -1)
    # B = 1 and T = 1
    reg, sw = eng.simulate_smart_curve_batch(f.z[:1], f.y[:1], CK7, TH7C, lanes_per_seq=1,
                                             return_switch=True)
    for k, (t, th) in enumerate(zip(CK7, TH7C)):
        ref, rsw = O.simulate_SMART_like(f.z[0, :t], f.y[0, :t], th, SQ2, return_switch=True)
        assert (reg[0, k], sw[0, k]) == (ref, rsw), (t, th)
    reg, sw = eng.simulate_smart_curve_batch(f.z[:, :1], f.y[:, :1], [0, 1, 1], [-1.0, -1.0, 9.0],
                                             lanes_per_seq=1, return_switch=True)
    want = [O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :1]),
                                   np.ascontiguousarray(f.y[:, :1]), np.full(B, th), SQ2, nthreads=4)
            for th in (-1.0, 9.0)]
    assert np.all(reg[:, 0] == 0.0) and np.all(sw[:, 0] == -1)
    for k, w in ((1, want[0]), (2, want[1])):
        assert np.array_equal(reg[:, k], w[0]) and np.array_equal(sw[:, k], w[1])
    # NaN and -inf thresholds; the default thresholds are sqrt(2 t_k)
    hz = [50, 50, 120, 257]
    got = host(db.simulate_smart_curve(hz, [np.nan, -np.inf, np.nan, -np.inf]))
    for k, t in enumerate(hz):
        w = O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                   np.ascontiguousarray(f.y[:, :t]),
                                   np.full(B, [np.nan, -np.inf][k % 2]), SQ2)
        assert np.array_equal(got["regret"][:, k], w[0]), k
        assert np.array_equal(got["switch_step"][:, k], w[1]), k
        assert np.all(got["switch_step"][:, k] == (-1 if k % 2 == 0 else 0))
    dflt = host(db.simulate_smart_curve(hz))
    expl = host(db.simulate_smart_curve(hz, [math.sqrt(2.0 * t) for t in hz]))
    assert all(np.array_equal(dflt[k], expl[k]) for k in dflt)
    # per-sequence thresholds [B, K]
    per = np.random.default_rng(3).uniform(-1.0, 6.0, size=(B, 3))
    got = host(db.simulate_smart_curve([40, 130, 257], per))
    for k, t in enumerate((40, 130, 257)):
        w = O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                   np.ascontiguousarray(f.y[:, :t]), per[:, k].copy(), SQ2)
        assert np.array_equal(got["regret"][:, k], w[0]), k
        assert np.array_equal(got["switch_step"][:, k], w[1]), k
    # a bad host list raises before any launch, in Python and in the C call
    for bad in ([5, 4], [0, T + 1], [-1], [[1, 2]], [True], [1.5], None):
        with pytest.raises(ValueError):
            eng.simulate_smart_curve_batch(f.z, f.y, bad, [1.0] * 2)
        with pytest.raises(ValueError):
            db.simulate_smart_curve(bad, [1.0] * 2)
    with pytest.raises(ValueError):
        db.simulate_smart_curve([1, 2, 3], [1.0, 2.0])   # one threshold per horizon
    from online_convex_optimization_amd import _lib
    import torch
    hz_bad = np.array([9, 3], dtype=np.int64)
    th = torch.zeros((B, 2), dtype=torch.float64, device=db.device)
    reg = torch.full((B, 2), 7.0, dtype=torch.float64, device=db.device)
    with pytest.raises(ValueError, match="non-decreasing"):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_curve", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), hz_bad.ctypes.data_as(_lib.c_i64p), th.data_ptr(), 2, SQ2,
                      reg.data_ptr(), None, 0, None, db._sp)
    torch.cuda.synchronize()
    assert bool((reg == 7.0).all())   # nothing was launched
    with pytest.raises(ValueError, match="unknown flags"):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_curve", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), hz_bad[::-1].copy().ctypes.data_as(_lib.c_i64p),
                      th.data_ptr(), 2, SQ2, reg.data_ptr(), None, 64, None, db._sp)


# ------------------------------------------------------------------ 8. capture
def test_device_call_is_capture_safe(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = C.family("gt_like", 64)
    s = torch.cuda.Stream()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=s).pack(f.z, f.y)
    assert (db.L.P, db.L.C) == (8, 8)
    tha = np.ascontiguousarray(np.broadcast_to(np.array(TH7C), (B, K7)))
    hz = np.array(CK7, dtype=np.int64)
    flags = _lib.OCX_SMART_CLOSED_PREFIX | _lib.OCX_ALG_CLOSED_COMPARATOR
    with torch.cuda.stream(s):
        th = torch.as_tensor(tha).to(db.device)

    def buffers():
        with torch.cuda.stream(s):
            return (torch.zeros((B, K7), dtype=torch.float64, device=db.device),
                    torch.full((B, K7), -7, dtype=torch.int64, device=db.device))

    def run(o):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_curve", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), hz.ctypes.data_as(_lib.c_i64p), th.data_ptr(), K7, SQ2,
                      o[0].data_ptr(), o[1].data_ptr(), flags, None,
                      ctypes.c_void_p(s.cuda_stream))

    eager, cap = buffers(), buffers()
    run(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(cap)
    torch.cuda.synchronize()
    for t in cap:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        assert torch.equal(a, b)
    assert not torch.equal(eager[1][:, 0], eager[1][:, 1])   # it did run, column by column
    ref_reg, ref_sw, _ = truncated(eng, f.z, f.y, 8, CK7, TH7C, True, True)
    assert np.array_equal(cap[0].cpu().numpy(), ref_reg)
    assert np.array_equal(cap[1].cpu().numpy(), ref_sw)


# ------------------------------------------------------------------ 9. the comparison figure
@pytest.mark.parametrize("name", C.FAMILIES)
def test_comparison_curves_equal_the_oracle(eng, name):
    d = 5
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=1).pack(f.z, f.y)
    g_emp = [0.5, 2.5, 3.5, 4.0, 5.5, 6.5, 7.5]
    got = host(db.comparison_curves(CK7, g_emp))
    assert sorted(got) == ["EMP", "FTL", "FTRL", "SMART"]
    assert all(v.shape == (B, K7) for v in got.values())
    for k, t in enumerate(CK7):
        zt, yt = np.ascontiguousarray(f.z[:, :t]), np.ascontiguousarray(f.y[:, :t])
        assert np.array_equal(got["FTRL"][:, k],
                              O.simulate_alg_batch(zt, yt, 0, SQ2, nthreads=4)[0]), (name, k)
        assert np.array_equal(got["FTL"][:, k],
                              O.simulate_alg_batch(zt, yt, 1, SQ2, nthreads=4)[0]), (name, k)
        for key, th in (("SMART", math.sqrt(2.0 * t)), ("EMP", g_emp[k])):
            want = O.simulate_smart_batch(zt, yt, np.full(B, th), SQ2, nthreads=4)[0]
            assert np.array_equal(got[key][:, k], want), (name, key, k)
    ftl = host(db.simulate_alg_curve(CK7, 1, SQ2))["regret"]
    assert np.array_equal(got["FTL"], ftl)
    assert sorted(host(db.comparison_curves(CK7))) == ["FTL", "FTRL", "SMART"]
    # different runs (on gt_like rows sqrt(2 t_k) is never reached: SMART there is FTL)
    assert len({got[k].tobytes() for k in ("FTRL", "FTL", "EMP")}) == 3
    with pytest.raises(ValueError):
        db.comparison_curves([1, 1, 2])          # strictly increasing
    with pytest.raises(ValueError):
        db.comparison_curves(CK7, g_emp[:3])
