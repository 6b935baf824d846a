"""SMART regret grids (ocx_dev_simulate_smart_grid and the layers above it): SMART for M
thresholds, each observed at K checkpoint horizons, in passes over z that each serve a group of
thresholds and run once, to the last checkpoint.

Bit for bit against the C oracle on truncated rows in the exact modes; bit for bit against the
existing DeviceBatch.simulate_smart_curve on the expanded pair list — and, for three layouts,
against DeviceBatch.simulate_smart(..., stats=...) on batches packed with the first t_k rows —
for every layout, every forced group size and every flag pair; the one-wave-per-sequence form
against the oracle and the lane-group grid.  There are no tolerances.  CK7 / THG7 and HZ9 / THG9
(tests/_smart_grid_cases.py, conditions asserted in tests/test_smart_grid_cpu.py) split a
column's switch steps at the interior checkpoints."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F
from tests import _smart_grid_cases as C
from tests import _thresholds_cases as TC
from tests.test_gpu_smart_curve import FLAG_PAIRS, LAYOUTS, has_instance, truncated

pytestmark = pytest.mark.gpu

B, T, SQ2 = C.B, C.T, C.SQ2
CK7, THG7, HZ9, THG9 = C.CK7, C.THG7, C.HZ9, C.THG9
K7, M7 = len(CK7), len(THG7)


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


def assert_grid(got, want_reg, want_sw, what):
    assert got["regret"].shape == got["switch_step"].shape == want_reg.shape, what
    for m in range(want_reg.shape[1]):
        for k in range(want_reg.shape[2]):
            assert np.array_equal(got["switch_step"][:, m, k], want_sw[:, m, k]), \
                (*what, m, k, "switch_step")
            assert np.array_equal(got["regret"][:, m, k], want_reg[:, m, k]), \
                (*what, m, k, "regret")


def pair_list(db, ck, ths, **kw):
    """The grid from the existing curve call on the M·K pairs sorted by horizon: regret and
    switch_step [B, M, K]."""
    hz, th = C.pairs(ck, ths)
    got = host(db.simulate_smart_curve(hz, th, SQ2, **kw))
    M, K = len(ths), len(ck)
    return {k: v.reshape(-1, K, M).transpose(0, 2, 1) for k, v in got.items()}


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100)]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle_on_truncated_rows(eng, P, d, name):
    f = C.family(name, d)
    want_reg, want_sw = C.oracle_grid(name, d, tuple(CK7), tuple(THG7))
    reg, sw = eng.simulate_smart_grid_batch(f.z, f.y, CK7, THG7, lanes_per_seq=P,
                                            return_switch=True)
    assert reg.shape == sw.shape == (B, M7, K7) and sw.dtype == np.int64
    assert_grid({"regret": reg, "switch_step": sw}, want_reg, want_sw, (P, d, name))
    assert np.array_equal(eng.simulate_smart_grid_batch(f.z, f.y, CK7, THG7, lanes_per_seq=P),
                          reg)


# ------------------------------------------------------------------ 2. every layout, every group
SINGLE_LAYOUTS = [(8, 64), (0, 5), (-4, 16)]   # also against the single call on packed prefixes


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_grid_equals_the_existing_curve_on_the_pair_list(eng, P, d, name):
    from online_convex_optimization_amd import _lib
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    Cl = int(db.L.C)
    dbs = {}
    for pf, cc in FLAG_PAIRS:
        ref = pair_list(db, CK7, THG7, closed_prefix=pf, closed_comparator=cc)
        if (P, d) in SINGLE_LAYOUTS:
            for m, th in enumerate(THG7):
                sreg, ssw, _ = truncated(eng, f.z, f.y, P, CK7, [th] * K7, pf, cc, full=db,
                                         dbs=dbs)
                assert np.array_equal(ref["regret"][:, m, :], sreg), (P, d, name, pf, cc, m)
                assert np.array_equal(ref["switch_step"][:, m, :], ssw), (P, d, name, pf, cc, m)
        ok = []
        for group in (1, 2, 4):
            try:
                got = host(db.simulate_smart_grid(CK7, THG7, SQ2, closed_prefix=pf,
                                                  closed_comparator=cc, _group=group))
            except _lib.OCXError as e:
                assert not has_instance(Cl, group) and "unsupported" in str(e), \
                    (P, d, group, str(e))
                continue
            assert has_instance(Cl, group), (P, d, group)
            ok.append(group)
            assert_grid(got, ref["regret"], ref["switch_step"], (P, d, name, pf, cc, group))
        pub = host(db.simulate_smart_grid(CK7, THG7, SQ2, closed_prefix=pf, closed_comparator=cc))
        assert_grid(pub, ref["regret"], ref["switch_step"], (P, d, name, pf, cc, "public"))
        assert _lib.load().ocx_smart_grid_group(ctypes.byref(db.L), M7) in ok
    # the duplicate columns agree; the others are different runs
    for key in ("regret", "switch_step"):
        assert np.array_equal(pub[key][:, C.DUP_COLS[0]], pub[key][:, C.DUP_COLS[1]])
        assert len({pub[key][:, m].tobytes() for m in range(M7)}) == M7 - 1, (P, d, name, key)


# ------------------------------------------------------------------ 3. slices
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (8, 64), (0, 5), (-4, 16)])
def test_slices_are_the_sweep_and_the_curve(eng, P, d, name):
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    sweep = host(db.simulate_smart_thresholds(THG7, SQ2))
    groups = [None] + [g for g in (1, 2, 4) if has_instance(int(db.L.C), g)]
    for group in groups:
        got = host(db.simulate_smart_grid(CK7, THG7, SQ2, _group=group))
        for key in ("regret", "switch_step"):
            assert np.array_equal(got[key][:, :, -1], sweep[key]), (P, d, name, group, key)
        s = sweep["switch_step"][:, :, None]
        t = np.array(CK7)[None, None, :]
        assert np.array_equal(got["switch_step"], np.where((s >= 0) & (s < t), s, -1))
        for m, th in enumerate(THG7):
            curve = host(db.simulate_smart_curve(CK7, [th] * K7, SQ2))
            for key in ("regret", "switch_step"):
                assert np.array_equal(got[key][:, m, :], curve[key]), (P, d, name, group, m, key)
    # +inf: FTL's regret at every horizon
    ftl = host(db.simulate_alg_curve(CK7, 1, SQ2, closed_comparator=not db.exact))["regret"]
    if db.exact:
        assert np.array_equal(got["regret"][:, C.INF_COL, :], ftl), (P, d, name)
    assert np.all(got["switch_step"][:, C.INF_COL, :] == -1)


# ------------------------------------------------------------------ 4. the re-scan is shared
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-4, 16)])
def test_one_rescan_per_step_for_all_columns_of_a_launch(eng, P, d, name):
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert db.exact   # the oracle's switch steps are the layout's
    full_sw = C.oracle_full(name, d, tuple(THG7))[1]
    ck = CK7[:-1]     # the last checkpoint before T: the count is capped at it
    pre = C.pre_switch_steps(full_sw, ck[-1])      # [B, M]
    ran = 0
    for group in (1, 2, 4):
        if not has_instance(int(db.L.C), group):
            continue
        ran += 1
        st = new_stats(db)
        got = host(db.simulate_smart_grid(ck, THG7, SQ2, closed_prefix=False,
                                          closed_comparator=False, stats=st, _group=group))
        assert np.array_equal(got["switch_step"], C.truncate_switch(full_sw, ck)), (P, d, group)
        want = sum(int(pre[:, m0:m0 + group].max(axis=1).sum()) for m0 in range(0, M7, group))
        stv = st.cpu().numpy()
        print("rescans", P, d, name, group, int(stv[0]), want)
        assert stv[0] == want and stv[1] == 0, (P, d, name, group, stv, want)
    assert ran >= 2


# ------------------------------------------------------------------ 5. certificates per pair
CERT_HZ = [0, 1, 63, 64, 65, 129, 130]


def test_certificates_are_per_sequence_and_checkpoint(eng):
    P, d = 8, 64
    f, edits, _ = F.cert_case(d)
    Bc, Tc = f.y.shape
    assert (Bc, Tc) == (37, 130)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.C, db.L.chain) == (P, 8, 0)
    # the pair (b, k) is clean if no edit of sequence b lies in its first t_k rows
    clean = np.ones((Bc, len(CERT_HZ)), dtype=bool)
    for b, (_, _, te) in edits.items():
        clean[b] = [te >= t for t in CERT_HZ]
    assert 0 < (~clean).sum() < clean.size
    plain = host(db.simulate_smart_grid(CERT_HZ, THG7, SQ2, closed_prefix=False,
                                        closed_comparator=False))
    ref = pair_list(db, CERT_HZ, THG7, closed_prefix=True, closed_comparator=True)
    cm = np.broadcast_to(clean[:, None, :], (Bc, M7, len(CERT_HZ)))
    for group in (1, 2, 4):
        st = new_stats(db)
        got = host(db.simulate_smart_grid(CERT_HZ, THG7, SQ2, closed_prefix=True,
                                          closed_comparator=True, stats=st, _group=group))
        # nt x (clean pairs), summed over the launches: M x (clean pairs)
        assert st.cpu().numpy()[1] == M7 * clean.sum(), (group, st.cpu().numpy(), clean.sum())
        assert np.array_equal(got["switch_step"], plain["switch_step"]), group
        # uncertified pairs stream the comparator: the flags-0 bits
        assert np.array_equal(got["regret"][~cm], plain["regret"][~cm]), group
        assert_grid(got, ref["regret"], ref["switch_step"], ("cert", group))
    S = db.L.S
    shared = [b for b in range(Bc) if b not in edits and any(e // S == b // S for e in edits)]
    assert shared
    # certified neighbours in the same wave keep the closed value: it differs from the streamed
    # sum by rounding only, and on these rows it does differ somewhere
    assert not np.array_equal(got["regret"][shared], plain["regret"][shared])
    assert np.allclose(got["regret"], plain["regret"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------ 6. guard band
def test_guard_band_ties_keep_the_reference_steps_at_every_horizon(eng):
    z, y, _ = O.flip_sequence(TC.FLIP_T)
    z, y = z.astype(np.float64), y.astype(np.float64)
    ck = [100, 200, 300, 400]
    ths = [float(t) for t in TC.FLIP_TH[72:80]]   # eight consecutive half-integers
    ref_reg = np.zeros((len(ths), len(ck)))
    ref_sw = np.zeros((len(ths), len(ck)), dtype=np.int64)
    for k, h in enumerate(ck):
        for m, th in enumerate(ths):
            ref_reg[m, k], ref_sw[m, k] = O.simulate_SMART_like(z[:h], y[:h], th, SQ2,
                                                                return_switch=True)
    Bn = 3
    Z, Y = np.repeat(z[None], Bn, axis=0), np.repeat(y[None], Bn, axis=0)
    for lanes, pf in ((1, False), (1, True), (eng.LANES_BEST, True)):
        db = eng.DeviceBatch(Bn, TC.FLIP_T, z.shape[1], lanes_per_seq=lanes).pack(Z, Y)
        got = host(db.simulate_smart_grid(ck, ths, SQ2, closed_prefix=pf,
                                          closed_comparator=False))
        for b in range(Bn):
            assert np.array_equal(got["switch_step"][b], ref_sw), (lanes, pf, b)
            if lanes == 1:
                assert np.array_equal(got["regret"][b], ref_reg), (lanes, pf, b)
    # the ties matter: the columns switch at different steps, some after the first checkpoints
    assert len(set(ref_sw[:, -1].tolist())) >= 6 and (ref_sw[:, 0] == -1).any()


# ------------------------------------------------------------------ 7. degenerate cases
def test_degenerate_cases(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = C.family("beam", 5)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    # M = 0 and K = 0, host and device
    reg, sw = eng.simulate_smart_grid_batch(f.z, f.y, [], THG7, lanes_per_seq=1,
                                            return_switch=True)
    assert reg.shape == sw.shape == (B, M7, 0)
    assert eng.simulate_smart_grid_batch(f.z, f.y, CK7, [], lanes_per_seq=1).shape == (B, 0, K7)
    assert all(v.shape == (B, M7, 0) for v in host(db.simulate_smart_grid([], THG7)).values())
    assert all(v.shape == (B, 0, K7) for v in host(db.simulate_smart_grid(CK7, [])).values())
    # t_1 = 0: zeros and -1, whatever the threshold
    for lanes in (1, 0):
        reg, sw = eng.simulate_smart_grid_batch(f.z, f.y, [0, 5], [-1.0, 0.0, 2.0, -np.inf],
                                                lanes_per_seq=lanes, return_switch=True)
        assert np.all(reg[:, :, 0] == 0.0) and np.all(sw[:, :, 0] == -1)
        assert np.all(sw[:, 0, 1] == 0) and np.all(sw[:, 3, 1] == 0)
    # T = 0
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    reg, sw = eng.simulate_smart_grid_batch(z0, y0, [0], [1.0, -1.0], lanes_per_seq=1,
                                            return_switch=True)
    assert reg.shape == (B, 2, 1) and np.all(reg == 0.0) and np.all(sw == -1)
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_smart_grid([0], THG7))
    assert np.all(out["regret"] == 0.0) and np.all(out["switch_step"] == -1)
    # B = 1
    reg, sw = eng.simulate_smart_grid_batch(f.z[:1], f.y[:1], CK7, THG7, lanes_per_seq=1,
                                            return_switch=True)
    for k, t in enumerate(CK7):
        for m, th in enumerate(THG7):
            ref, rsw = O.simulate_SMART_like(f.z[0, :t], f.y[0, :t], th, SQ2, return_switch=True)
            assert (reg[0, m, k], sw[0, m, k]) == (ref, rsw), (t, th)
    # T = 1
    z1, y1 = np.ascontiguousarray(f.z[:, :1]), np.ascontiguousarray(f.y[:, :1])
    reg, sw = eng.simulate_smart_grid_batch(z1, y1, [0, 1], [-1.0, 9.0], lanes_per_seq=1,
                                            return_switch=True)
    assert np.all(reg[:, :, 0] == 0.0) and np.all(sw[:, :, 0] == -1)
    for m, th in enumerate((-1.0, 9.0)):
        w = O.simulate_smart_batch(z1, y1, np.full(B, th), SQ2, nthreads=4)
        assert np.array_equal(reg[:, m, 1], w[0]) and np.array_equal(sw[:, m, 1], w[1])
    # NaN and ±inf thresholds
    ck = [50, 120, 257]
    ths = [np.nan, -np.inf, np.inf]
    got = host(db.simulate_smart_grid(ck, ths))
    for k, t in enumerate(ck):
        for m, th in enumerate(ths):
            w = O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                       np.ascontiguousarray(f.y[:, :t]), np.full(B, th), SQ2)
            assert np.array_equal(got["regret"][:, m, k], w[0]), (m, k)
            assert np.array_equal(got["switch_step"][:, m, k], w[1]), (m, k)
    assert np.all(got["switch_step"][:, 0] == -1) and np.all(got["switch_step"][:, 1] == 0)
    assert np.all(got["switch_step"][:, 2] == -1)
    # per-sequence thresholds [B, M]
    per = np.random.default_rng(3).uniform(-1.0, 6.0, size=(B, 3))
    got = host(db.simulate_smart_grid([40, 130, 257], per))
    for k, t in enumerate((40, 130, 257)):
        for m in range(3):
            w = O.simulate_smart_batch(np.ascontiguousarray(f.z[:, :t]),
                                       np.ascontiguousarray(f.y[:, :t]), per[:, m].copy(), SQ2)
            assert np.array_equal(got["regret"][:, m, k], w[0]), (m, k)
            assert np.array_equal(got["switch_step"][:, m, k], w[1]), (m, k)
    # a bad list raises with nothing launched: the output sentinel is left intact
    for bad in ([5, 4], [3, 3], [0, T + 1], [-1], [[1, 2]], [1.5], None):
        with pytest.raises(ValueError):
            eng.simulate_smart_grid_batch(f.z, f.y, bad, [1.0] * 2)
        with pytest.raises(ValueError):
            db.simulate_smart_grid(bad, [1.0] * 2)
    reg = np.full((B, 2, 2), 7.0)
    th = np.zeros((B, 2))
    bad = np.array([9, 3], dtype=np.int64)
    with pytest.raises(ValueError, match="strictly increasing"):
        _lib.call("ocx_simulate_smart_grid_batch", f.z.ctypes.data_as(_lib.c_dp),
                  f.y.ctypes.data_as(_lib.c_dp), B, T, 5, th.ctypes.data_as(_lib.c_dp), 2,
                  bad.ctypes.data_as(_lib.c_i64p), 2, SQ2, reg.ctypes.data_as(_lib.c_dp), None,
                  1, 0)
    assert np.all(reg == 7.0)
    # unknown flags: nothing launched
    thd = torch.zeros((B, 2), dtype=torch.float64, device=db.device)
    ckd = torch.as_tensor(np.array([3, 9], dtype=np.int64)).to(db.device)
    regd = torch.full((B, 2, 2), 7.0, dtype=torch.float64, device=db.device)
    with pytest.raises(ValueError, match="unknown flags"):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_grid", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), thd.data_ptr(), 2, ckd.data_ptr(), 2, SQ2,
                      regd.data_ptr(), None, 64, None, db._sp)
    torch.cuda.synchronize()
    assert bool((regd == 7.0).all())


# ------------------------------------------------------------------ 8. capture
def test_device_call_is_capture_safe(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = C.family("gt_like", 64)
    s = torch.cuda.Stream()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=s).pack(f.z, f.y)
    assert (db.L.P, db.L.C) == (8, 8)
    tha = np.ascontiguousarray(np.broadcast_to(np.array(THG7), (B, M7)))
    flags = _lib.OCX_SMART_CLOSED_PREFIX | _lib.OCX_ALG_CLOSED_COMPARATOR
    with torch.cuda.stream(s):
        th = torch.as_tensor(tha).to(db.device)
        ck = torch.as_tensor(np.array(CK7, dtype=np.int64)).to(db.device)

    def buffers():
        with torch.cuda.stream(s):
            return (torch.zeros((B, M7, K7), dtype=torch.float64, device=db.device),
                    torch.full((B, M7, K7), -7, dtype=torch.int64, device=db.device))

    def run(o):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_grid", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), th.data_ptr(), M7, ck.data_ptr(), K7, SQ2,
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
    ref = pair_list(db, CK7, THG7, closed_prefix=True, closed_comparator=True)
    assert np.array_equal(cap[0].cpu().numpy(), ref["regret"])
    assert np.array_equal(cap[1].cpu().numpy(), ref["switch_step"])


# ------------------------------------------------------------------ 9. the wave form
@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("d", C.WAVE_DIMS)
def test_wave_form_equals_the_oracle_and_the_lane_group_grid(eng, d, name, monkeypatch):
    f = C.family(name, d)
    want_reg, want_sw = C.oracle_grid(name, d, tuple(HZ9), tuple(THG9))
    for P in (1, -1, -4):
        db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
        assert db.exact
        stl = new_stats(db)
        lanes = host(db.simulate_smart_grid(HZ9, THG9, SQ2, closed_prefix=False,
                                            closed_comparator=False, stats=stl, _group=1))
        assert_grid(lanes, want_reg, want_sw, (P, d, name, "lanes"))
        counts = {}
        for group in (1, 2, 4, 8):
            st = new_stats(db)
            got = host(db.simulate_smart_grid(HZ9, THG9, SQ2, stats=st, _wave=group))
            assert_grid(got, want_reg, want_sw, (P, d, name, group))
            counts[group] = int(st.cpu().numpy()[0])
            assert int(st.cpu().numpy()[1]) == 0
        # group 1: one column per launch, as the lane-group grid at group 1
        assert counts[1] == int(stl.cpu().numpy()[0]), (P, d, name, counts)
        assert counts[1] >= counts[2] >= counts[4] >= counts[8] > 0, counts
        # the unforced call: the same bits, whichever kernel the dispatch takes
        for env in (None, "wave", "lanes"):
            with monkeypatch.context() as mp:
                if env:
                    mp.setenv("OCX_SMART_KERNEL", env)   # read at every call
                pub = host(db.simulate_smart_grid(HZ9, THG9, SQ2))
            assert_grid(pub, want_reg, want_sw, (P, d, name, "public", env))


def test_wave_form_shares_the_lane_group_rescan_count(eng):
    d, P = 16, -4
    f = C.family("gt_like", d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    full_sw = C.oracle_full("gt_like", d, tuple(THG9))[1]
    ck = HZ9[:-2]   # the last checkpoint, 130, is before T: the count is capped at it
    pre = C.pre_switch_steps(full_sw, ck[-1])
    for group in (1, 2, 4):
        stl, stw = new_stats(db), new_stats(db)
        a = host(db.simulate_smart_grid(ck, THG9, SQ2, closed_prefix=False,
                                        closed_comparator=False, stats=stl, _group=group))
        b = host(db.simulate_smart_grid(ck, THG9, SQ2, stats=stw, _wave=group))
        assert all(np.array_equal(a[k], b[k]) for k in a)
        want = sum(int(pre[:, m0:m0 + group].max(axis=1).sum())
                   for m0 in range(0, len(THG9), group))
        assert int(stl.cpu().numpy()[0]) == int(stw.cpu().numpy()[0]) == want, (group, want)


# ------------------------------------------------------------------ 10. drivers and g(T)
def test_driver_grid_equals_the_per_horizon_driver(eng):
    from online_convex_optimization_amd import drivers
    ck = [20, 57, 100]
    ths = [2.0, math.inf, 0.5, 4.5, -1.0]
    reg, sw = drivers.case_threshold_regret_grid("Label flips", ck, ths, runs=2, replicates=3)
    assert reg.shape == sw.shape == (2, 3, len(ths), len(ck)) and sw.dtype == np.int64
    for k, t in enumerate(ck):
        r, s = drivers.case_threshold_regrets("Label flips", t, ths, runs=2, replicates=3)
        assert np.array_equal(reg[..., k], r) and np.array_equal(sw[..., k], s), t
    assert len({reg[..., m, -1].tobytes() for m in range(len(ths))}) >= 3


def test_gT_smart_grids_is_generate_and_simulate(eng):
    Tn, runs, d = 120, 70, 5
    ck = [0, 30, 64, 120]
    ths = [1.0, 2.5, math.inf]
    db = eng.DeviceBatch(runs, Tn, d, lanes_per_seq=1)
    db.generate_gT(11, 3)
    want = host(db.simulate_smart_grid(ck, ths, SQ2))
    reg, sw = eng.gT_smart_grids(Tn, runs, ck, ths, base_seed=11, d=d, run0=3, lanes_per_seq=1,
                                 return_switch=True)
    assert reg.shape == sw.shape == (runs, len(ths), len(ck))
    assert np.array_equal(reg, want["regret"][:runs])
    assert np.array_equal(sw, want["switch_step"][:runs])
    for batch in (16, 69, 1000):
        got = eng.gT_smart_grids(Tn, runs, ck, ths, base_seed=11, d=d, run0=3, lanes_per_seq=1,
                                 batch=batch)
        assert np.array_equal(got, reg), batch
    assert (sw[:, 0, -1] >= 0).any() and np.all(sw[:, 2] == -1)
