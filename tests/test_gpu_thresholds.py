"""Threshold sweeps (ocx_dev_simulate_smart_thresholds and the layers above it): SMART for M
switch thresholds in passes over z that each serve a group of them.

Bit for bit against the C oracle in the exact modes, and bit for bit per column against
DeviceBatch.simulate_smart on the same packed batch for every forced group size and every
flag pair.  That single-threshold call is the sweep kernel's own one-column instance (one
launch, [B] read as [B][1]), so against group 1 the comparison checks the wrapper's strides
and against groups 2 and 4 that a column's bits do not depend on its neighbours; what pins the
one-column bits themselves is the oracle in the exact modes, the plain re-scan kernel in
lane-group form (flags 0, every layout) and the record of tests/test_gpu_smart.py.  TH7 on
the `beam` and `gt_like` rows (tests/_thresholds_cases.py, conditions
asserted in tests/test_thresholds_cpu.py) gives every column of every sequence its own switch
step and FTRL trajectory."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F
from tests import _thresholds_cases as C

pytestmark = pytest.mark.gpu

B, T = C.B, C.T
SQ2 = C.SQ2
TH7 = C.TH7
M7 = len(TH7)


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


def single(db, th, pf, cc, stats=True):
    """(regret [B], switch_step [B], stats [2]) of the single-threshold call on the packed
    batch; th scalar or [B].  With a stats tensor the call runs the lane-group kernel in the
    batch's own layout for every flag pair: one launch of the sweep kernel's one-column
    instance, thresholds and outputs [B] read as [B][1].  Without one, flags (False, False)
    go to ocx_dev_simulate_smart's dispatch, other kernels: the plain re-scan kernel in
    lane-group form (ocx_smart_kernel; always, under OCX_SMART_KERNEL=lanes), or at d <= 64
    the one-wave-per-sequence kernel, which sums in the reference's order whatever the
    layout, so it carries a butterfly layout's bits only in the exact modes."""
    import torch
    Bn = int(db.L.B)
    sw = torch.full((Bn,), -7, dtype=torch.int64, device=db.device)
    st = new_stats(db) if stats else None
    reg = db.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=pf, closed_comparator=cc,
                            stats=st)
    torch.cuda.synchronize()
    return (reg[:Bn].cpu().numpy().copy(), sw.cpu().numpy(),
            st.cpu().numpy() if stats else None)


def existing(db, ths, pf, cc, stats=True):
    """[B, M] regret and switch_step of M single-threshold calls, and their summed stats."""
    cols = [single(db, th, pf, cc, stats) for th in ths]
    return (np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1),
            sum(c[2] for c in cols) if stats else None)


def has_instance(C_lane, group):
    return group == 1 or C_lane <= 8 or (group == 2 and C_lane <= 16)


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100)]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle(eng, P, d, name):
    f = C.family(name, d)
    want_reg, want_sw = C.oracle_columns(name, d)
    reg, sw = eng.simulate_smart_thresholds_batch(f.z, f.y, TH7, lanes_per_seq=P,
                                                  return_switch=True)
    assert reg.shape == sw.shape == (B, M7) and sw.dtype == np.int64
    for m in range(M7):
        assert np.array_equal(sw[:, m], want_sw[:, m]), (P, d, name, m, "switch_step")
        assert np.array_equal(reg[:, m], want_reg[:, m]), (P, d, name, m, "regret")
    ftl = O.simulate_alg_batch(f.z, f.y, 1, SQ2, nthreads=4)[0]
    assert np.array_equal(reg[:, C.INF_COL], ftl) and np.all(sw[:, C.INF_COL] == -1)
    # the plain call returns the same regrets
    assert np.array_equal(eng.simulate_smart_thresholds_batch(f.z, f.y, TH7, lanes_per_seq=P),
                          reg)


# ------------------------------------------------------------------ 2. every layout, every group
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 5), (-4, 16), (1, 64)]
FLAG_PAIRS = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_columns_equal_the_existing_kernel_for_every_group(eng, monkeypatch, P, d, name):
    from online_convex_optimization_amd import _lib
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    Cl = int(db.L.C)
    for pf, cc in FLAG_PAIRS:
        ref_reg, ref_sw, _ = existing(db, TH7, pf, cc)
        if pf or cc or d > 64 or db.L.chain or db.L.P == 1:
            # the call without a stats tensor carries the same bits, except where it is the
            # one-wave kernel in a butterfly layout (see `single`; measured there on these
            # inputs: the same switch steps, regrets up to 1.2e-13 apart)
            plain_reg, plain_sw, _ = existing(db, TH7, pf, cc, stats=False)
            assert np.array_equal(plain_sw, ref_sw), (P, d, name, pf, cc)
            assert np.array_equal(plain_reg, ref_reg), (P, d, name, pf, cc)
        if not (pf or cc):
            # an independent witness in every layout: the plain re-scan kernel in lane-group
            # form (ocx_smart_kernel, ocx_sim.hip) shares no kernel code with the sweep
            with monkeypatch.context() as mp:
                mp.setenv("OCX_SMART_KERNEL", "lanes")   # read at every call
                wit_reg, wit_sw, _ = existing(db, TH7, False, False, stats=False)
            assert np.array_equal(wit_sw, ref_sw), (P, d, name, "lane-group witness")
            assert np.array_equal(wit_reg, ref_reg), (P, d, name, "lane-group witness")
        ok = []
        # group 1 against ref compares the one-column instance with itself: it still checks
        # the wrapper's strides; groups 2 and 4, the oracle tests and the record of
        # tests/test_gpu_smart.py carry the weight
        for group in (1, 2, 4):
            try:
                got = host(db.simulate_smart_thresholds(TH7, SQ2, closed_prefix=pf,
                                                        closed_comparator=cc, _group=group))
            except _lib.OCXError as e:
                assert not has_instance(Cl, group) and "unsupported" in str(e), \
                    (P, d, group, str(e))
                continue
            assert has_instance(Cl, group), (P, d, group)
            ok.append(group)
            for m in range(M7):
                assert np.array_equal(got["switch_step"][:, m], ref_sw[:, m]), \
                    (P, d, name, pf, cc, group, m, "switch_step")
                assert np.array_equal(got["regret"][:, m], ref_reg[:, m]), \
                    (P, d, name, pf, cc, group, m, "regret")
        pub = host(db.simulate_smart_thresholds(TH7, SQ2, closed_prefix=pf, closed_comparator=cc))
        for k, ref in (("regret", ref_reg), ("switch_step", ref_sw)):
            for m in range(M7):
                assert np.array_equal(pub[k][:, m], ref[:, m]), (P, d, name, pf, cc, "public", m, k)
            assert np.array_equal(pub[k][:, C.DUP_COLS[0]], pub[k][:, C.DUP_COLS[1]]), \
                (P, d, name, pf, cc, "duplicate", k)
        assert _lib.load().ocx_smart_thresholds_group(ctypes.byref(db.L), M7) in ok
    # the columns are different runs
    assert len({pub["switch_step"][:, m].tobytes() for m in range(M7)}) == 6
    assert len({pub["regret"][:, m].tobytes() for m in range(M7)}) == 6


# ------------------------------------------------------------------ 3. the re-scan is shared
# columns of TH7 per forced group; (4, three columns): the spare column of a tail launch
SHARED = [(1, [0]), (2, [0, 1]), (4, [0, 1, 2, 6]), (4, [0, 1, 6])]


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("P,d", [(1, 5), (-4, 16), (-1, 16)])
def test_one_rescan_per_step_serves_every_column(eng, P, d, name):
    f = C.family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    assert db.exact   # the oracle's switch steps are the layout's
    ran = 0
    for group, idx in SHARED:
        if not has_instance(int(db.L.C), group):
            continue
        ran += 1
        ths = [TH7[i] for i in idx]
        assert len(ths) <= group
        sw = C.oracle_columns(name, d)[1][:, idx]
        st = new_stats(db)
        got = host(db.simulate_smart_thresholds(ths, SQ2, closed_prefix=False,
                                                closed_comparator=False, stats=st, _group=group))
        assert np.array_equal(got["switch_step"], sw), (P, d, name, group)
        want = int(C.pre_switch_steps(sw, T).max(axis=1).sum())
        stv = st.cpu().numpy()
        print("rescans", P, d, name, group, idx, int(stv[0]), want)
        assert stv[0] == want and stv[1] == 0, (P, d, name, group, stv, want)
    assert ran >= 2


@pytest.mark.parametrize("P,d", [(1, 5), (8, 64), (0, 5)])
def test_closed_forms_count_once_per_launch(eng, P, d):
    f = C.family("gt_like", d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    groups = [g for g in (1, 2, 4) if has_instance(int(db.L.C), g)]
    singles_pf = existing(db, TH7, True, False)[2]
    for group in groups:
        st = new_stats(db)
        host(db.simulate_smart_thresholds(TH7, SQ2, closed_prefix=True, closed_comparator=False,
                                          stats=st, _group=group))
        stv = st.cpu().numpy()
        print("closed prefix rescans", P, d, group, int(stv[0]), int(singles_pf[0]))
        assert stv[0] <= singles_pf[0] and stv[1] == 0, (P, d, group, stv, singles_pf)
        st = new_stats(db)
        host(db.simulate_smart_thresholds(TH7, SQ2, closed_prefix=True, closed_comparator=True,
                                          stats=st, _group=group))
        launches = -(-M7 // group)
        assert st.cpu().numpy()[1] == B * launches, (P, d, group, st.cpu().numpy())


# ------------------------------------------------------------------ 4. guard-band ties
def test_guard_band_ties_rescan_and_keep_the_reference_steps(eng):
    z, y, _ = O.flip_sequence(C.FLIP_T)
    th = C.FLIP_TH
    Bn = 3
    Z = np.repeat(z[None].astype(np.float64), Bn, axis=0)
    Y = np.repeat(y[None].astype(np.float64), Bn, axis=0)
    Zc = np.repeat(z[None].astype(np.float64), len(th), axis=0)
    Yc = np.repeat(y[None].astype(np.float64), len(th), axis=0)
    ref, rsw = O.simulate_smart_batch(Zc, Yc, th, SQ2, nthreads=4)   # one sequence per column
    for lanes in (1, eng.LANES_BEST):
        db = eng.DeviceBatch(Bn, C.FLIP_T, z.shape[1], lanes_per_seq=lanes).pack(Z, Y)
        st = new_stats(db)
        got = host(db.simulate_smart_thresholds(th, SQ2, closed_prefix=True,
                                                closed_comparator=lanes != 1, stats=st))
        for b in range(Bn):
            assert np.array_equal(got["switch_step"][b], rsw), (lanes, b)
            assert np.array_equal(got["regret"][b], ref), (lanes, b)
        assert st.cpu().numpy()[0] > 0   # some exact ties were caught by the band


# ------------------------------------------------------------------ 5. non-finite thresholds
def test_non_finite_thresholds_decide_without_rescan(eng):
    Bn, Tn, d = 4, 300, 8
    th = [np.inf, -np.inf, np.nan, 1e300]
    db = eng.DeviceBatch(Bn, Tn, d, lanes_per_seq=1).generate_gT(base_seed=5)
    st = new_stats(db)
    got = host(db.simulate_smart_thresholds(th, SQ2, closed_prefix=True, closed_comparator=False,
                                            stats=st))
    assert st.cpu().numpy()[0] == 0, st
    for b in range(Bn):
        assert list(got["switch_step"][b]) == [-1, 0, -1, -1], b
        z, y = O.gT_sample(5, Tn, b, d)
        for m, t in enumerate(th):
            ref, rsw = O.simulate_SMART_like(z, y, float(t), SQ2, return_switch=True)
            assert got["regret"][b, m] == ref and got["switch_step"][b, m] == rsw, (b, m)


# ------------------------------------------------------------------ 6. per-sequence thresholds
def test_per_sequence_thresholds(eng):
    Bn, Tn, d, M = 64, 600, 8, 5
    th = np.random.default_rng(12).uniform(-1.0, 30.0, size=(Bn, M))
    db = eng.DeviceBatch(Bn, Tn, d, lanes_per_seq=1).generate_gT(base_seed=11)
    got = host(db.simulate_smart_thresholds(th, SQ2))
    assert got["regret"].shape == got["switch_step"].shape == (Bn, M)
    for m in range(M):
        reg, sw, _ = single(db, th[:, m].copy(), None, None, stats=False)
        assert np.array_equal(got["switch_step"][:, m], sw), m
        assert np.array_equal(got["regret"][:, m], reg), m
    assert len({got["switch_step"][:, m].tobytes() for m in range(M)}) == M


# ------------------------------------------------------------------ 7. degenerate cases
def test_degenerate_cases(eng):
    from online_convex_optimization_amd import drivers
    f = C.family("beam", 5)
    # M = 0, host and device
    reg, sw = eng.simulate_smart_thresholds_batch(f.z, f.y, [], lanes_per_seq=1, return_switch=True)
    assert reg.shape == sw.shape == (B, 0)
    assert eng.simulate_smart_thresholds_batch(f.z, f.y, []).shape == (B, 0)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    assert all(v.shape == (B, 0) for v in host(db.simulate_smart_thresholds([])).values())
    # M = 1: the single-threshold call
    reg, sw = eng.simulate_smart_thresholds_batch(f.z, f.y, [1.5], lanes_per_seq=1,
                                                  return_switch=True)
    ref, rsw = eng.simulate_smart_batch(f.z, f.y, 1.5, SQ2, lanes_per_seq=1, return_switch=True)
    assert reg.shape == (B, 1) and np.array_equal(reg[:, 0], ref) and np.array_equal(sw[:, 0], rsw)
    # T = 0: zeros and -1
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    for lanes in (1, 0):
        reg, sw = eng.simulate_smart_thresholds_batch(z0, y0, TH7, lanes_per_seq=lanes,
                                                      return_switch=True)
        assert reg.shape == sw.shape == (B, M7) and np.all(reg == 0.0) and np.all(sw == -1)
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_smart_thresholds(TH7))
    assert np.all(out["regret"] == 0.0) and np.all(out["switch_step"] == -1)
    # B = 1
    reg, sw = eng.simulate_smart_thresholds_batch(f.z[:1], f.y[:1], TH7, lanes_per_seq=1,
                                                  return_switch=True)
    for m, th in enumerate(TH7):
        ref, rsw = O.simulate_SMART_like(f.z[0], f.y[0], th, SQ2, return_switch=True)
        assert (reg[0, m], sw[0, m]) == (ref, rsw), th
    # thresholds that are not [M] or [B, M] real numbers
    for bad in (np.zeros((B, 2, 1)), ["a", "b"], None, [1.0 + 2.0j], np.zeros((B + 1, 2))):
        with pytest.raises(ValueError):
            eng.simulate_smart_thresholds_batch(f.z, f.y, bad)
        with pytest.raises(ValueError):
            db.simulate_smart_thresholds(bad)
        with pytest.raises(ValueError):
            drivers.case_threshold_regrets("Massart noise 10%", 20, bad, runs=4, replicates=6)


# ------------------------------------------------------------------ 8. capture
def test_device_call_is_capture_safe(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = C.family("gt_like", 64)
    s = torch.cuda.Stream()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=s).pack(f.z, f.y)
    assert (db.L.P, db.L.C) == (8, 8)
    tha = np.ascontiguousarray(np.broadcast_to(np.array(TH7), (B, M7)))
    flags = _lib.OCX_SMART_CLOSED_PREFIX | _lib.OCX_ALG_CLOSED_COMPARATOR
    with torch.cuda.stream(s):
        th = torch.as_tensor(tha).to(db.device)

    def buffers():
        with torch.cuda.stream(s):
            return (torch.zeros((B, M7), dtype=torch.float64, device=db.device),
                    torch.full((B, M7), -7, dtype=torch.int64, device=db.device))

    def run(o):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_smart_thresholds", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), th.data_ptr(), M7, SQ2, o[0].data_ptr(), o[1].data_ptr(),
                      flags, None, ctypes.c_void_p(s.cuda_stream))

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
    for m, t in enumerate(TH7):                               # and it is the existing kernel's
        reg, sw, _ = single(db, t, True, True)
        assert np.array_equal(cap[0][:, m].cpu().numpy(), reg), m
        assert np.array_equal(cap[1][:, m].cpu().numpy(), sw), m


# ------------------------------------------------------------------ 9. driver layer
def test_driver_columns_are_case_regrets(eng):
    from online_convex_optimization_amd import drivers
    title, Tn = "Massart noise 10%", 300
    reg, sw = drivers.case_threshold_regrets(title, Tn, [math.sqrt(600), 4.2, math.inf],
                                             runs=2, replicates=3)
    assert reg.shape == sw.shape == (2, 3, 3)
    want = drivers.case_regrets(title, Tn, g_emp_T=4.2, runs=2, replicates=3)
    for m, key in enumerate(("SMART", "EMP", "FTL")):
        assert np.array_equal(reg[:, :, m], want[key]), key
    assert np.all(sw[:, :, 2] == -1)
