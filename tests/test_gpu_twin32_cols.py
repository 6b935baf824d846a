"""GPU: the float32 twin's column sweeps (csrc/ocx_twin32_cols.hip; engine.twin32_cols_batch,
DeviceBatch.simulate_twin32_cols / twin32_comparison_curves, drivers.driver_case_regret_curves).

Column k must carry the bits of the single call on the batch truncated at t_k: every comparison
is np.array_equal on all four outputs (result float32, cum_loss float64, comp_loss float32,
switch_step int64), against the golden values of the twin's own NumPy calls
(tests/golden/twin32.npz), against engine.twin32_batch on the truncated arrays and against the
explicit-order oracle (oracle.t32_*).  tests/test_twin32_cols_cpu.py shows that the inputs of
tests/_twin32_cols_cases.py can catch a kernel that ignores or misplaces a horizon."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import _twin32_cols_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SQ2 = math.sqrt(2)
F = np.float32


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    assert _lib.device_count() >= 1
    return engine


@pytest.fixture(scope="module")
def fx():
    with np.load(os.path.join(HERE, "golden", "twin32.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def _same(got, want, what):
    assert len(got) == len(want) == 4
    for i, name in enumerate(("result", "cum", "comp", "switch_step")):
        g, w = np.asarray(got[i]), np.asarray(want[i])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype)
        assert np.array_equal(g, w), (what, name)


def _fill(th):
    """NaN (no threshold: FTRL / FTL columns) -> 0.0, everything else as it is."""
    th = np.asarray(th, dtype=np.float64)
    return np.where(np.isnan(th), 0.0, th)


def _singles(eng, z, y, hz, algos, th, eta0=SQ2):
    """The columns one by one: twin32_batch on the truncated arrays ([B, K] each)."""
    B, K = z.shape[0], len(hz)
    th = np.broadcast_to(np.asarray(th, dtype=np.float64), (B, K))
    cols = []
    for k in range(K):
        t, a = int(hz[k]), int(algos[k])
        cols.append(eng.twin32_batch(np.ascontiguousarray(z[:, :t]), np.ascontiguousarray(y[:, :t]),
                                     a, eta0, thresh=th[:, k] if a == 2 else None,
                                     return_all=True))
    return tuple(np.stack([c[i] for c in cols], axis=1) for i in range(4))


def _oracle_rows(z, y, hz, algos, th, rows, eta0=SQ2):
    """The oracle on the sequences `rows`: ([len(rows), K] each)."""
    K = len(hz)
    th = np.broadcast_to(np.asarray(th, dtype=np.float64), (z.shape[0], K))
    res = np.zeros((len(rows), K), dtype=F)
    cum = np.zeros((len(rows), K))
    comp = np.zeros((len(rows), K), dtype=F)
    sw = np.full((len(rows), K), -1, dtype=np.int64)
    for i, b in enumerate(rows):
        for k in range(K):
            t, a = int(hz[k]), int(algos[k])
            if a == 2:
                res[i, k], cum[i, k], comp[i, k], sw[i, k] = O.t32_simulate_smart_full(
                    z[b, :t], y[b, :t], float(th[b, k]), eta0)
            else:
                res[i, k], cum[i, k], comp[i, k] = O.t32_simulate_alg_full(z[b, :t], y[b, :t], a,
                                                                          eta0)
    return res, cum, comp, sw


def test_golden_full_horizon(eng, fx):
    z, y = fx["smart_z"], fx["smart_y"]
    th = fx["smart_thresh"]
    got = eng.twin32_cols_batch(z, y, [z.shape[1]] * len(th), 2, th, return_all=True)
    _same(got, (fx["smart_res"].T, fx["smart_cum"].T, fx["smart_comp"].T, fx["smart_sw"].T),
          "smart fixtures")
    for key in ("alg_T100", "alg_T7", "alg_T1"):
        z, y = fx[key + "_z"], fx[key + "_y"]
        runs = fx[key + "_runs"]
        for e in sorted({float(e) for _, e in runs}):
            idx = [i for i, (_, ee) in enumerate(runs) if float(ee) == e]
            algos = [int(runs[i][0]) for i in idx]
            got = eng.twin32_cols_batch(z, y, [z.shape[1]] * len(idx), algos, None, e,
                                        return_all=True)
            want = (fx[key + "_res"][idx].T, fx[key + "_cum"][idx].T, fx[key + "_comp"][idx].T,
                    np.full((z.shape[0], len(idx)), -1, dtype=np.int64))
            _same(got, want, (key, e))


def test_golden_cut(eng, fx):
    z, y = fx["smart_z"], fx["smart_y"]
    hz, th = [30, 75, 300, 300], [2.0, 5.0, 2.0, 5.0]
    got = eng.twin32_cols_batch(z, y, hz, 2, th, return_all=True)
    _same(got, _singles(eng, z, y, hz, [2] * 4, th), "cut vs twin32_batch")
    _same(got, _oracle_rows(z, y, hz, [2] * 4, th, range(z.shape[0])), "cut vs oracle")
    # the cut columns differ from the full ones where a sequence switches after the cut
    assert (got[3][:, 0] != got[3][:, 2]).sum() == 3 and (got[3][:, 1] != got[3][:, 3]).sum() == 2


@pytest.mark.parametrize("d", C.DIMS)
def test_cases_smart_pairs_and_mixed_list(eng, d):
    z, y = C.case(d)
    rows = list(range(6)) + list(range(C.B - 6, C.B))
    # the seven SMART pairs
    got = eng.twin32_cols_batch(z, y, C.CK7, "SMART", C.TH7, return_all=True)
    _same(got, _singles(eng, z, y, C.CK7, [2] * 7, C.TH7), ("pairs", d))
    _same(tuple(g[rows] for g in got), _oracle_rows(z, y, C.CK7, [2] * 7, C.TH7, rows),
          ("pairs vs oracle", d))
    assert np.all(got[3][:, C.INF_COL] == -1)
    # FTRL, FTL and SMART at repeated horizons, K = 9: more than one launch at every group
    algos = [C.ALGO_CODE[a] for a in C.MIX_ALGO]
    got = eng.twin32_cols_batch(z, y, C.MIX_HZ, C.MIX_ALGO, C.MIX_TH, return_all=True)
    _same(got, _singles(eng, z, y, C.MIX_HZ, algos, _fill(C.MIX_TH)), ("mixed", d))
    _same(tuple(g[rows] for g in got),
          _oracle_rows(z, y, C.MIX_HZ, algos, _fill(C.MIX_TH), rows),
          ("mixed vs oracle", d))
    # the +inf SMART column is the FTL column at the same horizon (columns 5 and 6, t = 102)
    assert C.MIX_TH[5] == np.inf and C.MIX_ALGO[6] == "FTL" and C.MIX_HZ[5] == C.MIX_HZ[6]
    for i in range(4):
        assert np.array_equal(got[i][:, 5], got[i][:, 6]), i
    # horizon 0: 0.0f, 0.0, 0.0f, -1
    assert not got[0][:, 0].any() and not got[1][:, 0].any() and not got[2][:, 0].any()
    assert np.all(got[3][:, 0] == -1)
    if d == 5:  # eta0 = 0.3 once: FTRL's rescale branch (||x|| > 1) is rarely taken at sqrt 2
        got = eng.twin32_cols_batch(z, y, C.MIX_HZ, C.MIX_ALGO, C.MIX_TH, 0.3, return_all=True)
        _same(got, _singles(eng, z, y, C.MIX_HZ, algos, _fill(C.MIX_TH), 0.3),
              ("mixed eta0 = 0.3", d))


def _resident(eng, z, y):
    import torch
    B, T, d = z.shape
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=-1)
    db.pack(torch.as_tensor(z.astype(np.float64)).cuda(), torch.as_tensor(y.astype(np.float64)).cuda())
    return db


def _dev(out):
    return tuple(out[k].cpu().numpy() for k in ("result", "cum", "comp", "switch_step"))


def test_groups_give_identical_arrays(eng):
    from online_convex_optimization_amd import _lib
    z, y = C.case(5)
    db = _resident(eng, z, y)
    algos = [C.ALGO_CODE[a] for a in C.MIX_ALGO]
    assert _lib.load().ocx_twin32_cols_group(ctypes.byref(db.L), 9) == 8
    assert _lib.load().ocx_twin32_cols_group(ctypes.byref(db.L), 3) == 4
    assert _lib.load().ocx_twin32_cols_group(ctypes.byref(db.L), 1) == 1
    want = _dev(db.simulate_twin32_cols(C.MIX_HZ, algos, C.MIX_TH))
    _same(want, eng.twin32_cols_batch(z, y, C.MIX_HZ, algos, C.MIX_TH, return_all=True),
          "resident vs host")
    want7 = _dev(db.simulate_twin32_cols(C.CK7, 2, C.TH7))
    for g in (1, 2, 4, 8):
        _same(_dev(db.simulate_twin32_cols(C.MIX_HZ, algos, C.MIX_TH, _group=g)), want, ("mixed", g))
        _same(_dev(db.simulate_twin32_cols(C.CK7, 2, C.TH7, _group=g)), want7, ("pairs", g))
    with pytest.raises(ValueError):
        db.simulate_twin32_cols(C.CK7, 2, C.TH7, _group=3)
    # d = 31 (32 coordinates: two columns per launch) and d = 2, at their default group
    for d, B, T in ((31, 3, 41), (2, 5, 77)):
        rng = np.random.default_rng(900 + d)
        z = (rng.standard_normal((B, T, d)) * 0.5).astype(F)
        y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0).astype(F)
        hz = [1, 9, 9, T - 3, T, T]
        al = [2, 0, 2, 1, 2, 0]
        th = [0.2, np.nan, 1.0, np.nan, 2.5, np.nan]
        got = eng.twin32_cols_batch(z, y, hz, al, th, return_all=True)
        _same(got, _singles(eng, z, y, hz, al, _fill(th)), ("d", d))
        _same(got, _oracle_rows(z, y, hz, al, _fill(th), range(B)), ("oracle", d))
    db31 = eng.DeviceBatch(3, 41, 31, lanes_per_seq=-1)
    assert _lib.load().ocx_twin32_cols_group(ctypes.byref(db31.L), 6) == 2
    with pytest.raises(NotImplementedError):  # no 4-column form at 32 coordinates
        db31.simulate_twin32_cols([1, 2], 1, None, _group=4)


def test_per_sequence_thresholds(eng):
    z, y = C.case(8)
    rng = np.random.default_rng(8)
    th = rng.choice([0.3, 1.5, 1e9], size=(C.B, len(C.CK7)))
    got = eng.twin32_cols_batch(z, y, C.CK7, 2, th, return_all=True)
    _same(got, _singles(eng, z, y, C.CK7, [2] * 7, th), "per-sequence thresholds")
    sw = got[3]
    assert (sw[th == 1e9] == -1).all() and (sw[th == 0.3] >= 0).sum() > 50


def test_edges(eng):
    import torch
    from online_convex_optimization_amd import _lib
    z, y = C.case(5)
    z, y = z[:3, :20], y[:3, :20]
    # K = 0, B = 0, T = 0, horizons all 0
    r = eng.twin32_cols_batch(z, y, [], 2, None, return_all=True)
    assert [a.shape for a in r] == [(3, 0)] * 4
    r = eng.twin32_cols_batch(z[:0], y[:0], [3, 5], [0, 2], None, return_all=True)
    assert [a.shape for a in r] == [(0, 2)] * 4
    r = eng.twin32_cols_batch(z[:, :0], y[:, :0], [0, 0, 0], [0, 1, 2], None, return_all=True)
    zero = (np.zeros((3, 3), dtype=F), np.zeros((3, 3)), np.zeros((3, 3), dtype=F),
            np.full((3, 3), -1, dtype=np.int64))
    _same(r, zero, "T = 0")
    _same(eng.twin32_cols_batch(z, y, [0, 0, 0], [0, 1, 2], [np.nan, np.nan, -1.0],
                                return_all=True), zero, "horizons all 0")
    assert eng.twin32_cols_batch(z, y, [4, 20], [1, 2]).dtype == np.float32
    # null optional outputs through the C ABI, and a bad list that leaves the outputs untouched
    db = _resident(eng, np.ascontiguousarray(z), np.ascontiguousarray(y))
    want = _dev(db.simulate_twin32_cols([4, 20, 20], [1, 2, 0], [np.nan, 1.0, np.nan]))
    hz = np.array([4, 20, 20], dtype=np.int64)
    al = np.array([1, 2, 0], dtype=np.int32)
    th = torch.tensor([[0.0, 1.0, 0.0]] * 3, dtype=torch.float64, device="cuda")
    res = torch.full((3, 3), 7.0, dtype=torch.float32, device="cuda")
    lib = _lib.load()

    def call(hz, al, thp, resp):
        return lib.ocx_dev_twin32_cols(ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), 3,
                                       hz.ctypes.data_as(_lib.c_i64p),
                                       al.ctypes.data_as(_lib.c_i32p), SQ2, thp, resp, None, None,
                                       None, None)
    assert call(hz, al, th.data_ptr(), res.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(res.cpu().numpy(), want[0])
    res.fill_(7.0)
    torch.cuda.synchronize()
    for bhz, bal, bth in (([20, 4, 20], [1, 2, 0], th.data_ptr()), ([4, 20, 21], [1, 2, 0], th.data_ptr()),
                          ([-1, 20, 20], [1, 2, 0], th.data_ptr()), ([4, 20, 20], [1, 3, 0], th.data_ptr()),
                          ([4, 20, 20], [1, -1, 0], th.data_ptr()), ([4, 20, 20], [1, 2, 0], None)):
        rc = call(np.array(bhz, dtype=np.int64), np.array(bal, dtype=np.int32), bth, res.data_ptr())
        assert rc == -1, (bhz, bal, bth)  # OCX_E_INVALID
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == 7.0).all()
    # a layout that is not one lane per sequence
    db4 = eng.DeviceBatch(3, 20, 64, lanes_per_seq=1)
    with pytest.raises((ValueError, _lib.OCXError)):
        db4.simulate_twin32_cols([4], 1)


def test_lds_limit(eng):
    rng = np.random.default_rng(23)
    B, T, d = 3, 2300, 5
    z = (rng.standard_normal((B, T, d)) * 0.5).astype(F)
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0).astype(F)
    db = _resident(eng, z, y)
    hz, al, th = [50, 50, 100, 100], [2, 0, 2, 1], [1.5, np.nan, 4.0, np.nan]
    got = _dev(db.simulate_twin32_cols(hz, al, th))
    _same(got, _singles(eng, z, y, hz, al, _fill(th)), "resident 2300, cut")
    with pytest.raises(NotImplementedError, match="2194"):
        db.simulate_twin32_cols([50, 2300], 2)
    with pytest.raises(NotImplementedError, match="2194"):
        eng.twin32_cols_batch(z, y, [2195], 0)
    # nothing was launched or written by the refused calls: the batch still answers
    _same(_dev(db.simulate_twin32_cols(hz, al, th)), got, "after the refusal")


def test_comparison_curves_match_the_per_T_driver(eng):
    from online_convex_optimization_amd import drivers
    grid, runs, reps = [30, 64, 100], 2, 3
    g_emp = {30: 2.5, 64: 4.0, 100: 5.5}
    for title in ("Label flips", "Switching leaders"):
        family, stream0 = drivers.CASE_FAMILIES[title]
        B = runs * reps
        db = eng.DeviceBatch(B, grid[-1], 5, lanes_per_seq=-1)
        run_idx = np.repeat(np.arange(runs), reps)
        rep_idx = np.tile(np.arange(reps), runs)
        db.generate_family(family, 2025 * (run_idx + 1), stream0 + rep_idx)
        out = db.twin32_comparison_curves(grid, [g_emp[t] for t in grid])
        assert sorted(out) == ["EMP", "FTL", "FTRL", "SMART"]
        curves = drivers.driver_case_regret_curves(title, grid, g_emp, runs=runs, replicates=reps)
        for ti, T in enumerate(grid):
            want = drivers.case_regrets_twin32(title, T, g_emp[T], runs=runs, replicates=reps)
            # and the four single launches on the family generated at T itself
            dbT = eng.DeviceBatch(B, T, 5, lanes_per_seq=-1)
            dbT.generate_family(family, 2025 * (run_idx + 1), stream0 + rep_idx)
            single = {"FTRL": dbT.simulate_twin32(0, SQ2), "FTL": dbT.simulate_twin32(1, SQ2),
                      "SMART": dbT.simulate_twin32(2, SQ2, math.sqrt(2 * T)),
                      "EMP": dbT.simulate_twin32(2, SQ2, g_emp[T])}
            for k in drivers.ALGO_KEYS:
                assert np.array_equal(single[k][:B].cpu().numpy().reshape(runs, reps), want[k])
                got = out[k][:B, ti].cpu().numpy()
                assert got.dtype == np.float32
                assert np.array_equal(got.reshape(runs, reps), want[k]), (title, T, k)
                assert np.array_equal(curves[k][:, ti], got), (title, T, k)
        assert sorted(db.twin32_comparison_curves(grid)) == ["FTL", "FTRL", "SMART"]


def test_driver_beyond_the_lds_limit_keeps_the_single_calls(eng):
    """case_regrets_twin32 at a T whose rows do not fit the LDS takes the four single calls,
    as it did before the column call existed."""
    from online_convex_optimization_amd import drivers
    T, runs, reps, g = 2300, 1, 2, 3.0
    got = drivers.case_regrets_twin32("Label flips", T, g, runs=runs, replicates=reps)
    db = eng.DeviceBatch(runs * reps, T, 5, lanes_per_seq=-1)
    db.generate_family("flip", 2025 * np.ones(2, dtype=np.int64), np.arange(2))
    with pytest.raises(NotImplementedError):
        db.simulate_twin32_cols([T], 1)
    want = {"FTRL": db.simulate_twin32(0, SQ2), "FTL": db.simulate_twin32(1, SQ2),
            "SMART": db.simulate_twin32(2, SQ2, math.sqrt(2 * T)),
            "EMP": db.simulate_twin32(2, SQ2, g)}
    for k in drivers.ALGO_KEYS:
        assert got[k].dtype == np.float32 and got[k].shape == (runs, reps)
        assert np.array_equal(got[k], want[k][:2].cpu().numpy().reshape(runs, reps)), k
