"""CPU checks of the SMART regret grids (NumPy, the C oracle and the ABI; no GPU).

Input conditions, asserted from the oracle and never from the kernel: the inputs of
tests/test_gpu_smart_grid.py do what it needs.  At every dimension the GPU tests use, each of
the columns 3.0, 4.0, 6.0 and 7.0 of THG7 has an interior checkpoint of CK7 that splits it —
at least two sequences switched before it and at least two not yet — so a kernel that emits the
final switch step early, or a column's own total before its switch, cannot pass; HZ9 x THG9
split a column at every checkpoint >= 63 on `gt_like` rows and at checkpoints 2 and 3 on `beam`
rows.  A truncated run is the first t_k steps of the full run; the +inf column is FTL on every
prefix.

Entry points: the group rule, argument checking and the nothing-to-do shapes are host logic and
report through the error channel before a device or a data pointer is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from online_convex_optimization_amd import _lib, drivers, engine
from tests import _smart_grid_cases as C
from tests.test_curve_cpu import BAD_CHECKPOINTS, BUF, i64, last_error

DP = ctypes.cast(BUF, _lib.c_dp)     # never dereferenced: the checks come first
IP = ctypes.cast(BUF, _lib.c_i64p)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ input conditions
def split_counts(full_sw, ck):
    """before[m][k], later[m][k]: sequences of column m switched before checkpoint k, and not
    yet (they switch later or never)."""
    full_sw = np.asarray(full_sw)
    t = np.asarray(ck)[None, None, :]
    s = full_sw[:, :, None]
    before = ((s >= 0) & (s < t)).sum(axis=0)
    return before, full_sw.shape[0] - before


@pytest.mark.parametrize("name", C.FAMILIES)
@pytest.mark.parametrize("d", C.DIMS)
def test_ck7_splits_every_mid_column(name, d):
    full = C.oracle_full(name, d, tuple(C.THG7))[1]
    before, later = split_counts(full, C.CK7)
    interior = slice(1, len(C.CK7) - 1)
    for th in C.SPLIT_TH:
        m = C.THG7.index(th)
        ok = (before[m, interior] >= 2) & (later[m, interior] >= 2)
        print("split", name, d, th, before[m].tolist())
        assert ok.any(), (name, d, th, before[m], later[m])
    assert np.all(full[:, C.THG7.index(-1.0)] == 0) and np.all(full[:, C.INF_COL] == -1)
    assert np.array_equal(full[:, C.DUP_COLS[0]], full[:, C.DUP_COLS[1]])


@pytest.mark.parametrize("d", C.WAVE_DIMS)
def test_hz9_splits_a_column_at_every_late_checkpoint(d):
    full = C.oracle_full("gt_like", d, tuple(C.THG9))[1]
    before, later = split_counts(full, C.HZ9)
    for k, t in enumerate(C.HZ9):
        if t >= 63:
            ok = (before[:, k] >= 2) & (later[:, k] >= 2)
            assert ok.any(), (d, t, before[:, k], later[:, k])
    full = C.oracle_full("beam", d, tuple(C.THG9))[1]
    before, later = split_counts(full, C.HZ9)
    for k in (1, 2):   # checkpoints 2 and 3: inside the first group of speculated steps
        ok = (before[:, k] >= 1) & (later[:, k] >= 1)
        assert C.HZ9[k] in (2, 3) and ok.any(), (d, k, before[:, k], later[:, k])


@pytest.mark.parametrize("name,d", [("gt_like", 5), ("beam", 5), ("gt_like", 64), ("beam", 16)])
def test_truncated_runs_are_prefixes_of_the_full_run(name, d):
    f = C.family(name, d)
    for ck, ths in ((C.CK7, C.THG7), (C.HZ9, C.THG9)):
        reg, sw = C.oracle_grid(name, d, tuple(ck), tuple(ths))
        full_reg, full_sw = C.oracle_full(name, d, tuple(ths))
        assert np.array_equal(sw, C.truncate_switch(full_sw, ck)), (name, d)
        assert np.array_equal(reg[:, :, -1], full_reg)
        inf = ths.index(np.inf)
        for k, t in enumerate(ck):
            ftl = O.simulate_alg_batch(np.ascontiguousarray(f.z[:, :t]),
                                       np.ascontiguousarray(f.y[:, :t]), 1, C.SQ2, nthreads=4)[0]
            assert np.array_equal(reg[:, inf, k], ftl), (name, d, t)
        if ck[0] == 0:
            assert np.all(reg[:, :, 0] == 0.0) and np.all(sw[:, :, 0] == -1)


# ------------------------------------------------------------------ entry points
@pytest.mark.parametrize("B,T,d,lanes", [(24, 257, 5, 1), (24, 257, 64, -4), (37, 130, 64, 8),
                                         (24, 257, 1024, 64), (100, 10, 64, engine.LANES_BEST),
                                         (24, 257, 16, 0), (24, 257, 256, -32), (24, 257, 32, 8),
                                         (24, 257, 64, 16)])
def test_group_range_and_monotonicity(B, T, d, lanes):
    lib = _lib.load()
    L = _lib.layout(B, T, d, lanes)
    Lp = ctypes.byref(L)
    Cl = int(L.C)
    widest = 4 if Cl <= 8 else (2 if Cl <= 16 else 1)   # the instances that exist
    if int(L.chain) and Cl == 8 and int(L.P) == 32:
        widest = 2   # the four-column long chain on 32 lanes is not compiled
        assert lib.ocx_test_simulate_smart_grid(Lp, BUF, BUF, BUF, 5, BUF, 3, 1.0, BUF, None, 0,
                                                None, 4, None) == -3 and last_error(lib)
    assert lib.ocx_smart_grid_group(Lp, 0) == lib.ocx_smart_grid_group(Lp, 1) == 1
    prev = 1
    for M in range(1, 12):
        g = lib.ocx_smart_grid_group(Lp, M)
        assert g in (1, 2, 4) and g <= widest and (g == 1 or g // 2 < M), (M, g)
        assert g >= prev, (M, g, prev)
        prev = g
    assert lib.ocx_smart_grid_group(Lp, -1) < 0 and last_error(lib)
    assert lib.ocx_smart_grid_group(None, 3) < 0
    bad = _lib.Layout()
    ctypes.memmove(ctypes.byref(bad), Lp, ctypes.sizeof(L))
    bad.C = 5
    assert lib.ocx_smart_grid_group(ctypes.byref(bad), 3) < 0 and last_error(lib)


@pytest.mark.parametrize("name", sorted(BAD_CHECKPOINTS))
def test_host_entry_rejects_bad_checkpoints_before_the_gpu(name):
    lib = _lib.load()
    ck, ckp = i64(BAD_CHECKPOINTS[name])
    rc = lib.ocx_simulate_smart_grid_batch(DP, DP, 4, 10, 5, DP, 2, ckp, len(ck), 1.0, DP, None,
                                           1, 0)
    assert rc == -1 and last_error(lib), name


def test_host_entry_rejects_bad_counts_and_null_before_the_gpu():
    lib = _lib.load()
    ck, ckp = i64([1, 2])
    f = lib.ocx_simulate_smart_grid_batch
    for kw in (dict(M=-1), dict(K=-1), dict(th=None), dict(ck=None), dict(z=None), dict(B=-1),
               dict(reg=None)):
        a = dict(z=DP, B=4, th=DP, M=2, ck=ckp, K=2, reg=DP)
        a.update(kw)
        assert f(a["z"], DP, a["B"], 10, 5, a["th"], a["M"], a["ck"], a["K"], 1.0, a["reg"],
                 None, 1, 0) == -1, kw
        assert last_error(lib), kw
    # nothing to do: valid and no device needed
    assert f(DP, DP, 4, 10, 5, DP, 0, ckp, 2, 1.0, DP, None, 1, 0) == 0
    assert f(DP, DP, 4, 10, 5, DP, 2, ckp, 0, 1.0, DP, None, 1, 0) == 0
    assert f(DP, DP, 0, 10, 5, DP, 2, ckp, 2, 1.0, DP, None, 1, 0) == 0


def test_dev_and_test_entries_reject_bad_arguments_before_the_gpu():
    lib = _lib.load()
    L = _lib.layout(100, 10, 64, 8)
    K, M = 3, 5

    def rc(flags=0, K=K, M=M, th=BUF, ck=BUF, reg=BUF, z=BUF, Lp=ctypes.byref(L), group=None,
           wave=None):
        head = (Lp, z, BUF, th, M, ck, K, 1.0, reg, None, flags, None)
        if wave is not None:
            return lib.ocx_test_simulate_smart_wave_grid(*head, wave, None)
        if group is None:
            return lib.ocx_dev_simulate_smart_grid(*head, None)
        return lib.ocx_test_simulate_smart_grid(*head, group, None)

    for entry in (dict(), dict(group=2), dict(wave=2)):
        for kw in (dict(flags=0x80), dict(flags=4), dict(K=-1), dict(M=-1), dict(th=None),
                   dict(ck=None), dict(reg=None), dict(z=None), dict(Lp=None)):
            assert rc(**entry, **kw) == -1, (entry, kw)
            assert last_error(lib), (entry, kw)
        # M == 0, K == 0 and an empty batch are valid and launch nothing
        assert rc(**entry, K=0, ck=None) == 0
        assert rc(**entry, M=0, th=None) == 0
        L0 = _lib.layout(0, 10, 64, 8)
        assert rc(**entry, Lp=ctypes.byref(L0), z=None) == 0
    for group in (0, 3, 8, -1):
        assert rc(group=group) == -1 and last_error(lib), group
    for wave in (0, 3, 16, -1):
        assert rc(wave=wave) == -1 and last_error(lib), wave
    assert rc(wave=2, flags=_lib.OCX_SMART_CLOSED_PREFIX) == -1   # re-scan mode only
    # no group-2 or -4 form above 16 / 8 coordinates; no wave form above d = 64
    L32 = _lib.layout(100, 10, 1024, 32)
    assert L32.C == 32
    for group in (2, 4):
        assert rc(Lp=ctypes.byref(L32), group=group) == -3 and last_error(lib)   # unsupported
    assert rc(Lp=ctypes.byref(L32), group=1, K=0, ck=None) == 0
    L65 = _lib.layout(100, 10, 100, 1)
    assert rc(Lp=ctypes.byref(L65), wave=1) == -3 and last_error(lib)


C_TYPES = {"const ocx_layout*": ctypes.POINTER(_lib.Layout), "int64_t": _lib.c_i64,
           "int": ctypes.c_int, "double": ctypes.c_double}
HOST_TYPES = {"const double*": _lib.c_dp, "double*": _lib.c_dp, "const int64_t*": _lib.c_i64p,
              "int64_t*": _lib.c_i64p}


@pytest.mark.parametrize("header,table,sym,host", [
    ("ocx.h", "SIGNATURES", "ocx_smart_grid_group", False),
    ("ocx.h", "SIGNATURES", "ocx_dev_simulate_smart_grid", False),
    ("ocx.h", "SIGNATURES", "ocx_simulate_smart_grid_batch", True),
    ("ocx_testing.h", "TEST_SIGNATURES", "ocx_test_simulate_smart_grid", False),
    ("ocx_testing.h", "TEST_SIGNATURES", "ocx_test_simulate_smart_wave_grid", False)])
def test_header_declarations_agree_with_the_binding(header, table, sym, host):
    with open(os.path.join(ROOT, "include", header)) as f:
        txt = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"^int\s+" + sym + r"\s*\((.*?)\)\s*;", txt, flags=re.M | re.S)
    assert m, sym
    want = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", " ".join(arg.split()))   # drop the parameter's name
        if ctype in C_TYPES:
            want.append(C_TYPES[ctype])
        elif host and ctype in HOST_TYPES:
            want.append(HOST_TYPES[ctype])
        else:   # device pointers, stats and the stream travel as void*
            assert ctype.endswith("*"), (sym, arg)
            want.append(ctypes.c_void_p)
    restype, argtypes = getattr(_lib, table)[sym]
    assert restype is ctypes.c_int and list(argtypes) == want, (sym, argtypes, want)
    assert hasattr(_lib.load(), sym)


@pytest.mark.parametrize("bad", list(BAD_CHECKPOINTS.values()) + [[[1, 2]], [1.5, 2.0]])
def test_python_wrappers_raise_value_error_for_checkpoints(bad):
    z = np.zeros((4, 10, 5))
    y = np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_smart_grid_batch(z, y, bad, [1.0, 2.0], lanes_per_seq=1)
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, 4, bad, [1.0, 2.0])
    if bad != BAD_CHECKPOINTS["above_T"]:   # the driver's horizon is the last checkpoint
        with pytest.raises(ValueError):
            drivers.case_threshold_regret_grid("Label flips", bad, [1.0, 2.0], runs=2,
                                               replicates=2)


@pytest.mark.parametrize("bad", [[[[1.0]]], ["a", "b"], [None], 1.0, [1.0 + 2.0j]])
def test_python_wrappers_raise_value_error_for_thresholds(bad):
    z = np.zeros((4, 10, 5))
    y = np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_smart_grid_batch(z, y, [1, 5], bad, lanes_per_seq=1)
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, 4, [1, 5], bad)
    with pytest.raises(ValueError):
        drivers.case_threshold_regret_grid("Label flips", [1, 5], bad, runs=2, replicates=2)


def test_python_wrappers_validate_the_rest_and_the_empty_shapes():
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, 4, [1, 2], [1.0], base_seed=-1)
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, 4, [1, 2], [1.0], batch=0)
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, -1, [1, 2], [1.0])
    with pytest.raises(ValueError):
        engine.gT_smart_grids(10, 4, [1, 2], np.ones((4, 2)))    # one list for every run
    z, y = np.zeros((4, 10, 5)), np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_smart_grid_batch(z, y, [1, 2], np.ones((3, 2)))   # [B, M] needs B rows
    with pytest.raises(ValueError):
        engine.simulate_smart_grid_batch(z, np.ones((4, 9)), [1], [1.0])
    # nothing to compute: no device needed
    reg, sw = engine.simulate_smart_grid_batch(z, y, [], [1.0, 2.0], return_switch=True)
    assert reg.shape == sw.shape == (4, 2, 0) and sw.dtype == np.int64
    assert engine.simulate_smart_grid_batch(z, y, [1, 5], []).shape == (4, 0, 2)
    assert engine.simulate_smart_grid_batch(z[:0], y[:0], [1, 5], [1.0]).shape == (0, 1, 2)
    assert engine.gT_smart_grids(10, 0, [1, 2], [1.0]).shape == (0, 1, 2)
    assert engine.gT_smart_grids(10, 4, [], [1.0, 2.0]).shape == (4, 2, 0)
    reg, sw = engine.gT_smart_grids(10, 4, [1, 2], [], return_switch=True)
    assert reg.shape == sw.shape == (4, 0, 2) and sw.dtype == np.int64
    reg, sw = drivers.case_threshold_regret_grid("Label flips", [], [1.0], runs=2, replicates=3)
    assert reg.shape == sw.shape == (2, 3, 1, 0)
    reg, sw = drivers.case_threshold_regret_grid("Label flips", [4, 8], [], runs=2, replicates=3)
    assert reg.shape == sw.shape == (2, 3, 0, 2)
    reg, sw = drivers.case_threshold_regret_grid("Label flips", [4, 8], [1.0], runs=0,
                                                 replicates=3)
    assert reg.shape == sw.shape == (0, 3, 1, 2)
