"""CPU checks for the one-wave-per-sequence SMART sweeps (NumPy, the C oracle and the ABI
only): the inputs of tests/test_gpu_smart_wave_cols.py (the sweeps' and, from
tests/_smart_wave_single_cases.py, the single call's) do what that file needs, and
include/ocx_testing.h declares ocx_test_simulate_smart_wave_cols with the argument list
_lib.py binds.

The bounds of the first test are the oracle's own minima over DIMS (5 sequences switched before
a MID9 horizon, at d = 8; 10 unswitched, at d = 64); a change of HZ9 or TH9 re-derives them from
the oracle, never from the kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from online_convex_optimization_amd import _lib
from tests import _smart_wave_cols_cases as W
from tests import _smart_wave_single_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d", W.DIMS)
def test_mid_horizons_cut_the_switch_steps_in_two(d):
    name = "gt_like"
    f = W.family(name, d)
    reg, sw = W.oracle_curve9(name, d)
    K = len(W.HZ9)
    assert reg.shape == sw.shape == (W.B, K)
    hz = np.array(W.HZ9)
    assert np.all((sw == -1) | ((sw >= 0) & (sw < hz[None, :])))
    before = np.array([(sw[:, k] >= 0).sum() for k in range(K)])
    print("switched before its horizon / not", d, before.tolist(), (W.B - before).tolist())
    mid = list(W.MID9)
    assert before[mid].min() >= 5, (d, before)
    assert (W.B - before[mid]).min() >= 10, (d, before)
    # where a truncated run switched, its step is the full run's
    full = np.stack([O.simulate_smart_batch(f.z, f.y, np.full(W.B, th), W.SQ2, nthreads=4)[1]
                     for th in W.TH9], axis=1)
    assert np.array_equal(sw[sw >= 0], full[sw >= 0]), d
    # the empty run; -1 would switch at step 0 had it a step
    assert np.all(reg[:, 0] == 0.0) and np.all(sw[:, 0] == -1)
    # +inf on the whole rows is FTL
    ftl = O.simulate_alg_batch(f.z, f.y, 1, W.SQ2, nthreads=4)[0]
    assert np.all(sw[:, K - 1] == -1) and np.array_equal(reg[:, K - 1], ftl)


@pytest.mark.parametrize("d", S.DIMS)
def test_single_call_switches_at_every_position_of_a_group(d):
    """What the single-threshold wave test needs of its inputs, from the oracle alone: at
    T = 67 the switch steps hit every position of a group of four speculated steps, the last
    (partial) group and -1; the shorter horizons run the same rows."""
    assert S.DIMS == (8, 9) and S.HORIZONS == (1, 3, 64, 67) and S.B % 4 and 24 <= S.B <= 48
    assert set(S.LAYOUTS) == {1, -1, -4, 8}
    z, y, th = S.inputs(d)
    assert z.shape == (S.B, 67, d) and y.shape == (S.B, 67) and len(set(th.tolist())) == S.B
    sw = S.oracle(d, 67)[1]
    on = sw[sw >= 0]
    print("switch steps", d, sorted(sw.tolist()))
    assert set((on % 4).tolist()) == {0, 1, 2, 3}, d
    assert np.any(on >= 64) and np.all(on < 67) and np.any(sw == -1), d
    # a truncated run switches where the full run does, if it gets there
    for T in S.HORIZONS[:-1]:
        reg_t, sw_t = S.oracle(d, T)
        assert reg_t.shape == sw_t.shape == (S.B,)
        assert np.array_equal(sw_t, np.where(sw < T, sw, -1)), (d, T)


def test_mid_horizons_sit_on_the_kernels_edges():
    """Horizons inside a group of four speculated steps, and on both sides of a 64-row chunk."""
    assert any(h % 4 for h in W.HZ9) and {63, 65} <= set(W.HZ9) and 0 in W.HZ9
    assert W.HZ9 == sorted(W.HZ9) and W.HZ9[-1] == W.T


# C type of a parameter -> its ctypes binding; `horizons` is the call's one host array
CTYPES = {"const ocx_layout*": ctypes.POINTER(_lib.Layout), "const double*": _lib.c_vp,
          "double*": _lib.c_vp, "int64_t*": _lib.c_vp, "unsigned long long*": _lib.c_vp,
          "void*": _lib.c_vp, "const int64_t*": _lib.c_i64p, "int64_t": _lib.c_i64,
          "double": _lib.c_double, "int": _lib.c_int}


def test_header_declares_what_the_binding_binds():
    with open(os.path.join(ROOT, "include", "ocx_testing.h")) as f:
        txt = f.read()
    m = re.search(r"^int\s+ocx_test_simulate_smart_wave_cols\s*\(([^)]*)\)\s*;", txt, flags=re.M)
    assert m, "ocx_testing.h does not declare ocx_test_simulate_smart_wave_cols"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names, types = [], []
    for p in params:
        ty, nm = re.fullmatch(r"(.*?)\s*(\w+)", p).groups()
        names.append(nm)
        types.append(ty.replace(" *", "*"))
    assert names == ["L", "z_tiled", "y_tiled", "horizons", "thresh", "M", "eta0", "regret",
                     "switch_step", "stats", "group", "stream"]
    res, args = _lib.TEST_SIGNATURES["ocx_test_simulate_smart_wave_cols"]
    assert res is _lib.c_int
    assert args == [CTYPES[t] for t in types], list(zip(names, types))
    lib = _lib.load()
    assert hasattr(lib, "ocx_test_simulate_smart_wave_cols")


def test_arguments_are_checked_before_the_gpu():
    lib = _lib.load()
    buf = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    L = _lib.layout(24, 257, 5, 1)
    hz = np.array([3, 9], dtype=np.int64)

    def rc(L, hz, M=2, group=2, th=buf, reg=buf, z=buf):
        hp = hz.ctypes.data_as(_lib.c_i64p) if hz is not None else None
        return lib.ocx_test_simulate_smart_wave_cols(ctypes.byref(L), z, buf, hp, th, M, 1.0,
                                                     reg, None, None, group, None)

    for group in (0, 3, 5, 16, -1):
        assert rc(L, hz, group=group) == -1 and "group" in _lib.last_error()
    assert rc(L, hz, M=-1) == -1
    assert rc(L, hz[::-1].copy()) == -1 and "non-decreasing" in _lib.last_error()
    assert rc(L, np.array([3, 258], dtype=np.int64)) == -1 and "outside" in _lib.last_error()
    assert rc(L, hz, th=None) == -1 and rc(L, hz, reg=None) == -1 and rc(L, hz, z=None) == -1
    assert rc(L, None, reg=None) == -1       # NULL horizons: the threshold sweep
    for d in (65, 100, 1024):
        assert rc(_lib.layout(24, 257, d, 1), hz) == -3, d
        assert "d <= 64" in _lib.last_error()
    assert rc(L, hz, M=0, reg=None) == 0     # nothing to do
