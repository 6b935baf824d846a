"""CPU checks of the regret-grid entry points (include/ocx.h: ocx_curve_etas_group,
ocx_curve_etas_workspace_bytes, ocx_dev_simulate_alg_curve_etas,
ocx_simulate_alg_curve_etas_batch, ocx_dev_max_regret_cols): the group rule, workspace sizing
and argument checking are host logic and report through the error channel before a device or
a data pointer is touched (no GPU is needed here)."""
import ctypes

import numpy as np
import pytest

from online_convex_optimization_amd import _lib, engine
from tests.test_curve_cpu import BAD_CHECKPOINTS, BUF, i64, last_error

DP = ctypes.cast(BUF, _lib.c_dp)   # never dereferenced: the checks come first


@pytest.mark.parametrize("B,T,d,lanes", [(24, 257, 5, 1), (24, 257, 64, -4), (37, 130, 64, 8),
                                         (24, 257, 1024, 64), (100, 10, 64, engine.LANES_BEST),
                                         (24, 257, 16, 0), (24, 257, 256, -32), (24, 257, 512, -64),
                                         (24, 257, 32, 8), (24, 257, 64, 16)])
def test_group_and_workspace_bytes(B, T, d, lanes):
    lib = _lib.load()
    L = _lib.layout(B, T, d, lanes)
    Lp = ctypes.byref(L)
    C, P, chain = int(L.C), int(L.P), int(L.chain)
    # the step-size sweep's rule, less the two chained instances DESIGN.md §3.16 drops, and
    # group 2 where group 4 measured slower (8 x 4 pipelined)
    best = 4 if C <= 8 else (2 if C <= 16 else 1)
    if (chain and C == 8 and P == 32) or (not chain and (P, C) == (8, 4)):
        best = 2
    assert lib.ocx_curve_etas_group(Lp, 100) == best
    assert lib.ocx_curve_etas_group(Lp, 0) == lib.ocx_curve_etas_group(Lp, 1) == 1
    for M in range(1, 9):
        g = lib.ocx_curve_etas_group(Lp, M)
        assert g in (1, 2, 4) and g <= best and (g == 1 or g // 2 < M), (M, g)
        if chain and C == 8 and P == 64:
            assert g != 2   # not compiled there: two step sizes run one at a time
    assert lib.ocx_curve_etas_group(Lp, -1) < 0 and last_error(lib)
    assert lib.ocx_curve_etas_group(None, 3) < 0
    per_slot = int(L.G) * 64 * (8 * C + 12)
    for K in (0, 1, 3, min(T, 12) + 1):
        for M in (0, 1, 2, 3, 4, 7):
            want = per_slot * K * min(best, M)
            assert lib.ocx_curve_etas_workspace_bytes(Lp, K, M) == want, (K, M)
    assert lib.ocx_curve_etas_workspace_bytes(Lp, -1, 2) < 0 and last_error(lib)
    assert lib.ocx_curve_etas_workspace_bytes(Lp, 2, -1) < 0 and last_error(lib)
    assert lib.ocx_curve_etas_workspace_bytes(Lp, T + 2, 2) < 0   # more than horizons 0..T
    bad = _lib.Layout()
    ctypes.memmove(ctypes.byref(bad), Lp, ctypes.sizeof(L))
    bad.C = 5
    assert lib.ocx_curve_etas_workspace_bytes(ctypes.byref(bad), 3, 2) < 0 and last_error(lib)
    assert lib.ocx_curve_etas_workspace_bytes(None, 3, 2) < 0
    L0 = _lib.layout(0, T, d, lanes)   # an empty batch needs none
    assert lib.ocx_curve_etas_workspace_bytes(ctypes.byref(L0), 5, 4) == 0


@pytest.mark.parametrize("name", sorted(BAD_CHECKPOINTS))
def test_host_entry_rejects_bad_checkpoints_before_the_gpu(name):
    lib = _lib.load()
    ck, ckp = i64(BAD_CHECKPOINTS[name])
    rc = lib.ocx_simulate_alg_curve_etas_batch(DP, DP, 4, 10, 5, DP, 2, ckp, len(ck), DP, None,
                                               None, None, 1, 0)
    assert rc == -1 and last_error(lib), name


def test_host_entry_rejects_bad_counts_and_null_before_the_gpu():
    lib = _lib.load()
    ck, ckp = i64([1, 2])
    f = lib.ocx_simulate_alg_curve_etas_batch
    for kw in (dict(M=-1), dict(K=-1), dict(et=None), dict(ck=None), dict(z=None), dict(B=-1)):
        a = dict(z=DP, B=4, et=DP, M=2, ck=ckp, K=2)
        a.update(kw)
        assert f(a["z"], DP, a["B"], 10, 5, a["et"], a["M"], a["ck"], a["K"], DP, None, None,
                 None, 1, 0) == -1, kw
        assert last_error(lib), kw
    # nothing to do: valid and no device needed
    assert f(DP, DP, 4, 10, 5, DP, 0, ckp, 2, DP, None, None, None, 1, 0) == 0
    assert f(DP, DP, 4, 10, 5, DP, 2, ckp, 0, DP, None, None, None, 1, 0) == 0
    assert f(DP, DP, 0, 10, 5, DP, 2, ckp, 2, DP, None, None, None, 1, 0) == 0


def test_dev_entries_reject_bad_arguments_before_the_gpu():
    lib = _lib.load()
    L = _lib.layout(100, 10, 64, 8)
    K, M = 3, 5
    need = lib.ocx_curve_etas_workspace_bytes(ctypes.byref(L), K, M)
    assert need > 0

    def rc(flags=0, K=K, M=M, et=DP, ck=BUF, ws=BUF, nbytes=need, z=BUF, Lp=ctypes.byref(L),
           group=None):
        head = (Lp, z, BUF, et, M, ck, K, BUF, BUF, BUF, BUF, flags)
        if group is None:
            return lib.ocx_dev_simulate_alg_curve_etas(*head, ws, nbytes, None)
        return lib.ocx_test_simulate_alg_curve_etas(*head, group, ws, nbytes, None)

    for kw in (dict(flags=0x80), dict(flags=4), dict(nbytes=need - 1), dict(ws=None),
               dict(K=-1), dict(K=12), dict(M=-1), dict(et=None), dict(ck=None), dict(z=None),
               dict(Lp=None), dict(ws=ctypes.c_void_p(12)), dict(group=3), dict(group=0)):
        assert rc(**kw) == -1, kw
        assert last_error(lib), kw
    # forced groups: the workspace they need, and no group-2 or -4 form above 16 / 8 coordinates
    assert rc(group=1, nbytes=need // 4 - 1) == -1 and rc(group=2, nbytes=need // 2 - 1) == -1
    L32 = _lib.layout(100, 10, 1024, 32)
    assert L32.C == 32
    for group in (2, 4):
        assert rc(Lp=ctypes.byref(L32), group=group) == -3 and last_error(lib)   # unsupported
    # M == 0, K == 0 and an empty batch are valid and launch nothing
    assert rc(K=0, ck=None, ws=None, nbytes=0) == 0
    assert rc(M=0, et=None, ws=None, nbytes=0) == 0
    L0 = _lib.layout(0, 10, 64, 8)
    assert rc(Lp=ctypes.byref(L0), ws=None, nbytes=0, z=None) == 0
    # the column-wise maximum
    assert lib.ocx_dev_max_regret_cols(BUF, 4, 3, None, 0, None) == -1 and last_error(lib)
    assert lib.ocx_dev_max_regret_cols(None, 4, 3, BUF, 0, None) == -1
    assert lib.ocx_dev_max_regret_cols(BUF, -1, 3, BUF, 0, None) == -1
    assert lib.ocx_dev_max_regret_cols(BUF, 4, -1, BUF, 0, None) == -1
    assert lib.ocx_dev_max_regret_cols(None, 4, 0, None, 1, None) == 0   # no columns: nothing to do


@pytest.mark.parametrize("bad", list(BAD_CHECKPOINTS.values()) + [[[1, 2]], [1.5, 2.0]])
def test_python_wrappers_raise_value_error_for_checkpoints(bad):
    z = np.zeros((4, 10, 5))
    y = np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_alg_curve_etas_batch(z, y, bad, [1.0, 2.0], lanes_per_seq=1)
    with pytest.raises(ValueError):
        engine.gT_regret_curves_etas(10, 4, bad, [1.0, 2.0])
    with pytest.raises(ValueError):
        engine.gT_surface(10, 4, bad, [1.0, 2.0])


@pytest.mark.parametrize("bad", [[[1.0, 2.0]], ["a", "b"], [None], 1.0, [1.0 + 2.0j]])
def test_python_wrappers_raise_value_error_for_etas(bad):
    z = np.zeros((4, 10, 5))
    y = np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_alg_curve_etas_batch(z, y, [1, 5], bad, lanes_per_seq=1)
    with pytest.raises(ValueError):
        engine.gT_regret_curves_etas(10, 4, [1, 5], bad)
    with pytest.raises(ValueError):
        engine.gT_surface(10, 4, [1, 5], bad)


def test_python_wrappers_validate_the_rest():
    for f in (engine.gT_regret_curves_etas, engine.gT_surface):
        with pytest.raises(ValueError):
            f(10, 4, [1, 2], [1.0], base_seed=-1)
        with pytest.raises(ValueError):
            f(10, 4, [1, 2], [1.0], batch=0)
        with pytest.raises(ValueError):
            f(10, -1, [1, 2], [1.0])
    # nothing to compute: no device needed
    assert engine.gT_regret_curves_etas(10, 0, [1, 2], [1.0]).shape == (0, 1, 2)
    assert engine.gT_regret_curves_etas(10, 4, [], [1.0, 2.0]).shape == (4, 2, 0)
    reg, closed = engine.gT_regret_curves_etas(10, 4, [1, 2], [], return_closed=True)
    assert reg.shape == closed.shape == (4, 0, 2) and closed.dtype == np.int32
    assert engine.gT_surface(10, 0, [1, 2], [1.0, 2.0]).shape == (2, 2)
    assert np.all(engine.gT_surface(10, 0, [1, 2], [1.0, 2.0]) == 0.0)
    assert engine.gT_surface(10, 4, [], [1.0]).shape == (1, 0)
    z, y = np.zeros((4, 10, 5)), np.ones((4, 10))
    assert engine.simulate_alg_curve_etas_batch(z, y, [], [1.0]).shape == (4, 1, 0)
    assert engine.simulate_alg_curve_etas_batch(z, y, [1, 5], []).shape == (4, 0, 2)
    assert engine.simulate_alg_curve_etas_batch(z[:0], y[:0], [1, 5], [1.0]).shape == (0, 1, 2)
    with pytest.raises(ValueError):
        engine.simulate_alg_curve_etas_batch(z, np.ones((4, 9)), [1], [1.0])
