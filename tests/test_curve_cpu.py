"""CPU checks of the regret-curve entry points (include/ocx.h: ocx_curve_workspace_bytes,
ocx_dev_simulate_alg_curve, ocx_simulate_alg_curve_batch): workspace sizing and argument
checking are host logic and report through the error channel before a device or a data pointer
is touched (no GPU is needed here)."""
import ctypes

import numpy as np
import pytest

from online_convex_optimization_amd import _lib, engine

BUF = ctypes.c_void_p(16)  # never dereferenced: the checks come first


def last_error(lib):
    msg = ctypes.create_string_buffer(512)
    lib.ocx_last_error(msg, 512)
    return msg.value


def i64(vals):
    a = np.ascontiguousarray(vals, dtype=np.int64)
    return a, a.ctypes.data_as(_lib.c_i64p)


@pytest.mark.parametrize("B,T,d,lanes", [(24, 257, 5, 1), (24, 257, 64, -4), (37, 130, 64, 8),
                                         (24, 257, 1024, 64), (100, 10, 64, engine.LANES_BEST)])
def test_workspace_bytes(B, T, d, lanes):
    lib = _lib.load()
    L = _lib.layout(B, T, d, lanes)
    ws = [lib.ocx_curve_workspace_bytes(ctypes.byref(L), K) for K in range(0, min(T, 12) + 2)]
    assert ws[0] == 0
    assert all(b >= a for a, b in zip(ws, ws[1:])) and ws[1] > 0
    # room for theta (C words per lane), the loss and a flag per lane, group and checkpoint
    assert ws[1] >= L.G * 64 * (8 * L.C + 8 + 4)
    assert lib.ocx_curve_workspace_bytes(ctypes.byref(L), -1) < 0 and last_error(lib)
    assert lib.ocx_curve_workspace_bytes(ctypes.byref(L), T + 2) < 0  # more than horizons 0..T
    bad = _lib.Layout()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(L), ctypes.sizeof(L))
    bad.C = 5
    assert lib.ocx_curve_workspace_bytes(ctypes.byref(bad), 3) < 0 and last_error(lib)
    bad.C, bad.S = L.C, L.S + 1
    assert lib.ocx_curve_workspace_bytes(ctypes.byref(bad), 3) < 0
    assert lib.ocx_curve_workspace_bytes(None, 3) < 0
    # an empty batch needs none
    L0 = _lib.layout(0, T, d, lanes)
    assert lib.ocx_curve_workspace_bytes(ctypes.byref(L0), 5) == 0


BAD_CHECKPOINTS = {
    "decreasing": [5, 3],
    "repeated": [2, 2],
    "negative": [-1, 4],
    "above_T": [4, 11],
}


@pytest.mark.parametrize("name", sorted(BAD_CHECKPOINTS))
def test_host_entry_rejects_bad_checkpoints_before_the_gpu(name):
    lib = _lib.load()
    ck, ckp = i64(BAD_CHECKPOINTS[name])
    rc = lib.ocx_simulate_alg_curve_batch(
        ctypes.cast(BUF, _lib.c_dp), ctypes.cast(BUF, _lib.c_dp), 4, 10, 5, 0, 1.0, ckp, len(ck),
        ctypes.cast(BUF, _lib.c_dp), None, None, None, 1, 0)
    assert rc == -1 and last_error(lib), name


def test_host_entry_rejects_bad_K_and_null_before_the_gpu():
    lib = _lib.load()
    ck, ckp = i64([1, 2])
    z = y = out = ctypes.cast(BUF, _lib.c_dp)
    assert lib.ocx_simulate_alg_curve_batch(z, y, 4, 10, 5, 0, 1.0, ckp, -1, out, None, None,
                                            None, 1, 0) == -1 and last_error(lib)
    assert lib.ocx_simulate_alg_curve_batch(z, y, 4, 10, 5, 0, 1.0, None, 2, out, None, None,
                                            None, 1, 0) == -1 and last_error(lib)
    # valid checkpoints, NULL data: still refused on the host
    assert lib.ocx_simulate_alg_curve_batch(None, y, 4, 10, 5, 0, 1.0, ckp, 2, out, None, None,
                                            None, 1, 0) == -1 and last_error(lib)
    assert lib.ocx_simulate_alg_curve_batch(z, y, -1, 10, 5, 0, 1.0, ckp, 2, out, None, None,
                                            None, 1, 0) == -1
    # nothing to do: valid and no device needed
    assert lib.ocx_simulate_alg_curve_batch(z, y, 4, 10, 5, 0, 1.0, ckp, 0, out, None, None,
                                            None, 1, 0) == 0
    assert lib.ocx_simulate_alg_curve_batch(z, y, 0, 10, 5, 0, 1.0, ckp, 2, out, None, None,
                                            None, 1, 0) == 0


def test_dev_entry_rejects_bad_arguments_before_the_gpu():
    lib = _lib.load()
    L = _lib.layout(100, 10, 64, 8)
    K = 3
    need = lib.ocx_curve_workspace_bytes(ctypes.byref(L), K)
    assert need > 0

    def rc(flags=0, K=K, ck=BUF, ws=BUF, nbytes=need, z=BUF, Lp=ctypes.byref(L)):
        return lib.ocx_dev_simulate_alg_curve(Lp, z, BUF, 0, 1.0, ck, K, BUF, BUF, BUF, BUF,
                                              flags, ws, nbytes, None)

    for kw in (dict(flags=0x80), dict(flags=4), dict(nbytes=need - 1), dict(ws=None),
               dict(K=-1), dict(K=12), dict(ck=None), dict(z=None), dict(Lp=None),
               dict(ws=ctypes.c_void_p(12))):
        assert rc(**kw) == -1, kw
        assert last_error(lib), kw
    bad = _lib.Layout()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(L), ctypes.sizeof(L))
    bad.P = 3
    assert rc(Lp=ctypes.byref(bad)) == -1
    # K == 0 and an empty batch are valid and launch nothing
    assert rc(K=0, ck=None, ws=None, nbytes=0) == 0
    L0 = _lib.layout(0, 10, 64, 8)
    assert rc(Lp=ctypes.byref(L0), ws=None, nbytes=0, z=None) == 0


@pytest.mark.parametrize("bad", list(BAD_CHECKPOINTS.values()) + [[[1, 2]], [1.5, 2.0]])
def test_python_wrappers_raise_value_error(bad):
    z = np.zeros((4, 10, 5))
    y = np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.simulate_alg_curve_batch(z, y, bad, lanes_per_seq=1)
    with pytest.raises(ValueError):
        engine.gT_regret_curves(10, 4, bad)


def test_python_wrappers_validate_the_rest():
    with pytest.raises(ValueError):
        engine.gT_regret_curves(10, 4, [1, 2], base_seed=-1)
    with pytest.raises(ValueError):
        engine.gT_regret_curves(10, 4, [1, 2], batch=0)
    with pytest.raises(ValueError):
        engine.simulate_alg_curve_batch(np.zeros((4, 10, 5)), np.ones((4, 9)), [1])
    # nothing to compute: no device needed
    assert engine.gT_regret_curves(10, 0, [1, 2]).shape == (0, 2)
    assert engine.gT_regret_curves(10, 4, []).shape == (4, 0)
    assert engine.simulate_alg_curve_batch(np.zeros((4, 10, 5)), np.ones((4, 10)), []).shape == (4, 0)
    assert engine.simulate_alg_curve_batch(np.zeros((0, 10, 5)), np.ones((0, 10)), [1, 5]).shape \
        == (0, 2)
