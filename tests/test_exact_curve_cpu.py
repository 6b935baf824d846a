"""CPU checks of the FTRL-vs-exact-FTL regret-curve entry points (include/ocx.h:
ocx_ftrl_exact_curve_workspace_bytes, ocx_dev_ftrl_vs_exact_curve,
ocx_ftrl_vs_exact_curve_batch) and of their Python wrappers: workspace sizing and argument
checking are host logic and report through the error channel before a device or a data pointer
is touched (no GPU is needed here)."""
import ctypes

import numpy as np
import pytest

from online_convex_optimization_amd import _lib, drivers, engine

BUF = ctypes.c_void_p(16)  # never dereferenced: the checks come first
DP = ctypes.cast(BUF, _lib.c_dp)
IP = ctypes.cast(BUF, ctypes.POINTER(ctypes.c_int32))


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
    f = lib.ocx_ftrl_exact_curve_workspace_bytes
    for wf in (0, 1):
        ws = [f(ctypes.byref(L), K, wf) for K in range(0, min(T, 12) + 2)]
        assert ws[0] == 0
        assert all(b > a for a, b in zip(ws, ws[1:]))          # monotone in K
        # theta_e (and theta_r with comp_ftl): C words per lane; a flag per lane; per group, K
        assert ws[1] >= L.G * 64 * (8 * L.C * (1 + wf) + 4)
        assert all(w % 8 == 0 for w in ws)
    assert f(ctypes.byref(L), 3, 1) > f(ctypes.byref(L), 3, 0)
    assert f(ctypes.byref(L), T + 1, 0) > 0                    # every horizon 0..T
    assert f(ctypes.byref(L), -1, 0) < 0 and last_error(lib)
    assert f(ctypes.byref(L), T + 2, 0) < 0 and last_error(lib)  # more than horizons 0..T
    bad = _lib.Layout()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(L), ctypes.sizeof(L))
    bad.C = 5
    assert f(ctypes.byref(bad), 3, 0) < 0 and last_error(lib)
    bad.C, bad.S = L.C, L.S + 1
    assert f(ctypes.byref(bad), 3, 0) < 0
    assert f(None, 3, 0) < 0
    # an empty batch needs none
    L0 = _lib.layout(0, T, d, lanes)
    assert f(ctypes.byref(L0), 5, 1) == 0


BAD_CHECKPOINTS = {
    "decreasing": [5, 3],
    "repeated": [2, 2],
    "negative": [-1, 4],
    "above_T": [4, 11],
}


def host_rc(lib, ckp, K, *, z=DP, y=DP, B=4, T=10, d=5, out=DP, rg=IP, norm=0, lanes=1):
    return lib.ocx_ftrl_vs_exact_curve_batch(z, y, B, T, d, 1.0, ckp, K, out, out, out, None, None,
                                             rg, None, norm, lanes, 0)


@pytest.mark.parametrize("name", sorted(BAD_CHECKPOINTS))
def test_host_entry_rejects_bad_checkpoints_before_the_gpu(name):
    lib = _lib.load()
    ck, ckp = i64(BAD_CHECKPOINTS[name])
    assert host_rc(lib, ckp, len(ck)) == -1 and last_error(lib), name


def test_host_entry_rejects_bad_arguments_before_the_gpu():
    lib = _lib.load()
    ck, ckp = i64([1, 2])
    assert host_rc(lib, ckp, -1) == -1 and last_error(lib)
    assert host_rc(lib, None, 2) == -1 and last_error(lib)
    assert host_rc(lib, ckp, 2, norm=3) == -1 and last_error(lib)
    assert host_rc(lib, ckp, 2, norm=-1) == -1
    # valid checkpoints, NULL data or required outputs: still refused on the host
    assert host_rc(lib, ckp, 2, z=None) == -1 and last_error(lib)
    assert host_rc(lib, ckp, 2, y=None) == -1
    assert host_rc(lib, ckp, 2, out=None) == -1 and last_error(lib)
    assert host_rc(lib, ckp, 2, rg=None) == -1
    assert host_rc(lib, ckp, 2, B=-1) == -1
    # nothing to do: valid and no device needed
    assert host_rc(lib, ckp, 0) == 0
    assert host_rc(lib, ckp, 2, B=0) == 0


def test_dev_entry_rejects_bad_arguments_before_the_gpu():
    lib = _lib.load()
    L = _lib.layout(100, 10, 64, 8)
    K = 3
    need = lib.ocx_ftrl_exact_curve_workspace_bytes(ctypes.byref(L), K, 0)
    need_f = lib.ocx_ftrl_exact_curve_workspace_bytes(ctypes.byref(L), K, 1)
    assert 0 < need < need_f

    def rc(flags=0, K=K, ck=BUF, ws=BUF, nbytes=need_f, z=BUF, Lp=ctypes.byref(L), norm=0,
           cum=BUF, rg=BUF, cf=None):
        return lib.ocx_dev_ftrl_vs_exact_curve(Lp, z, BUF, 1.0, ck, K, cum, BUF, BUF, cf, None, rg,
                                               None, norm, flags, ws, nbytes, None)

    for kw in (dict(flags=0x80), dict(flags=8), dict(nbytes=need - 1), dict(ws=None),
               dict(K=-1), dict(K=12), dict(ck=None), dict(z=None), dict(Lp=None),
               dict(ws=ctypes.c_void_p(12)), dict(norm=3), dict(norm=-1), dict(cum=None),
               dict(rg=None),
               dict(cf=BUF, nbytes=need)):   # comp_ftl asks for the larger workspace
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
        engine.ftrl_vs_exact_curve_batch(z, y, bad, lanes_per_seq=1)
    if bad != BAD_CHECKPOINTS["above_T"]:
        # the driver's horizon is max(T_grid): it refuses everything but a large value
        with pytest.raises(ValueError):
            drivers.exact_case_regret_curves("Label flips", bad, runs=1, replicates=1)


def test_python_wrappers_validate_the_rest():
    z, y = np.zeros((4, 10, 5)), np.ones((4, 10))
    with pytest.raises(ValueError):
        engine.ftrl_vs_exact_curve_batch(z, y, [1, 2], norm="l3")
    with pytest.raises(ValueError):
        engine.ftrl_vs_exact_curve_batch(z, np.ones((4, 9)), [1])
    with pytest.raises(ValueError):
        engine.ftrl_vs_exact_curve_batch(np.zeros((4, 10)), y, [1])
    # nothing to compute: no device needed
    for zz, yy, ck, shape in ((z, y, [], (4, 0)),
                              (np.zeros((0, 10, 5)), np.ones((0, 10)), [1, 5], (0, 2))):
        out = engine.ftrl_vs_exact_curve_batch(zz, yy, ck, with_ftl_comparator=True)
        for k in ("ftrl", "exact", "cum_ftrl", "cum_exact", "comp", "comp_ftl", "in_regime",
                  "closed"):
            assert out[k].shape == shape, k
        assert out["action"].shape == shape + (5,) and out["exact_gap_max"] == 0.0
    r = drivers.exact_case_regret_curves("Label flips", [], runs=2, replicates=2)
    assert r["FTRL"].shape == r["FTL (exact)"].shape == (4, 0)
    r = drivers.exact_case_regret_curves("Label flips", [5, 10], runs=0, replicates=2)
    assert r["FTRL"].shape == (0, 2)
