"""CPU checks of the C ABI: libocx.so loads, exports every symbol include/ocx.h declares,
the ctypes binding covers them, and layout planning (pure host logic) is right."""
import os
import re
import subprocess

import numpy as np
import pytest

from online_convex_optimization_amd import _lib
from tests._tiles import untile_y, untile_z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="ocx.h"):
    with open(os.path.join(ROOT, "include", header)) as f:
        txt = f.read()
    return sorted(set(re.findall(r"^\s*(?:int|int64_t)\s+(ocx_\w+)\s*\(", txt, flags=re.M)))


@pytest.mark.parametrize("header,table", [("ocx.h", "SIGNATURES"),
                                          ("ocx_testing.h", "TEST_SIGNATURES")])
def test_library_exports_every_declared_symbol(header, table):
    lib = _lib.load()
    syms = declared_symbols(header)
    assert len(syms) >= (14 if header == "ocx.h" else 1)
    for s in syms:
        assert hasattr(lib, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (ocx_\w+)$", out, flags=re.M))
    assert set(syms) <= exported
    sig = getattr(_lib, table)
    assert set(syms) == set(sig), set(syms) ^ set(sig)


def test_version_and_error_channel():
    with open(os.path.join(ROOT, "include", "ocx.h")) as f:
        ver = int(re.search(r"#define OCX_VERSION (\d+)", f.read()).group(1))
    assert _lib.load().ocx_version() == ver == _lib.OCX_VERSION == 400
    with pytest.raises(ValueError):
        _lib.layout(-1, 10, 5)
    assert "negative" in _lib.last_error()


@pytest.mark.parametrize("B,T,d,P", [(1, 1000, 5, 1), (32768, 10000, 64, 0), (65536, 1000, 16, 0),
                                     (2048, 10, 1024, 0), (100, 7, 3, 4), (5, 3, 0, 0),
                                     (7, 3, 100, -2), (9, 4, 64, -1)])
def test_layout(B, T, d, P):
    L = _lib.layout(B, T, d, P)
    assert L.P * L.S == 64 and L.C % 2 == 0 and L.Dp == L.P * L.C >= d
    assert L.G == -(-B // L.S)
    assert L.z_elems == L.G * T * 64 * L.C and L.y_elems == L.G * T * L.S
    if P > 1 or P < 0:
        assert L.P == abs(P)
    assert L.chain == (1 if (P == 1 or P < 0) and L.P > 1 else 0)


def test_auto_layout_choices():
    assert (_lib.layout(32768, 10, 64).P, _lib.layout(32768, 10, 64).C) == (4, 16)
    assert _lib.layout(1 << 20, 10, 64).P == 4          # at most 16 coordinates per lane
    assert _lib.layout(1 << 20, 10, 16).P == 1          # enough sequences: one lane each
    assert _lib.layout(1, 10, 5).C == 2                 # lanes keep >= 2 coordinates
    assert _lib.layout(8, 10, 4096).C == 64             # d/P <= 64
    with pytest.raises(_lib.OCXError):
        _lib.layout(1, 10, 5000)
    ex = _lib.layout(3, 10, 1000, 1)                     # exact mode, d >= 512: 32 coords/lane
    assert (ex.P, ex.C, ex.chain) == (32, 32, 1)
    ex = _lib.layout(3, 10, 300, 1)                      # exact mode below: 16 coords/lane
    assert (ex.P, ex.C, ex.chain) == (32, 16, 1)
    assert _lib.layout(3, 10, 64, -1).chain == 0          # exact, one lane per sequence
    ch = _lib.layout(3, 10, 64, 1)                         # exact, auto lanes: chained
    assert ch.chain == 1 and ch.P == 8 and ch.C == 8       # few waves: 8 lanes
    assert _lib.layout(3, 10, 16, 1).P == 4                # keeps >= 8 coords to go past 4
    assert _lib.layout(8192, 10, 64, 1).P == 4             # 32768 lanes at 4 lanes
    assert (_lib.layout(65536, 10, 16, 1).P, _lib.layout(65536, 10, 16, 1).chain) == (1, 0)
    assert _lib.layout(32768, 10, 64, 1).P == 4
    assert _lib.layout(5, 10, 1024, 1).P == 32
    assert _lib.layout(3, 10, 5, -4).C == 2 and _lib.layout(3, 10, 5, -4).chain == 1
    assert _lib.layout(3, 10, 12, -2).C == 8                # chain C is a power of two


def test_best_layout_choices():
    """OCX_LANES_BEST (128): the exact layout while its chains stay under 8 lanes, except
    the big batches at 64 <= d <= 128 (>= 4096 sequences); else butterfly sums with 8
    coordinates per lane up to d = 128 (4 below 4096 sequences), 32 from d = 512."""
    best = 128
    L = _lib.layout(32768, 10, 64, best)       # the bench batch: butterfly 8 x 8
    assert (L.P, L.C, L.chain) == (8, 8, 0)
    L = _lib.layout(32768, 10, 64, 1)          # its exact layout: a 4-lane chain
    assert (L.P, L.C, L.chain) == (4, 16, 1)
    L = _lib.layout(32768, 10, 32, best)       # d < 64: exact
    assert L.chain == 1 or L.P == 1
    L = _lib.layout(65536, 10, 16, best)       # configs[1]: exact, one lane per sequence
    assert (L.P, L.chain) == (1, 0)
    L = _lib.layout(768, 10, 5, best)          # the drivers' batches: exact
    assert (L.P, L.C, L.chain) == (4, 2, 1)
    L = _lib.layout(4900, 10, 64, best)        # few-wave (T = 1e5 batch): butterfly 8 x 8
    assert (L.P, L.C, L.chain) == (8, 8, 0)
    L = _lib.layout(3328, 10, 64, best)        # fewer: twice the waves, 16 x 4
    assert (L.P, L.C, L.chain) == (16, 4, 0)
    L = _lib.layout(2048, 10, 1024, best)      # configs[4]: butterfly 32 x 32
    assert (L.P, L.C, L.chain) == (32, 32, 0)
    L = _lib.layout(500, 10, 200, best)        # between: 16 coordinates per lane
    assert (L.P, L.C, L.chain) == (16, 16, 0)
    L = _lib.layout(1, 10, 3, best)            # a single short sequence: exact
    assert L.P * L.C >= 3 and (L.P == 1 or L.chain == 1)


def test_untile_roundtrip_matches_pack_formula():
    # host restatement of ocx_pack_z_kernel's plane-major index map, inverted by untile_z
    B, T, d = 37, 5, 11
    for P in (1, 2, 4, 8, 64):
        L = _lib.layout(B, T, d, P)
        rng = np.random.default_rng(P)
        z = rng.standard_normal((B, T, d))
        y = rng.standard_normal((B, T))
        zt = np.zeros(L.z_elems)
        o = np.arange(L.z_elems)
        row, lane, e = o >> 7, (o & 127) >> 1, o & 1
        kg, t = row // T, row % T
        k, g = kg // L.G, kg % L.G
        b = g * L.S + lane // L.P
        j = (lane % L.P) * L.C + 2 * k + e
        ok = (b < B) & (j < d)
        zt[ok] = z[b[ok], t[ok], j[ok]]
        assert np.array_equal(untile_z(zt, L), z)
        yt = np.zeros(L.y_elems)
        o = np.arange(L.y_elems)
        tix, s = o // L.S, o % L.S
        g, t = tix // T, tix % T
        b = g * L.S + s
        ok = b < B
        yt[ok] = y[b[ok], t[ok]]
        assert np.array_equal(untile_y(yt, L), y)


def test_positive_double_bit_patterns_order_as_values():
    """ocx_gT_max folds regrets with a 64-bit unsigned atomic max over their bit patterns
    (csrc/ocx_capi.hip ocx_max_fold_kernel): only values > +0.0 reach it, and for those
    (subnormals, normals, +inf) the unsigned order of the patterns is the order of the
    values, so the fold selects the same element as fast_algorithms.py:242-243's `>` loop."""
    rng = np.random.default_rng(7)
    v = np.abs(rng.standard_normal(20000)) * 10.0 ** rng.integers(-320, 300, 20000)
    v = np.concatenate([v[v > 0.0], [5e-324, 2.2250738585072014e-308, 1.0, np.inf]])
    bits = v.view(np.uint64)
    order_v = np.argsort(v, kind="stable")
    order_b = np.argsort(bits, kind="stable")
    assert np.array_equal(v[order_v], v[order_b])
    assert v[np.argmax(bits)] == v.max()


def test_gen_simulate_rejects_bad_arguments_before_the_gpu():
    """ocx_dev_gen_simulate checks its arguments on the host (unknown flags, NULL regret,
    negative run0 / nbatch) and reports them through the error channel without touching a
    device (this container has none)."""
    import ctypes
    lib = _lib.load()
    L = _lib.layout(100, 10, 64, 8)
    buf = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    cases = [(0, 1, 0x80, buf), (0, 1, 0, None), (-1, 1, 0, buf), (0, -1, 0, buf)]
    for run0, nbatch, flags, reg in cases:
        rc = lib.ocx_dev_gen_simulate(ctypes.byref(L), 0, run0, nbatch, buf, buf, 1.0, reg, None,
                                      flags, 0, None)
        assert rc == -1, (run0, nbatch, flags, reg)
        msg = ctypes.create_string_buffer(256)
        lib.ocx_last_error(msg, 256)
        assert msg.value, (run0, nbatch, flags)


def test_alg_range_rejects_bad_arguments_before_the_gpu():
    """ocx_test_alg_range takes the layouts the sub-batch pipeline's FTRL launch runs (8 x 8,
    16 x 4, 8 x 4, 8 x 2) and group ranges inside the layout; everything else is reported
    through the error channel before a device is touched."""
    import ctypes
    lib = _lib.load()
    buf = ctypes.c_void_p(16)  # never dereferenced: the checks come first

    def rc(L, onepass, g0, gn, reg=buf):
        return lib.ocx_test_alg_range(ctypes.byref(L), buf, buf, 1.0, onepass, g0, gn, reg, None,
                                      None)

    for d, P in ((64, 32), (128, 8), (64, -8), (16, 4), (16, -8), (1024, 64)):
        assert rc(_lib.layout(37, 10, d, P), 1, 0, 1) == -3, (d, P)
    for d, P in ((64, 8), (64, 16), (32, 8), (16, 8)):
        L = _lib.layout(37, 10, d, P)
        assert rc(L, 1, -1, 1) == -1 and rc(L, 1, 0, L.G + 1) == -1 and rc(L, 1, L.G, 1) == -1
        assert rc(L, 1, 0, -1) == -1 and rc(L, 2, 0, 1) == -1 and rc(L, 0, 0, 1, None) == -1
        assert _lib.last_error()
