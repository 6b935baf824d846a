"""The host-side tile builders of tests/_tiles.py, which the generator conformance suite
(tests/test_gpu_gen_tiles.py) compares the device tiles with: they invert the readers the
older tests use, index the layout as include/ocx.h states it, and keep padding +0.0.  Also the
two environment names that suite relies on to shrink a generator launch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _label_bits as LB
from tests._tiles import (expected_gT_tiles, slots_y, slots_z, tile_y, tile_z, untile_y,
                          untile_z)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_layout(B, T, d, P, C):
    S = 64 // P
    G = -(-B // S)
    assert P * S == 64 and C % 2 == 0 and P * C >= d
    return SimpleNamespace(B=B, T=T, d=d, P=P, C=C, S=S, G=G, Dp=P * C, chain=0,
                           z_elems=G * T * 64 * C, y_elems=G * T * S)


# (B, T, d, P, C): P in {1, 4, 8, 64}; P*C not a power of two (d = 5: 1 x 6; d = 33: 4 x 12);
# B not a multiple of S (and one that is); T in {0, 1, 65}
LAYOUTS = [(70, 65, 5, 1, 6), (70, 1, 5, 1, 6), (3, 0, 5, 1, 6), (1, 65, 5, 1, 6),
           (70, 65, 5, 4, 2), (37, 1, 33, 4, 12), (16, 65, 64, 4, 16), (5, 0, 64, 4, 16),
           (203, 65, 64, 8, 8), (9, 1, 16, 8, 2), (11, 65, 100, 8, 16), (8, 0, 64, 8, 8),
           (5, 65, 64, 64, 2), (3, 1, 1024, 64, 16), (2, 0, 128, 64, 2), (1, 65, 65, 64, 2)]


@pytest.mark.parametrize("B,T,d,P,C", LAYOUTS)
def test_tile_inverts_untile_and_indexes_the_layout(B, T, d, P, C):
    L = make_layout(B, T, d, P, C)
    rng = np.random.default_rng(B * 100000 + T * 1000 + d)
    z = rng.standard_normal((B, T, d))
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    zt, yt = tile_z(z, L), tile_y(y, L)
    assert zt.shape == (L.z_elems,) and yt.shape == (L.y_elems,)
    assert zt.dtype == np.float64 and yt.dtype == np.float64
    assert np.array_equal(untile_z(zt, L), z)
    assert np.array_equal(untile_y(yt, L), y)
    # the formula of include/ocx.h, element by element on a sample of indices
    S, G = L.S, L.G
    for _ in range(200 if T else 0):
        b, t, j = int(rng.integers(G * S)), int(rng.integers(T)), int(rng.integers(P * C))
        g, s, c, k, e = b // S, b % S, j // C, (j % C) // 2, j % 2
        want = z[b, t, j] if (b < B and j < d) else 0.0
        assert zt[((k * G + g) * T + t) * 128 + (s * P + c) * 2 + e] == want
        assert yt[(g * T + t) * S + s] == (y[b, t] if b < B else 0.0)
    # padding is +0.0 as a bit pattern, and there is exactly the real data beside it
    zs, ys = slots_z(zt.view(np.int64), L), slots_y(yt.view(np.int64), L)
    assert not zs[B:].any() and not zs[:, :, d:].any() and not ys[B:].any()
    assert np.array_equal(zs[:B, :, :d], z.view(np.int64))


@pytest.mark.parametrize("B,T,d,P,C", LAYOUTS)
def test_untile_inverts_tile_on_zero_padded_tiles(B, T, d, P, C):
    L = make_layout(B, T, d, P, C)
    rng = np.random.default_rng(B * 100000 + T * 1000 + d + 1)
    # a tile made directly in tiled order: random everywhere, then padding zeroed in place
    zt = rng.standard_normal(L.z_elems)
    yt = rng.standard_normal(L.y_elems)
    zv = zt.reshape(C // 2, L.G, T, L.S, P, 2)
    yv = yt.reshape(L.G, T, L.S)
    for g in range(L.G):
        for s in range(L.S):
            if g * L.S + s >= B:
                zv[:, g, :, s] = 0.0
                yv[g, :, s] = 0.0
    for c in range(P):
        for k in range(C // 2):
            for e in range(2):
                if c * C + 2 * k + e >= d:
                    zv[k, :, :, :, c, e] = 0.0
    assert np.array_equal(tile_z(untile_z(zt, L), L).view(np.int64), zt.view(np.int64))
    assert np.array_equal(tile_y(untile_y(yt, L), L).view(np.int64), yt.view(np.int64))


def test_expected_tiles_are_the_oracle_streams():
    from oracle import oracle as O
    L = make_layout(11, 70, 5, 4, 2)
    zt, yt, bits = expected_gT_tiles(3, 9, L)
    z, y = untile_z(zt, L), untile_y(yt, L)
    for b in range(L.B):
        zr, yr = O.gT_sample(3, 70, 9 + b, 5)
        assert np.array_equal(z[b], zr) and np.array_equal(y[b], yr)
    assert bits.dtype == np.uint64 and bits.shape == (LB.words(L),)
    assert np.array_equal(bits, LB.tile_from_tiled(yt, L))
    assert np.array_equal(LB.rows_from_tile(bits, L), y)


def test_generator_reads_the_two_wave_count_knobs():
    """tests/test_gpu_gen_tiles.py shrinks a launch to a few waves through these two names; a
    renamed knob would silently turn its cases back into one-sequence-per-wave runs."""
    src = open(os.path.join(ROOT, "online_convex_optimization_amd", "csrc", "ocx_gen_wave.hip")).read()
    assert 'getenv("OCX_GEN_CUS")' in src
    assert 'getenv("OCX_GEN_WAVES_PER_SIMD")' in src
