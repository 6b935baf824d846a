"""CPU twin of tests/test_gpu_label_bits.py: the label-bit tile's host-side arithmetic — its
size query (ocx_label_bits_words, pure host logic), the NumPy references the GPU tests compare
the kernels' tiles with, and the new entry points' argument checks that fail before any GPU
work."""
import ctypes

import numpy as np
import pytest

from online_convex_optimization_amd import _lib
from tests import _label_bits as LB
from tests._tiles import untile_y

SHAPES = [(1, 1, 64, 8), (8, 63, 64, 8), (24, 64, 64, 16), (2051, 65, 64, 8), (59, 130, 64, 8),
          (21, 1000, 64, 16), (7, 130, 5, 0), (5, 200, 1024, 64), (3, 0, 64, 8), (0, 70, 64, 8)]


@pytest.mark.parametrize("B,T,d,P", SHAPES)
def test_words_query_matches_the_layout_formula(B, T, d, P):
    L = _lib.layout(B, T, d, P)
    n = _lib.load().ocx_label_bits_words(ctypes.byref(L))
    assert n == L.G * ((T + 63) // 64) * L.S == LB.words(L)
    # 1/64 of y_tiled when T is a multiple of 64, never more than one word per 64 labels + 1
    assert n * 64 >= L.y_elems and n <= L.y_elems // 64 + L.G * L.S


def test_words_query_rejects_a_corrupt_layout():
    L = _lib.layout(8, 64, 64, 8)
    L.S = 3
    assert _lib.load().ocx_label_bits_words(ctypes.byref(L)) < 0
    assert _lib.load().ocx_label_bits_words(None) < 0


@pytest.mark.parametrize("B,T,d,P", [s for s in SHAPES if s[0] and s[1]])
def test_reference_tiles_agree_and_round_trip(B, T, d, P):
    """The tile built from row-major labels equals the one built from y_tiled, decodes back to
    the labels, and keeps every bit at t >= T and of the padding sequences 0."""
    L = _lib.layout(B, T, d, P)
    rng = np.random.default_rng(B * 1000 + T)
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    S, G, KB = L.S, L.G, (T + 63) // 64
    yt = np.zeros(G * T * S)
    yt.reshape(G, T, S)[...] = np.pad(y, ((0, G * S - B), (0, 0))).reshape(G, S, T).transpose(0, 2, 1)
    assert np.array_equal(untile_y(yt, L), y)
    a, b = LB.tile_from_rows(y, L), LB.tile_from_tiled(yt, L)
    assert a.dtype == np.uint64 and a.shape == (LB.words(L),)
    assert np.array_equal(a, b)
    assert np.array_equal(LB.rows_from_tile(a, L), y)
    w = a.reshape(G, KB, S)
    if T % 64:
        assert np.all(w[:, KB - 1, :] >> np.uint64(T % 64) == 0)
    pad = np.arange(G * S).reshape(G, S) >= B
    assert np.all(w.transpose(0, 2, 1)[pad] == 0)
    # word (g, k, s), bit i is label y[g*S + s][64k + i]
    g, k, s, i = G - 1, KB - 1, 0, (T - 1) % 64
    assert ((int(w[g, k, s]) >> i) & 1) == int(y[g * S + s, 64 * k + i] == 1.0)


def test_a_label_that_is_not_unit_sets_no_bit():
    """The reference marks +1 only: a 0.5 or 0.0 label reads as 'not +1' (the pack kernel's
    flag, not the tile, is what rejects such a batch)."""
    L = _lib.layout(8, 64, 64, 8)
    y = np.ones((8, 64))
    y[3, 10] = 0.5
    y[4, 63] = -1.0
    w = LB.tile_from_rows(y, L).reshape(L.G, 1, L.S)
    assert int(w[0, 0, 3]) == (1 << 64) - 1 - (1 << 10)
    assert int(w[0, 0, 4]) == (1 << 63) - 1


def test_new_entries_reject_bad_arguments_before_the_gpu():
    lib = _lib.load()
    L = _lib.layout(8, 64, 64, 8)
    one = ctypes.c_void_p(8)
    # ocx_dev_pack_bits: the flag and the tile are required
    assert lib.ocx_dev_pack_bits(ctypes.byref(L), one, one, one, one, one, None, None) == -1
    assert lib.ocx_dev_pack_bits(ctypes.byref(L), one, one, one, one, None, one, None) == -1
