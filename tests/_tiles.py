"""Host helpers for the engine's tiled HBM layout (include/ocx.h): reading a tile back into
rows, and building the tile a generator or the pack kernel must have written.

    z_tiled[((k*G + g)*T + t)*128 + L*2 + e] = z[b][t][c*C + 2k + e]     lane L = s*P + c
    y_tiled[(g*T + t)*S + s]                 = y[b][t]                   b = g*S + s

Padding (coordinates j >= d, sequences b >= B) is +0.0."""
import numpy as np


def untile_z(zt: np.ndarray, L) -> np.ndarray:
    """z_tiled (flat, (C/2)*G*T*128) → z [B, T, d]."""
    G, T, C, P, S = L.G, L.T, L.C, L.P, L.S
    a = zt.reshape(C // 2, G, T, S, P, 2)      # [k][g][t][s][c][e], lane = s*P + c
    a = a.transpose(1, 3, 2, 4, 0, 5)           # [g][s][t][c][k][e]
    a = a.reshape(G * S, T, P * C)              # j = c*C + 2k + e
    return a[:L.B, :, :L.d]


def untile_y(yt: np.ndarray, L) -> np.ndarray:
    a = yt.reshape(L.G, L.T, L.S).transpose(0, 2, 1).reshape(L.G * L.S, L.T)
    return a[:L.B]


def slots_z(zt: np.ndarray, L) -> np.ndarray:
    """untile_z without the cut: every sequence slot and padded coordinate, [G*S, T, P*C]
    (a copy; any 8-byte dtype, so bit patterns survive)."""
    G, T, C, P, S = int(L.G), int(L.T), int(L.C), int(L.P), int(L.S)
    a = np.asarray(zt)[:(C // 2) * G * T * 128].reshape(C // 2, G, T, S, P, 2)
    return a.transpose(1, 3, 2, 4, 0, 5).reshape(G * S, T, P * C)


def slots_y(yt: np.ndarray, L) -> np.ndarray:
    """untile_y without the cut: [G*S, T]."""
    G, T, S = int(L.G), int(L.T), int(L.S)
    return np.asarray(yt)[:G * T * S].reshape(G, T, S).transpose(0, 2, 1).reshape(G * S, T)


def tile_z(z, L) -> np.ndarray:
    """z [B, T, d] → z_tiled (flat float64, (C/2)*G*T*128), padding +0.0: untile_z's inverse."""
    B, T, d = int(L.B), int(L.T), int(L.d)
    G, C, P, S = int(L.G), int(L.C), int(L.P), int(L.S)
    a = np.zeros((G * S, T, P * C), dtype=np.float64)
    a[:B, :, :d] = np.asarray(z, dtype=np.float64).reshape(B, T, d)
    a = a.reshape(G, S, T, P, C // 2, 2)        # [g][s][t][c][k][e]
    a = a.transpose(4, 0, 2, 1, 3, 5)           # [k][g][t][s][c][e]
    return np.ascontiguousarray(a).reshape(-1)


def tile_y(y, L) -> np.ndarray:
    """y [B, T] → y_tiled (flat float64, G*T*S), padding sequences +0.0: untile_y's inverse."""
    B, T, G, S = int(L.B), int(L.T), int(L.G), int(L.S)
    a = np.zeros((G * S, T), dtype=np.float64)
    a[:B] = np.asarray(y, dtype=np.float64).reshape(B, T)
    return np.ascontiguousarray(a.reshape(G, S, T).transpose(0, 2, 1)).reshape(-1)


def gT_rows(base_seed: int, run0: int, B: int, T: int, d: int):
    """The g(T) sampler's batch in rows: z [B, T, d], y [B, T] of runs run0 .. run0 + B - 1
    (NumPy's own streams: oracle.gT_sample)."""
    from oracle import oracle as O
    z = np.zeros((B, T, d), dtype=np.float64)
    y = np.zeros((B, T), dtype=np.float64)
    for b in range(B):
        z[b], y[b] = O.gT_sample(int(base_seed), T, int(run0) + b, d)
    return z, y


def expected_gT_tiles(base_seed: int, run0: int, L, rows=None):
    """(z_tiled, y_tiled, y_bits) a g(T) generator must write for layout L: the tiles of
    sequences _rng(base_seed, L.T, run0 + b), b < L.B, padding +0.0 / zero bits.  rows: the
    (z, y) of gT_rows, if the caller already has them."""
    from tests._label_bits import tile_from_rows
    z, y = rows if rows is not None else gT_rows(base_seed, run0, int(L.B), int(L.T), int(L.d))
    return tile_z(z, L), tile_y(y, L), tile_from_rows(y, L)
