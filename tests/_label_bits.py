"""Host-side arithmetic of the label-bit tile (include/ocx.h), as NumPy references for the
tests: one 64-bit word per wave-group g, 64-step block k and sequence slot s,

    y_bits[(g*ceil(T/64) + k)*S + s]  bit (t mod 64)  =  (y[g*S + s][64k + (t mod 64)] == +1)

with the bits at t >= T and of padding sequences 0."""
import numpy as np


def words(L) -> int:
    return int(L.G) * ((int(L.T) + 63) // 64) * int(L.S)


def tile_from_rows(y, L) -> np.ndarray:
    """The tile of row-major labels y [B][T] for layout L (uint64 [words(L)])."""
    B, T, S, G = int(L.B), int(L.T), int(L.S), int(L.G)
    KB = (T + 63) // 64
    y = np.asarray(y, dtype=np.float64).reshape(B, T)
    plus = np.zeros((G * S, KB * 64), dtype=np.uint64)
    plus[:B, :T] = (y == 1.0)
    w = plus.reshape(G, S, KB, 64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(w, axis=3).transpose(0, 2, 1).reshape(-1)  # [g][k][s]


def tile_from_tiled(y_tiled, L) -> np.ndarray:
    """The tile of a y_tiled buffer (y_tiled[(g*T + t)*S + s] = y[g*S + s][t]; padding 0.0)."""
    T, S, G = int(L.T), int(L.S), int(L.G)
    yt = np.asarray(y_tiled, dtype=np.float64)[:G * T * S].reshape(G, T, S)
    rows = yt.transpose(0, 2, 1).reshape(G * S, T)  # padding sequences: zeros, so no bit
    KB = (T + 63) // 64
    plus = np.zeros((G * S, KB * 64), dtype=np.uint64)
    plus[:, :T] = (rows == 1.0)
    w = plus.reshape(G, S, KB, 64) << np.arange(64, dtype=np.uint64)
    return np.bitwise_or.reduce(w, axis=3).transpose(0, 2, 1).reshape(-1)


def rows_from_tile(bits, L) -> np.ndarray:
    """The ±1 labels [B][T] a tile stands for."""
    B, T, S, G = int(L.B), int(L.T), int(L.S), int(L.G)
    KB = (T + 63) // 64
    w = np.asarray(bits, dtype=np.uint64)[:G * KB * S].reshape(G, KB, S)
    b = (w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)  # [g][k][s][i]
    b = b.transpose(0, 2, 1, 3).reshape(G * S, KB * 64)[:B, :T]
    return np.where(b == 1, 1.0, -1.0)
