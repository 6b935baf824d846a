"""Batched API of the MI355X engine (new surface; the reference has only scalar calls).

Two ways in:

* host arrays (numpy) — ``simulate_alg_batch``, ``simulate_smart_batch``,
  ``replay_batch``, ``gT_regrets``: one synchronous call per batch, results back
  as numpy;
* device-resident batches — ``DeviceBatch``: z/y live in HBM in the engine's tiled
  layout (``include/ocx.h``), generated on device or packed once, then simulated
  any number of times without touching the host.  Device memory and streams come
  from PyTorch (plumbing only); every kernel is the HIP code in ``csrc/``.

Every batched call defaults to ``lanes_per_seq=LANES_BEST`` (include/ocx.h,
OCX_LANES_BEST), the fastest certified mode: the exact layout's sequential sums wherever its
lane chains are short and d < 64 (every d <= 16 batch, the drivers' d=5 batches), butterfly
sums (~1e-16 relative) where an exact chain of 8+ lanes would leave the kernel latency-bound
(d >= 512, few-wave batches such as the capacity-limited T=1e5 g(T) batch) and for batches
of >= 4096 sequences at 64 <= d <= 128 (the pipelined 8 x 8 kernel: the bench's 32 768 x 1e4
batch), and — for the g(T), DeviceBatch and FTRL-vs-exact
paths — the closed-form comparator losses wherever the kernel certifies them (one HBM pass
instead of two; about 1e-13 relative on the regret).  LANES_BEST results are therefore NOT
bit-identical to the reference.  ``lanes_per_seq=1`` forces the bit-exact mode (sequential
sums, streamed comparator pass); the drop-in modules (fast_algorithms, exact_ftl) always use
it.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import ptr

SQRT2 = math.sqrt(2.0)
LANES_BEST = 128  # OCX_LANES_BEST: exact where it streams at the roofline, butterfly elsewhere
LANES_EXACT = 1   # bit-identical to the reference's sequential sums


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _check_zy(z: np.ndarray, y: np.ndarray):
    if z.ndim != 3:
        raise ValueError(f"z must be [B, T, d], got shape {z.shape}")
    B, T, d = z.shape
    if y.shape != (B, T):
        raise ValueError(f"y must be [B, T] = {(B, T)}, got {y.shape}")
    return B, T, d


def simulate_alg_batch(z, y, alg_flag: int = 0, eta0: float = SQRT2, comparator=None, *,
                       lanes_per_seq: int = LANES_BEST, device: int = 0, return_all: bool = False):
    """fast_algorithms.py:88-115 over B independent sequences on one GPU.

    z [B, T, d], y [B, T]; comparator [B, d] optional (exact_ftl.py:266-269).
    Returns regret [B] or, with ``return_all``, (regret, cum_loss, comp_loss, x_last)."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    cmp = None
    if comparator is not None:
        cmp = _f64(comparator)
        if cmp.shape != (B, d):
            raise ValueError(f"comparator must be [B, d] = {(B, d)}, got {cmp.shape}")
    reg = np.zeros(B)
    cum = np.zeros(B) if return_all else None
    comp = np.zeros(B) if return_all else None
    xl = np.zeros((B, d)) if return_all else None
    _lib.call("ocx_simulate_alg_batch", ptr(z), ptr(y), B, T, d, int(alg_flag), float(eta0),
              ptr(cmp), ptr(reg), ptr(cum), ptr(comp), ptr(xl), int(lanes_per_seq), int(device))
    if return_all:
        return reg, cum, comp, xl
    return reg


def _checkpoints(checkpoints, T: int) -> np.ndarray:
    """The checkpoint horizons of a regret curve as a contiguous int64 array: integers,
    strictly increasing, inside [0, T] (0 and T allowed).  Raises ValueError otherwise."""
    a = np.asarray(checkpoints)
    if a.ndim != 1:
        raise ValueError(f"checkpoints must be one-dimensional, got shape {a.shape}")
    if a.size and not (np.issubdtype(a.dtype, np.integer) or np.all(a == np.floor(a))):
        raise ValueError("checkpoints must be integers")
    ck = np.ascontiguousarray(a, dtype=np.int64)
    if ck.size and (ck.min() < 0 or ck.max() > int(T)):
        raise ValueError(f"checkpoints must lie in [0, T = {int(T)}], got {ck.min()}..{ck.max()}")
    if np.any(np.diff(ck) <= 0):
        raise ValueError("checkpoints must be strictly increasing")
    return ck


def simulate_alg_curve_batch(z, y, checkpoints, alg_flag: int = 0, eta0: float = SQRT2, *,
                             lanes_per_seq: int = LANES_BEST, device: int = 0,
                             return_all: bool = False):
    """Regret curves: fast_algorithms.py:88-115 over B sequences, observed at every horizon of
    ``checkpoints`` (strictly increasing in [0, T]) in one pass (ocx_simulate_alg_curve_batch).

    Column k is simulate_alg on (z[b, :t_k], y[b, :t_k]).  Bit-exact modes (lanes_per_seq 1 /
    -k) stream the reference's comparator sum for every pair; the others take the closed form
    where the kernel certifies the prefix.  Returns regret [B, K] or, with ``return_all``,
    (regret, cum_loss, comp_loss, closed) — closed [B, K] int32, 1 where the closed form was
    taken."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _checkpoints(checkpoints, T)
    K = int(ck.size)
    reg = np.zeros((B, K))
    cum = np.zeros((B, K)) if return_all else None
    comp = np.zeros((B, K)) if return_all else None
    closed = np.zeros((B, K), dtype=np.int32) if return_all else None
    _lib.call("ocx_simulate_alg_curve_batch", ptr(z), ptr(y), B, T, d, int(alg_flag), float(eta0),
              ck.ctypes.data_as(_lib.c_i64p), K, ptr(reg), ptr(cum), ptr(comp),
              closed.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if return_all else None,
              int(lanes_per_seq), int(device))
    if return_all:
        return reg, cum, comp, closed
    return reg


def _anytime_checkpoints(checkpoints, T: int) -> np.ndarray:
    """The checkpoint horizons of an anytime regret: _checkpoints' rules inside [1, T] (a
    prefix has at least one step); None: [T], or the empty list at T = 0."""
    T = int(T)
    if checkpoints is None:
        checkpoints = [T] if T > 0 else []
    ck = _checkpoints(checkpoints, T)
    if ck.size and ck.min() < 1:
        raise ValueError(f"anytime checkpoints must lie in [1, T = {T}], got {ck.min()}")
    return ck


def _anytime_fold(torch, reg, lo: int, open_from, ck: np.ndarray, sup, argsup, run_best, run_arg,
                  trace=None):
    """One chunk of simulate_alg_anytime's completion.  reg [B, n]: the curve's regret at the
    horizons lo … lo + n - 1; open_from [B]; sup / argsup [B, K] at the horizons ck (host);
    run_best / run_arg [B]: the running max and its first argmax over the horizons before lo
    (of the sequences that are open by then; the others' never get out).  Only the open
    entries (t >= open_from[b]) are folded in, a later t only where strictly greater; the
    columns of the checkpoints inside the chunk, the open trace entries and the returned
    running pair are updated.  Tensors on one device, which need not be a GPU."""
    n = int(reg.shape[1])
    dev = reg.device
    ts = torch.arange(lo, lo + n, dtype=torch.int64, device=dev)
    is_open = ts[None, :] >= open_from[:, None]
    if trace is not None:
        trace[:, lo - 1:lo - 1 + n] = torch.where(is_open, reg, trace[:, lo - 1:lo - 1 + n])
    vals = torch.where(is_open, reg, torch.full_like(reg, -math.inf))
    cm = torch.maximum(torch.cummax(vals, dim=1).values, run_best[:, None])
    prev = torch.cat([run_best[:, None], cm[:, :-1]], dim=1)
    # the horizons that set a new record; the latest of them so far is the first argmax
    rec = torch.where(vals > prev, ts[None, :].expand_as(vals),
                      torch.zeros_like(vals, dtype=torch.int64))
    am = torch.maximum(torch.cummax(rec, dim=1).values, run_arg[:, None])
    ks = np.nonzero((ck >= lo) & (ck < lo + n))[0]
    if ks.size:
        kd = torch.as_tensor(ks).to(dev)
        col = torch.as_tensor(ck[ks] - lo).to(dev)
        upd = open_from[:, None] <= torch.as_tensor(ck[ks]).to(dev)[None, :]
        sup[:, kd] = torch.where(upd, cm[:, col], sup[:, kd])
        argsup[:, kd] = torch.where(upd, am[:, col], argsup[:, kd])
    return cm[:, -1].clone(), am[:, -1].clone()


def simulate_alg_anytime_batch(z, y, checkpoints=None, alg_flag: int = 0, eta0: float = SQRT2, *,
                               lanes_per_seq: int = LANES_BEST, device: int = 0,
                               return_trace: bool = False):
    """Anytime regret of B host sequences (DeviceBatch.simulate_alg_anytime on a packed
    batch): a dict of numpy arrays ``sup`` [B, K] (max over t <= t_k of the regret of
    simulate_alg on (z[b, :t], y[b, :t])), ``argsup`` [B, K] int64 (the smallest such t),
    ``open_from`` [B] int64 and, with ``return_trace``, ``trace`` [B, T] (the regret of every
    prefix).  ``checkpoints`` defaults to [T].

    Bit-exact layouts (lanes_per_seq 1 / -k) take ``closed_comparator=False``, as
    simulate_alg_curve_batch does: every prefix streams the reference's comparator sum,
    O(T²) rows per sequence.  The other layouts take the closed form in one pass wherever the
    kernel certifies the prefix and complete the rest from the curve."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _anytime_checkpoints(checkpoints, T)
    K = int(ck.size)
    if B == 0 or T == 0 or (K == 0 and not return_trace):  # nothing to compute: no device
        out = {"sup": np.full((B, K), -np.inf), "argsup": np.zeros((B, K), dtype=np.int64),
               "open_from": np.full((B,), T + 1, dtype=np.int64)}
        if return_trace:
            out["trace"] = np.zeros((B, T))
        return out
    db = DeviceBatch(B, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
    db.pack(z, y)
    res = db.simulate_alg_anytime(ck, alg_flag, eta0, trace=return_trace)
    with db._on_stream():
        return {k: v.cpu().numpy() for k, v in res.items()}


def _etas(etas) -> np.ndarray:
    """The step sizes of a sweep as a contiguous float64 array: a one-dimensional list of real
    numbers (any values, any order, duplicates allowed).  Raises ValueError otherwise."""
    try:
        a = np.asarray(etas)
    except Exception as e:  # ragged lists
        raise ValueError(f"etas must be a one-dimensional list of real numbers: {e}") from None
    if a.ndim != 1:
        raise ValueError(f"etas must be one-dimensional, got shape {a.shape}")
    if a.size and not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"etas must be real numbers, got dtype {a.dtype}")
    return np.ascontiguousarray(a, dtype=np.float64)


def simulate_alg_etas_batch(z, y, etas, *, lanes_per_seq: int = LANES_BEST, device: int = 0,
                            return_all: bool = False):
    """Step-size sweep: FTRL (fast_algorithms.py:88-115) over B sequences for every eta0 of
    ``etas``, each pass over z serving a group of them (ocx_simulate_alg_etas_batch).

    Column m is simulate_alg with eta0 = etas[m], bit for bit in the same layout.  Bit-exact
    modes (lanes_per_seq 1 / -k) stream the reference's comparator sum for every pair; the
    others take the closed form where the kernel certifies the (sequence, eta) pair.  Returns
    regret [B, M] or, with ``return_all``, (regret, cum_loss, comp_loss, closed) — closed
    [B, M] int32, 1 where the closed form was taken."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    et = _etas(etas)
    M = int(et.size)
    reg = np.zeros((B, M))
    cum = np.zeros((B, M)) if return_all else None
    comp = np.zeros((B, M)) if return_all else None
    closed = np.zeros((B, M), dtype=np.int32) if return_all else None
    _lib.call("ocx_simulate_alg_etas_batch", ptr(z), ptr(y), B, T, d, ptr(et), M, ptr(reg),
              ptr(cum), ptr(comp),
              closed.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if return_all else None,
              int(lanes_per_seq), int(device))
    if return_all:
        return reg, cum, comp, closed
    return reg


def simulate_alg_curve_etas_batch(z, y, checkpoints, etas, *, lanes_per_seq: int = LANES_BEST,
                                  device: int = 0, return_all: bool = False):
    """Regret grid: FTRL (fast_algorithms.py:88-115) over B sequences for every eta0 of
    ``etas``, observed at every horizon of ``checkpoints`` (strictly increasing in [0, T]),
    each pass over z serving a group of step sizes (ocx_simulate_alg_curve_etas_batch).

    Element (b, m, k) is simulate_alg with eta0 = etas[m] on (z[b, :t_k], y[b, :t_k]), bit for
    bit in the same layout: [:, m, :] is simulate_alg_curve_batch with etas[m], and with
    t_K = T, [:, :, -1] is simulate_alg_etas_batch.  Bit-exact modes (lanes_per_seq 1 / -k)
    stream the reference's comparator sum for every triple; the others take the closed form
    where the kernel certifies the (sequence, eta, prefix) triple.  Returns regret [B, M, K]
    or, with ``return_all``, (regret, cum_loss, comp_loss, closed) — closed [B, M, K] int32, 1
    where the closed form was taken."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _checkpoints(checkpoints, T)
    et = _etas(etas)
    K, M = int(ck.size), int(et.size)
    reg = np.zeros((B, M, K))
    cum = np.zeros((B, M, K)) if return_all else None
    comp = np.zeros((B, M, K)) if return_all else None
    closed = np.zeros((B, M, K), dtype=np.int32) if return_all else None
    _lib.call("ocx_simulate_alg_curve_etas_batch", ptr(z), ptr(y), B, T, d, ptr(et), M,
              ck.ctypes.data_as(_lib.c_i64p), K, ptr(reg), ptr(cum), ptr(comp),
              closed.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if return_all else None,
              int(lanes_per_seq), int(device))
    if return_all:
        return reg, cum, comp, closed
    return reg


def simulate_smart_batch(z, y, thresh, eta0: float = SQRT2, *, lanes_per_seq: int = LANES_BEST,
                         device: int = 0, return_switch: bool = False):
    """fast_algorithms.py:118-164 over B sequences; thresh scalar or [B].  Bit-exact modes
    (lanes_per_seq 1 / -k) run the reference's O(T²·d) prefix re-scan; the others the
    O(T·d) kernel (guarded closed-form prefix: the same switch steps; closed-form final
    comparator where certified: the regret within its rounding)."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    th = _f64(np.broadcast_to(np.asarray(thresh, dtype=np.float64), (B,)))
    reg = np.zeros(B)
    sw = np.zeros(B, dtype=np.int64)
    _lib.call("ocx_simulate_smart_batch", ptr(z), ptr(y), B, T, d, ptr(th), float(eta0), ptr(reg),
              sw.ctypes.data_as(_lib.c_i64p), int(lanes_per_seq), int(device))
    return (reg, sw) if return_switch else reg


def _thresholds(thresholds, B: int) -> np.ndarray:
    """The switch thresholds of a sweep as a contiguous float64 array [B, M]: real numbers,
    ``[M]`` (every sequence the same) or ``[B, M]`` (per sequence); any values (NaN and ±inf
    included), any order, duplicates allowed.  Raises ValueError otherwise."""
    try:
        a = np.asarray(thresholds)
    except Exception as e:  # ragged lists
        raise ValueError(f"thresholds must be [M] or [B, M] real numbers: {e}") from None
    if a.ndim not in (1, 2):
        raise ValueError(f"thresholds must be [M] or [B, M], got shape {a.shape}")
    if a.size and not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"thresholds must be real numbers, got dtype {a.dtype}")
    if a.ndim == 2 and a.shape[0] != B:
        raise ValueError(f"per-sequence thresholds must be [B = {B}, M], got shape {a.shape}")
    return np.array(np.broadcast_to(a, (B, a.shape[-1])), dtype=np.float64, order="C")


def simulate_smart_thresholds_batch(z, y, thresholds, eta0: float = SQRT2, *,
                                    lanes_per_seq: int = LANES_BEST, device: int = 0,
                                    return_switch: bool = False):
    """Threshold sweep: SMART (fast_algorithms.py:118-164) over B sequences for every switch
    threshold of ``thresholds`` ([M], or [B, M] per sequence), each pass over z serving a
    group of them (ocx_simulate_smart_thresholds_batch): one FTL trajectory, one prefix test
    and one comparator per pass, a switch step and an FTRL state per column.

    Column m is simulate_smart_batch with thresh = thresholds[..., m]: in the bit-exact modes
    (lanes_per_seq 1 / -k) the reference's prefix re-scan and streamed comparator, bit for
    bit — run by the one-wave-per-sequence kernel (ocx_smart_wave_cols.hip, one re-scan per
    step for up to eight columns) at d <= 64 and B <= 32768, by the lane-group kernel
    elsewhere or under ``OCX_SMART_KERNEL=lanes``; in the other modes the lane-group kernel
    with both closed forms.  ``thresh = +inf`` makes a
    column FTL's regret, with the same adds and the same comparator; ``sqrt(2T)`` and the
    empirical g(T) are the drivers' SMART and EMP.  Returns regret [B, M] or, with
    ``return_switch``, (regret, switch_step [B, M] int64, -1 = never)."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    th = _thresholds(thresholds, B)
    M = int(th.shape[1])
    reg = np.zeros((B, M))
    sw = np.full((B, M), -1, dtype=np.int64)
    _lib.call("ocx_simulate_smart_thresholds_batch", ptr(z), ptr(y), B, T, d, ptr(th), M,
              float(eta0), ptr(reg), sw.ctypes.data_as(_lib.c_i64p), int(lanes_per_seq),
              int(device))
    return (reg, sw) if return_switch else reg


def _horizons(horizons, T: int) -> np.ndarray:
    """The horizons of a SMART regret curve as a contiguous int64 array: a one-dimensional
    list of integers, non-decreasing (equal horizons are legal: SMART and EMP at the same
    t_k), inside [0, T].  Booleans and non-integral floats are rejected.  Raises ValueError
    otherwise."""
    try:
        a = np.asarray(horizons)
    except Exception as e:  # ragged lists
        raise ValueError(f"horizons must be a one-dimensional list of integers: {e}") from None
    if a.ndim != 1:
        raise ValueError(f"horizons must be one-dimensional, got shape {a.shape}")
    if a.size and not (np.issubdtype(a.dtype, np.integer) or
                       (np.issubdtype(a.dtype, np.floating) and np.all(np.isfinite(a)) and
                        np.all(a == np.floor(a)))):
        raise ValueError(f"horizons must be integers, got dtype {a.dtype}")
    hz = np.ascontiguousarray(a, dtype=np.int64)
    if hz.size and (hz.min() < 0 or hz.max() > int(T)):
        raise ValueError(f"horizons must lie in [0, T = {int(T)}], got {hz.min()}..{hz.max()}")
    if np.any(np.diff(hz) < 0):
        raise ValueError("horizons must be non-decreasing")
    return hz


def _smart_curve_thresholds(thresholds, hz: np.ndarray, B: int) -> np.ndarray:
    """[B, K] thresholds of a SMART curve: ``thresholds`` through _thresholds, or SMART's own
    sqrt(2 t_k) when None; one column per horizon."""
    if thresholds is None:
        thresholds = np.sqrt(2.0 * hz.astype(np.float64))
    th = _thresholds(thresholds, B)
    if th.shape[1] != hz.size:
        raise ValueError(f"need one threshold column per horizon: {hz.size} horizons, "
                         f"{th.shape[1]} threshold columns")
    return th


def simulate_smart_curve_batch(z, y, horizons, thresholds=None, eta0: float = SQRT2, *,
                               lanes_per_seq: int = LANES_BEST, device: int = 0,
                               return_switch: bool = False):
    """SMART regret curves: SMART (fast_algorithms.py:118-164) over B sequences for K pairs
    (horizon t_k, threshold), each pass over z serving a group of consecutive pairs and
    stopping at the group's last horizon (ocx_simulate_smart_curve_batch).

    ``horizons`` [K]: integers, non-decreasing in [0, T]; ``thresholds`` [K] or [B, K]
    (None: SMART's own sqrt(2 t_k)).  Column k is simulate_smart_batch on
    (z[:, :t_k], y[:, :t_k]) with thresh = thresholds[..., k]: bit for bit in the bit-exact
    modes (lanes_per_seq 1 / -k: the reference's prefix re-scan and streamed comparator; the
    one-wave-per-sequence kernel where simulate_smart_thresholds_batch says it runs), the
    lane-group kernel with both closed forms in the others.  Returns regret [B, K] or, with ``return_switch``, (regret,
    switch_step [B, K] int64, in [0, t_k) or -1 = never)."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    hz = _horizons(horizons, T)
    th = _smart_curve_thresholds(thresholds, hz, B)
    K = int(hz.size)
    reg = np.zeros((B, K))
    sw = np.full((B, K), -1, dtype=np.int64)
    _lib.call("ocx_simulate_smart_curve_batch", ptr(z), ptr(y), B, T, d,
              hz.ctypes.data_as(_lib.c_i64p), ptr(th), K, float(eta0), ptr(reg),
              sw.ctypes.data_as(_lib.c_i64p), int(lanes_per_seq), int(device))
    return (reg, sw) if return_switch else reg


def simulate_smart_grid_batch(z, y, checkpoints, thresholds, eta0: float = SQRT2, *,
                              lanes_per_seq: int = LANES_BEST, device: int = 0,
                              return_switch: bool = False):
    """SMART regret grid: SMART (fast_algorithms.py:118-164) over B sequences for every switch
    threshold of ``thresholds`` ([M], or [B, M] per sequence), observed at every horizon of
    ``checkpoints`` (strictly increasing in [0, T]); each pass over z serves a group of
    thresholds and runs once, to the last checkpoint (ocx_simulate_smart_grid_batch).

    Element (b, m, k) is simulate_smart_batch on (z[b, :t_k], y[b, :t_k]) with
    thresh = thresholds[..., m], bit for bit in the same layout: [:, m, :] is
    simulate_smart_curve_batch with that threshold at every checkpoint, and with t_K = T,
    [:, :, -1] is simulate_smart_thresholds_batch.  Bit-exact modes (lanes_per_seq 1 / -k): the
    reference's prefix re-scan and streamed comparator; the others: both closed forms.
    Returns regret [B, M, K] or, with ``return_switch``, (regret, switch_step [B, M, K] int64:
    the full run's switch step where it lies before t_k, else -1)."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _checkpoints(checkpoints, T)
    th = _thresholds(thresholds, B)
    K, M = int(ck.size), int(th.shape[1])
    reg = np.zeros((B, M, K))
    sw = np.full((B, M, K), -1, dtype=np.int64)
    _lib.call("ocx_simulate_smart_grid_batch", ptr(z), ptr(y), B, T, d, ptr(th), M,
              ck.ctypes.data_as(_lib.c_i64p), K, float(eta0), ptr(reg),
              sw.ctypes.data_as(_lib.c_i64p), int(lanes_per_seq), int(device))
    return (reg, sw) if return_switch else reg


def replay_batch(z, y, actions, *, device: int = 0):
    """exact_ftl.py:306-333 over B sequences: actions [B, T+1, d] → (cum_loss, comp_loss)."""
    z = _f64(z)
    y = _f64(y)
    a = _f64(actions)
    B, T, d = _check_zy(z, y)
    if a.shape != (B, T + 1, d):
        raise ValueError(f"actions must be [B, T+1, d] = {(B, T + 1, d)}, got {a.shape}")
    cum = np.zeros(B)
    comp = np.zeros(B)
    _lib.call("ocx_replay_batch", ptr(z), ptr(y), ptr(a), B, T, d, ptr(cum), ptr(comp),
              int(device))
    return cum, comp


NORMS = {"l2": 0, "l1": 1, "linf": 2}  # the ball of exact FTL (exact_ftl.py:83-105)


def _norm_code(norm: str) -> int:
    if norm not in NORMS:
        raise ValueError("norm must be one of {'l2','linf','l1'}")
    return NORMS[norm]


def exact_ball_solve(z, y, *, norm: str = "l2", all_prefixes: bool = True, device: int = 0):
    """The general exact-FTL solver (include/ocx.h, ocx_exact_ball_solve): ExactFTLNoClip's
    problem min ½Σ_{i<n}|z_i·x − y_i| over the unit ``norm`` ball (exact_ftl.py:83-105) for
    any rows and labels, on the GPU by a log-barrier path.  Problems are every prefix
    n = 0..T of each sequence (``all_prefixes``) or n = T only.

    Returns a dict of arrays over [B, NP] (NP = T+1 or 1): ``actions`` [B, NP, d]
    (actions[:, n] the prefix-n minimiser, as compute_prefix_actions returns), ``obj``
    (½Σ|r| at it), ``gap`` (a certified bound on obj − optimum), ``step_loss`` (½|z_n·x_n −
    y_n|, 0 at n = T) and ``info`` (Newton steps, negative where the cap ended a solve)."""
    code = _norm_code(norm)
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    if d > _lib.OCX_EXACT_BALL_MAX_D:
        raise NotImplementedError(f"the general exact-FTL solver takes d <= "
                                  f"{_lib.OCX_EXACT_BALL_MAX_D} (got {d})")
    NP = T + 1 if all_prefixes else 1
    out = {"actions": np.zeros((B, NP, d)), "obj": np.zeros((B, NP)), "gap": np.zeros((B, NP)),
           "step_loss": np.zeros((B, NP)), "info": np.zeros((B, NP), dtype=np.int32)}
    _lib.call("ocx_exact_ball_solve", ptr(z), ptr(y), B, T, d, code, int(bool(all_prefixes)),
              ptr(out["actions"]), ptr(out["obj"]), ptr(out["gap"]), ptr(out["step_loss"]),
              out["info"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(device))
    return out


# A general solve is accepted iff info >= 0 and gap <= EXACT_GAP_RTOL * (1 + |obj|).  The gap
# comes from the better of two duals: the barrier's multipliers (exact for the rows the optimum
# does not interpolate, only as good as μ_end = 1e-10 for the ones it does) and the dual the
# certificate polish rebuilds from the KKT system at the solver's x (ocx_exact_polish_kernel:
# ±½ on the first kind, least squares on stationarity for the second), which certifies the
# objective to the primal's own accuracy (~1e-10) where the optimum interpolates rows (n > d,
# real-valued rows: the barrier's certificate alone stayed near 1e-5 there).
EXACT_GAP_RTOL = 1e-8


def check_certificates(obj, gap, info, what: str = "exact FTL") -> float:
    """The general solver's answers are only as good as their certificates
    (include/ocx.h, ocx_exact_ball_solve): every solve must have finished (info >= 0: not
    ended by the step cap; 0 is the empty prefix, solved without a step) and certify obj − optimum <= gap <= EXACT_GAP_RTOL·(1 + |obj|).
    A breakdown stop (OCX_EXACT_INFO_BREAKDOWN) passes only on its certificate.  Raises
    RuntimeError otherwise — what exact_ftl.py:125-126 does when cvxpy's solve fails — and
    returns the worst gap."""
    obj = np.asarray(obj, dtype=np.float64)
    gap = np.asarray(gap, dtype=np.float64)
    info = np.asarray(info)
    if obj.size == 0:
        return 0.0
    bad = ~((info >= 0) & (gap <= EXACT_GAP_RTOL * (1.0 + np.abs(obj))))
    if bad.any():
        k = int(np.flatnonzero(bad.ravel())[0])
        raise RuntimeError(f"{what}: the general solver did not certify {int(bad.sum())} of "
                           f"{bad.size} problems (first: info {int(info.ravel()[k])}, gap "
                           f"{float(gap.ravel()[k]):.3g}, obj {float(obj.ravel()[k]):.6g})")
    return float(gap.max())


def _general_fill(z, y, ok: np.ndarray, norm: str, device: int):
    """Sequences outside the closed form's regime, solved by the general solver: (their
    indices, exact_ball_solve over all prefixes, exact FTL's cumulative loss Σ_n step_loss in
    step order, the comparator loss obj[:, T], the worst certified gap); None when every
    sequence is in the regime.  Raises RuntimeError where a solve is not certified."""
    bad = np.flatnonzero(~ok)
    if bad.size == 0:
        return None
    T = z.shape[1]
    res = exact_ball_solve(z[bad], y[bad], norm=norm, all_prefixes=True, device=device)
    worst = check_certificates(res["obj"], res["gap"], res["info"])
    sl = res["step_loss"][:, :T]
    cum = np.cumsum(sl, axis=1)[:, -1] if T > 0 else np.zeros(bad.size)  # sequential order
    return bad, res, cum, res["obj"][:, T], worst


def ftl_exact_batch(z, y, *, norm: str = "l2", lanes_per_seq: int = LANES_BEST, device: int = 0,
                    check_regime: bool = True):
    """exact_ftl.py:280-333 (compute_prefix_actions + replay) for B sequences on the GPU,
    over the unit ball of ``norm`` ('l2', 'l1', 'linf'), in the closed form that is the
    exact SOCP / LP solution when every row's dual norm is <= 1 and y_t = ±1
    (include/ocx.h, ocx_ftl_exact_batch).

    Returns (cum_loss [B], comp_loss [B], comparator actions[T] [B, d], in_regime [B]);
    with ``check_regime`` the sequences outside the regime are solved by the general solver
    (exact_ball_solve, d <= 256) — their numbers are the SOCP / LP's; without it they keep the
    closed form's (not the solution there: callers must reject them)."""
    code = _norm_code(norm)
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    cum = np.zeros(B)
    comp = np.zeros(B)
    act = np.zeros((B, d))
    rg = np.zeros(B, dtype=np.int32)
    _lib.call("ocx_ftl_exact_batch", ptr(z), ptr(y), B, T, d, code, ptr(cum), ptr(comp),
              ptr(act), rg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(lanes_per_seq),
              int(device))
    ok = rg.astype(bool)
    if check_regime:
        g = _general_fill(z, y, ok, norm, device)
        if g is not None:
            bad, res, gcum, gcomp, _ = g
            cum[bad], comp[bad], act[bad] = gcum, gcomp, res["actions"][:, T]
    return cum, comp, act, ok


def ftl_prefix_actions_batch(z, y, *, norm: str = "l2", lanes_per_seq: int = LANES_BEST, device: int = 0,
                             check_regime: bool = True):
    """exact_ftl.py:280-303 compute_prefix_actions for B sequences on the GPU
    (include/ocx.h, ocx_ftl_prefix_actions_batch): actions [B, T+1, d] with actions[:, t]
    the exact FTL solution of the first t rows, in the closed form of ftl_exact_batch.

    Returns (actions, in_regime [B]); with ``check_regime`` the sequences outside the regime
    get the general solver's actions (exact_ball_solve)."""
    code = _norm_code(norm)
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    act = np.zeros((B, T + 1, d))
    rg = np.zeros(B, dtype=np.int32)
    _lib.call("ocx_ftl_prefix_actions_batch", ptr(z), ptr(y), B, T, d, code, ptr(act),
              rg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(lanes_per_seq), int(device))
    ok = rg.astype(bool)
    if check_regime:
        g = _general_fill(z, y, ok, norm, device)
        if g is not None:
            act[g[0]] = g[1]["actions"]
    return act, ok


def ftrl_vs_exact_batch(z, y, eta0: float = SQRT2, *, norm: str = "l2",
                        lanes_per_seq: int = LANES_BEST, device: int = 0,
                        check_regime: bool = True, with_ftl_comparator: bool = False):
    """exact_ftl_driver.py:157-186 for B sequences in one read of the data: exact FTL
    (closed form, as ftl_exact_batch) and FTRL against its comparator actions[T].

    Returns a dict of [B] arrays: ``ftrl`` and ``exact`` regrets, ``cum_ftrl``,
    ``cum_exact``, ``comp`` (the loss of actions[T], shared by both), ``action``
    [B, d], ``in_regime``; with ``with_ftl_comparator`` also ``comp_ftl``, the loss of
    FTL(theta_ftrl) (the comparator simulate_alg itself uses).  With ``check_regime`` the
    exact side of sequences outside the closed form's regime comes from the general solver
    (exact_ball_solve), as in ftl_exact_batch."""
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    cr, ce, cmp_e, cmp_f = (np.zeros(B) for _ in range(4))
    act = np.zeros((B, d))
    rg = np.zeros(B, dtype=np.int32)
    _lib.call("ocx_ftrl_vs_exact_batch_ex", ptr(z), ptr(y), B, T, d, float(eta0), ptr(cr), ptr(ce),
              ptr(cmp_e), ptr(cmp_f) if with_ftl_comparator else None, ptr(act),
              rg.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _norm_code(norm),
              int(lanes_per_seq), int(device))
    ok = rg.astype(bool)
    worst = 0.0
    if check_regime:
        g = _general_fill(z, y, ok, norm, device)
        if g is not None:
            bad, res, gcum, gcomp, worst = g
            ce[bad], cmp_e[bad], act[bad] = gcum, gcomp, res["actions"][:, T]
    out = {"ftrl": cr - cmp_e, "exact": ce - cmp_e, "cum_ftrl": cr, "cum_exact": ce,
           "comp": cmp_e, "action": act, "in_regime": ok, "exact_gap_max": worst}
    if with_ftl_comparator:
        out["comp_ftl"] = cmp_f
    return out


def _general_curve_columns(step_loss, obj, ck: np.ndarray):
    """The general solver's columns of an exact curve from its all-prefix results (step_loss,
    obj [n, Tm + 1]): exact FTL's cumulative loss in step order at every horizon of ``ck``
    (cumsum(step_loss)[t_k - 1], 0 at t_k = 0) and the comparator loss obj[:, t_k]."""
    n = step_loss.shape[0]
    run = np.concatenate([np.zeros((n, 1)), np.cumsum(step_loss[:, :-1], axis=1)], axis=1)
    return run[:, ck], obj[:, ck]


def ftrl_vs_exact_curve_batch(z, y, checkpoints, eta0: float = SQRT2, *, norm: str = "l2",
                              lanes_per_seq: int = LANES_BEST, device: int = 0,
                              check_regime: bool = True, with_ftl_comparator: bool = False):
    """FTRL-vs-exact-FTL regret curves (exact_ftl_driver.py:157-190 against the horizon) for B
    sequences in one pass (ocx_ftrl_vs_exact_curve_batch): ftrl_vs_exact_batch observed at
    every horizon of ``checkpoints`` (strictly increasing in [0, T]).

    Returns a dict of [B, K] arrays ``ftrl``, ``exact``, ``cum_ftrl``, ``cum_exact``, ``comp``,
    ``in_regime`` (bool), ``closed`` (int32), ``action`` [B, K, d], ``exact_gap_max`` and, with
    ``with_ftl_comparator``, ``comp_ftl``; column k is ftrl_vs_exact_batch on (z[:, :t_k],
    y[:, :t_k]) with the same arguments.  With ``check_regime`` the pairs outside the closed
    form's regime are filled by ONE general solve (exact_ball_solve over all prefixes up to the
    largest checkpoint) of the sequences that have such a pair; the other pairs keep the
    closed form."""
    code = _norm_code(norm)
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _checkpoints(checkpoints, T)
    K = int(ck.size)
    cr, ce, cmp_e, cmp_f = (np.zeros((B, K)) for _ in range(4))
    act = np.zeros((B, K, d))
    rg = np.zeros((B, K), dtype=np.int32)
    closed = np.zeros((B, K), dtype=np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    _lib.call("ocx_ftrl_vs_exact_curve_batch", ptr(z), ptr(y), B, T, d, float(eta0),
              ck.ctypes.data_as(_lib.c_i64p), K, ptr(cr), ptr(ce), ptr(cmp_e),
              ptr(cmp_f) if with_ftl_comparator else None, ptr(act), rg.ctypes.data_as(i32p),
              closed.ctypes.data_as(i32p), code, int(lanes_per_seq), int(device))
    ok = rg.astype(bool)
    worst = 0.0
    bad = np.flatnonzero((~ok).any(axis=1)) if K else np.zeros(0, dtype=np.int64)
    if check_regime and bad.size:
        Tm = int(ck[-1])
        res = exact_ball_solve(z[bad, :Tm], y[bad, :Tm], norm=norm, all_prefixes=True,
                               device=device)
        worst = check_certificates(res["obj"], res["gap"], res["info"])
        gcum, gcomp = _general_curve_columns(res["step_loss"], res["obj"], ck)
        m = ~ok[bad]                                   # only these pairs change
        ce[bad] = np.where(m, gcum, ce[bad])
        cmp_e[bad] = np.where(m, gcomp, cmp_e[bad])
        act[bad] = np.where(m[:, :, None], res["actions"][:, ck], act[bad])
    out = {"ftrl": cr - cmp_e, "exact": ce - cmp_e, "cum_ftrl": cr, "cum_exact": ce,
           "comp": cmp_e, "action": act, "in_regime": ok, "closed": closed,
           "exact_gap_max": worst}
    if with_ftl_comparator:
        out["comp_ftl"] = cmp_f
    return out


def ftrl_vs_exact_curve_etas_batch(z, y, checkpoints, etas, *, norm: str = "l2",
                                   lanes_per_seq: int = LANES_BEST, device: int = 0,
                                   check_regime: bool = True, with_ftl_comparator: bool = False):
    """FTRL-vs-exact-FTL regret grid for B sequences (ocx_ftrl_vs_exact_curve_etas_batch):
    ftrl_vs_exact_curve_batch for every eta0 of ``etas`` (a one-dimensional list of reals, any
    order, duplicates allowed), each pass over z serving a group of FTRL columns beside one
    exact-FTL column.

    Returns a dict: ``ftrl``, ``cum_ftrl`` (and ``comp_ftl``) [B, M, K]; ``exact``,
    ``cum_exact``, ``comp``, ``in_regime`` (bool), ``closed`` (int32) [B, K], ``action``
    [B, K, d] and ``exact_gap_max``, which do not depend on the step size.  [:, m, :] and the
    [B, K] arrays are ftrl_vs_exact_curve_batch(z, y, checkpoints, etas[m]) with the same
    arguments.  With ``check_regime`` the pairs outside the closed form's regime are filled by
    ONE general solve, whatever M is."""
    code = _norm_code(norm)
    z = _f64(z)
    y = _f64(y)
    B, T, d = _check_zy(z, y)
    ck = _checkpoints(checkpoints, T)
    et = _etas(etas)
    K, M = int(ck.size), int(et.size)
    cr, cmp_f = np.zeros((B, M, K)), np.zeros((B, M, K))
    ce, cmp_e = np.zeros((B, K)), np.zeros((B, K))
    act = np.zeros((B, K, d))
    rg = np.zeros((B, K), dtype=np.int32)
    closed = np.zeros((B, K), dtype=np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    _lib.call("ocx_ftrl_vs_exact_curve_etas_batch", ptr(z), ptr(y), B, T, d, ptr(et), M,
              ck.ctypes.data_as(_lib.c_i64p), K, ptr(cr), ptr(ce), ptr(cmp_e),
              ptr(cmp_f) if with_ftl_comparator else None, ptr(act), rg.ctypes.data_as(i32p),
              closed.ctypes.data_as(i32p), code, int(lanes_per_seq), int(device))
    ok = rg.astype(bool)
    worst = 0.0
    bad = np.flatnonzero((~ok).any(axis=1)) if K and M else np.zeros(0, dtype=np.int64)
    if check_regime and bad.size:
        Tm = int(ck[-1])
        res = exact_ball_solve(z[bad, :Tm], y[bad, :Tm], norm=norm, all_prefixes=True,
                               device=device)
        worst = check_certificates(res["obj"], res["gap"], res["info"])
        gcum, gcomp = _general_curve_columns(res["step_loss"], res["obj"], ck)
        m = ~ok[bad]                                   # only these pairs change
        ce[bad] = np.where(m, gcum, ce[bad])
        cmp_e[bad] = np.where(m, gcomp, cmp_e[bad])
        act[bad] = np.where(m[:, :, None], res["actions"][:, ck], act[bad])
    out = {"ftrl": cr - cmp_e[:, None, :], "exact": ce - cmp_e, "cum_ftrl": cr, "cum_exact": ce,
           "comp": cmp_e, "action": act, "in_regime": ok, "closed": closed,
           "exact_gap_max": worst}
    if with_ftl_comparator:
        out["comp_ftl"] = cmp_f
    return out


def gT_regrets(T: int, runs: int, *, base_seed: int = 0, d: int = 5, eta0: float = SQRT2,
               run0: int = 0, lanes_per_seq: int = LANES_BEST, device: int = 0) -> np.ndarray:
    """Regrets of FTRL on _rng(base_seed, T, run) sequences, run in [run0, run0+runs),
    generated on device (fast_algorithms.py:230-241 with a ``d`` parameter)."""
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    out = np.zeros(int(runs))
    _lib.call("ocx_gT_regrets", int(base_seed), int(T), int(run0), int(runs), int(d),
              float(eta0), ptr(out), int(lanes_per_seq), int(device))
    return out


def gT_regrets_device(T: int, runs: int, *, base_seed: int = 0, d: int = 5,
                      eta0: float = SQRT2, run0: int = 0, lanes_per_seq: int = LANES_BEST,
                      device: int = 0, out=None):
    """gT_regrets with the regrets left in HBM (``ocx_gT_regrets_dev``): a float64 torch
    tensor [runs] on cuda:``device`` (``out`` if given), complete when this returns.  What a
    rank hands to an RCCL all-gather (parallel.gT_sweep_distributed): no host round trip."""
    import torch
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    dev = torch.device("cuda", int(device))
    if out is None:
        out = torch.empty(int(runs), dtype=torch.float64, device=dev)
    if out.dtype != torch.float64 or out.device != dev or not out.is_contiguous() \
            or out.numel() != int(runs):
        raise ValueError(f"out must be a contiguous float64 tensor of {runs} on {dev}")
    # the library writes on its own stream: let the allocating stream's pending work on
    # this memory finish first
    torch.cuda.current_stream(dev).synchronize()
    _lib.call("ocx_gT_regrets_dev", int(base_seed), int(T), int(run0), int(runs), int(d),
              float(eta0), ctypes.c_void_p(out.data_ptr()), int(lanes_per_seq), int(device))
    return out


TWIN32_ALGOS = {"FTRL": 0, "FTL": 1, "SMART": 2}


def twin32_batch(z, y, algo: int = 0, eta0: float = SQRT2, thresh=None, *, device: int = 0,
                 return_all: bool = False):
    """The float32 twin (algorithms.py:28-54 simulate_alg, algo 0 FTRL / 1 FTL; :65-120
    simulate_SMART_like, algo 2 with thresh scalar or [B]) over B sequences, in NumPy 2's
    float32 arithmetic; d <= 32.

    z [B, T, d] and y [B, T] are taken as float32 (the twin's callers pass float32).
    Returns the twin's np.float32 results [B] or, with ``return_all``, (result, cum_loss
    float64, comp_loss float32, switch_step int64; -1 = no switch / not SMART)."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    B, T, d = _check_zy(z, y)
    algo = int(algo)
    if algo not in (0, 1, 2):
        raise ValueError("algo must be 0 (FTRL), 1 (FTL) or 2 (SMART)")
    th = None
    if algo == 2:
        if thresh is None:
            raise ValueError("SMART needs thresh")
        th = _f64(np.broadcast_to(np.asarray(thresh, dtype=np.float64), (B,)))
    res = np.zeros(B, dtype=np.float32)
    cum = np.zeros(B) if return_all else None
    comp = np.zeros(B, dtype=np.float32) if return_all else None
    sw = np.full(B, -1, dtype=np.int64) if return_all else None
    fp = _lib.c_fp
    _lib.call("ocx_twin32_batch", z.ctypes.data_as(fp), y.ctypes.data_as(fp), B, T, d, algo,
              float(eta0), ptr(th), res.ctypes.data_as(fp), ptr(cum),
              comp.ctypes.data_as(fp) if comp is not None else None,
              sw.ctypes.data_as(_lib.c_i64p) if sw is not None else None, int(device))
    return (res, cum, comp, sw) if return_all else res


def _twin32_algos(algos, K: int) -> np.ndarray:
    """The algorithms of a twin column call as a contiguous int32 array [K]: a scalar (every
    column the same) or a length-K list of 0 / 1 / 2 or the names of TWIN32_ALGOS.  Booleans,
    other numbers and other names are rejected.  Raises ValueError otherwise."""
    if isinstance(algos, (str, bytes)) or np.ndim(algos) == 0:
        algos = [algos] * K
    try:
        items = list(algos)
    except TypeError:
        raise ValueError("algos must be a scalar or a one-dimensional list") from None
    if len(items) != K:
        raise ValueError(f"need one algorithm per horizon: {K} horizons, {len(items)} algorithms")
    out = np.zeros(K, dtype=np.int32)
    for k, a in enumerate(items):
        if isinstance(a, str):
            if a not in TWIN32_ALGOS:
                raise ValueError(f"algos[{k}] = {a!r}: must be one of {sorted(TWIN32_ALGOS)}")
            out[k] = TWIN32_ALGOS[a]
        elif isinstance(a, (int, np.integer)) and not isinstance(a, (bool, np.bool_)) \
                and int(a) in (0, 1, 2):
            out[k] = int(a)
        else:
            raise ValueError(f"algos[{k}] = {a!r}: must be 0 (FTRL), 1 (FTL), 2 (SMART) or a "
                             f"name of {sorted(TWIN32_ALGOS)}")
    return out


def _twin32_cols_thresholds(thresholds, hz: np.ndarray, al: np.ndarray, B: int):
    """[B, K] float64 thresholds of a twin column call, or None when no column is SMART.
    ``thresholds`` None: SMART's own sqrt(2 t_k) in the SMART columns.  Otherwise [K] or [B, K]
    through _thresholds, one column per horizon; the entries of FTRL / FTL columns are ignored
    (NaN is the natural filler), a NaN in a SMART column is a missing threshold: ValueError."""
    smart = al == 2
    if thresholds is None:
        if not smart.any():
            return None
        thresholds = np.where(smart, np.sqrt(2.0 * hz.astype(np.float64)), 0.0)
    th = _thresholds(thresholds, B)
    if th.shape[1] != hz.size:
        raise ValueError(f"need one threshold column per horizon: {hz.size} horizons, "
                         f"{th.shape[1]} threshold columns")
    if np.isnan(th[:, smart]).any():
        raise ValueError("a SMART column needs a threshold: NaN in columns "
                         f"{np.flatnonzero(smart & np.isnan(th).any(axis=0)).tolist()}")
    th[:, ~smart] = 0.0
    return th if smart.any() else None


def _twin32_cols_call(call, name: str, *args) -> None:
    """A twin column call; OCX_E_UNSUPPORTED (a horizon whose rows do not fit the LDS: the
    library's message names the limit for that d) surfaces as NotImplementedError."""
    try:
        call(name, *args)
    except _lib.OCXError as e:
        if ": unsupported: " in str(e):
            raise NotImplementedError(str(e)) from None
        raise


def twin32_cols_batch(z, y, horizons, algos=2, thresholds=None, eta0: float = SQRT2, *,
                      device: int = 0, return_all: bool = False):
    """Twin sweeps: the float32 twin (twin32_batch) over B sequences for K columns (horizon
    t_k, algorithm, threshold) from one staging of the rows and one prefix re-scan per step
    (ocx_twin32_cols_batch; csrc/ocx_twin32_cols.hip).

    ``horizons`` [K]: integers, non-decreasing in [0, T], duplicates legal (FTRL, FTL, SMART
    and EMP at the same t_k).  ``algos``: a scalar or a length-K list of 0 / 1 / 2 or "FTRL" /
    "FTL" / "SMART" (TWIN32_ALGOS).  ``thresholds``: None (sqrt(2 t_k) in the SMART columns),
    [K] or [B, K]; the entries of FTRL / FTL columns are ignored, NaN in a SMART column is an
    error.  Column k is twin32_batch(z[:, :t_k], y[:, :t_k], algos[k], eta0,
    thresh=thresholds[..., k]) bit for bit.  The rows of the last horizon must fit the LDS
    (2194 rows at d = 5): NotImplementedError otherwise.  Returns float32 results [B, K] or,
    with ``return_all``, (result, cum_loss float64, comp_loss float32, switch_step int64; -1 =
    no switch / not SMART), each [B, K]."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    B, T, d = _check_zy(z, y)
    hz = _horizons(horizons, T)
    K = int(hz.size)
    al = _twin32_algos(algos, K)
    th = _twin32_cols_thresholds(thresholds, hz, al, B)
    res = np.zeros((B, K), dtype=np.float32)
    cum = np.zeros((B, K)) if return_all else None
    comp = np.zeros((B, K), dtype=np.float32) if return_all else None
    sw = np.full((B, K), -1, dtype=np.int64) if return_all else None
    fp = _lib.c_fp
    _twin32_cols_call(_lib.call, "ocx_twin32_cols_batch", z.ctypes.data_as(fp),
                      y.ctypes.data_as(fp), B, T, d, K, hz.ctypes.data_as(_lib.c_i64p),
                      al.ctypes.data_as(_lib.c_i32p), float(eta0), ptr(th),
                      res.ctypes.data_as(fp), ptr(cum),
                      comp.ctypes.data_as(fp) if comp is not None else None,
                      sw.ctypes.data_as(_lib.c_i64p) if sw is not None else None, int(device))
    return (res, cum, comp, sw) if return_all else res


def twin32_gT_regrets(T: int, runs: int, *, base_seed: int = 0, d: int = 5,
                      eta0: float = SQRT2, run0: int = 0, device: int = 0) -> np.ndarray:
    """The float32 twin's g(T) regrets (algorithms.py:150-169) for runs [run0, run0+runs),
    generated and simulated on device: float32 [runs]."""
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    out = np.zeros(int(runs), dtype=np.float32)
    _lib.call("ocx_twin32_gT_regrets", int(base_seed), int(T), int(run0), int(runs), int(d),
              float(eta0), out.ctypes.data_as(_lib.c_fp), int(device))
    return out


def release_buffers(device: int = 0) -> None:
    """Free the HBM the engine caches on `device` for host-array calls and g(T) sweeps
    (it regrows on the next call): do this before allocating a large DeviceBatch."""
    _lib.release_buffers(device)


def max_regret(regrets: np.ndarray) -> float:
    """fast_algorithms.py:228, :242-243 — max over runs starting from 0.0 (`reg > max`)."""
    r = np.asarray(regrets, dtype=np.float64)
    pos = r[r > 0.0]
    return float(pos.max()) if pos.size else 0.0


def gT_max(T: int, runs: int, *, base_seed: int = 0, d: int = 5, eta0: float = SQRT2,
           run0: int = 0, lanes_per_seq: int = LANES_BEST, device: int = 0) -> float:
    """max(0, max of gT_regrets(...)) reduced on device (``ocx_gT_max``): the regrets never
    leave the GPU (fast_algorithms.py:228, :242-243)."""
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    out = np.zeros(1)
    _lib.call("ocx_gT_max", int(base_seed), int(T), int(run0), int(runs), int(d), float(eta0),
              int(lanes_per_seq), int(device), ptr(out))
    return float(out[0])


def gT_sweep(T_grid: Sequence[int], runs: int, *, base_seed: int = 0, d: int = 5,
             eta0: float = SQRT2, devices: Optional[Sequence[int]] = None,
             lanes_per_seq: int = LANES_BEST, return_regrets: bool = True) -> dict:
    """empirical_worst_case_thresholds on one or several GPUs of this process
    (``ocx_gT_sweep_devices``).

    For every T the runs are split into contiguous shards, one per device, each generated
    and simulated on its own GPU by a native host thread; the per-shard regrets land in
    run order.  Returns {T: (g(T), regrets[runs])}; with ``return_regrets=False`` each
    shard's max is reduced on its GPU and the regrets entry is None."""
    devs = [int(v) for v in devices] if devices else [0]
    grid = np.ascontiguousarray([int(T) for T in T_grid], dtype=np.int64)
    regs = np.zeros((len(grid), int(runs)), dtype=np.float64) if return_regrets else None
    gmax = np.zeros(len(grid), dtype=np.float64)
    dv = (ctypes.c_int * len(devs))(*devs)
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    _lib.call("ocx_gT_sweep_devices", grid.ctypes.data_as(_lib.c_i64p), len(grid), int(runs),
              int(base_seed), int(d), float(eta0), dv, len(devs), int(lanes_per_seq),
              ptr(gmax), ptr(regs))
    return {int(T): (float(gmax[i]), regs[i] if regs is not None else None)
            for i, T in enumerate(grid)}


# ---------------------------------------------------------------------------
# Device-resident batches (torch tensors as HBM buffers)
# ---------------------------------------------------------------------------

def tiled_rows(z_tiled, y_tiled, L, seqs):
    """z [n, T, d] and y [n, T] (row-major, contiguous) of the sequences ``seqs`` (int64 tensor
    of batch indices), gathered out of tiled tensors of layout L (include/ocx.h ocx_layout:
    z_tiled[((k*G + g)*T + t)*128 + L*2 + e], y_tiled[(g*T + t)*S + s]).  Reads only."""
    K, G, T, S, P = L.C // 2, L.G, L.T, L.S, L.P
    g, s = seqs // S, seqs % S
    z5 = z_tiled[:K * G * T * 128].view(K, G, T, S, P, 2)
    zs = z5[:, g, :, s, :, :]                      # [n, K, T, P, 2]
    zs = zs.permute(0, 2, 3, 1, 4).reshape(seqs.numel(), T, P * L.C)[:, :, :L.d]
    ys = y_tiled[:G * T * S].view(G, T, S)[g, :, s]  # [n, T]
    return zs.contiguous(), ys.contiguous()


class DeviceBatch:
    """B sequences of T steps in d dimensions, resident in HBM in the tiled layout.

    ``stream`` is a torch.cuda.Stream (default: the current stream); every kernel
    of this object is launched on it, so torch events recorded on that stream
    bracket the HIP kernels exactly.

    Beside the label tile ``y`` the batch owns the label-bit tile (include/ocx.h): one bit per
    label, filled by generate_gT and pack, and read by simulate_alg instead
    of ``y``'s doubles while it is known to describe them (``label_bits_valid``).  ``y`` is a
    property: any access from outside may write labels in place, so it marks the bits invalid
    until the next producer call."""

    def __init__(self, B: int, T: int, d: int, *, lanes_per_seq: int = LANES_BEST, device: int = 0,
                 stream=None):
        import torch
        self.torch = torch
        self.L = _lib.layout(B, T, d, lanes_per_seq)
        # bit-exact modes keep the reference's two-pass comparator sum (see simulate_alg)
        self.exact = lanes_per_seq == LANES_EXACT or lanes_per_seq < 0
        self.best = lanes_per_seq == LANES_BEST
        self.rows_clipped = False  # set by generate_gT: every ||z_t|| <= 1
        self.device = torch.device("cuda", device)
        with torch.cuda.device(self.device):
            self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            self.z = torch.empty(max(self.L.z_elems, 1), dtype=torch.float64, device=self.device)
            self._y = torch.empty(max(self.L.y_elems, 1), dtype=torch.float64, device=self.device)
            nbits = self.L.G * ((self.L.T + 63) // 64) * self.L.S
            self._ybits = torch.zeros(max(nbits, 1), dtype=torch.int64, device=self.device)
            self._bits_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.regret = torch.zeros(max(B, 1), dtype=torch.float64, device=self.device)
            self.cum = torch.zeros_like(self.regret)
            self.comp = torch.zeros_like(self.regret)
        self.cum_exact = None  # allocated by ftrl_vs_exact
        # whether the label-bit tile describes y (set by the producers, cleared by any access
        # to y from outside)
        self._bits_state = "invalid"

    @property
    def y(self):
        """The label tile (y_tiled).  Handing it out marks the label bits invalid: the caller
        may write labels in place."""
        self._bits_state = "invalid"
        return self._y

    @y.setter
    def y(self, value):
        self._bits_state = "invalid"
        self._y = value

    @property
    def label_bits_valid(self) -> bool:
        """Whether the label-bit tile describes ``y`` (every label of a real sequence ±1), so
        simulate_alg may read it.  Host state only: no device read, no synchronisation."""
        return self._bits_state == "valid"

    @property
    def _sp(self):
        return ctypes.c_void_p(self.stream.cuda_stream)

    def _on_stream(self):
        """Context that makes self.stream current on this device: helper tensors (seeds,
        thresholds, device-side dtype conversions) are then produced in the same stream
        order as the HIP kernels that read them."""
        return self.torch.cuda.stream(self.stream)

    def _hold(self, *tensors):
        """Keep helper tensors alive for the kernels queued on self.stream, and tell the
        caching allocator they are in use there (record_stream), so their memory is not
        handed out again before those kernels ran even if the next call replaces them."""
        for t in tensors:
            if t is not None and t.is_cuda:
                t.record_stream(self.stream)
        return tensors

    def _lp(self):
        return ctypes.byref(self.L)

    def _call(self, name, *args):
        """_lib.call with this batch's device current: the null stream of a torch device is
        the current device's, and the library sizes its launches and forks its streams
        from the current device (a DeviceBatch on device 1 works without set_device)."""
        with self.torch.cuda.device(self.device):
            return _lib.call(name, *args)

    def generate_gT(self, base_seed: int = 0, run0: int = 0):
        """Fill z/y with _rng(base_seed, T, run0 + b) sequences (on device)."""
        self._bits_state = "invalid"
        self._call("ocx_dev_gen_gT_bits", self._lp(), int(base_seed), int(run0), self.z.data_ptr(),
                  self._y.data_ptr(), self._ybits.data_ptr(), self._sp)
        self.rows_clipped = True
        self._bits_state = "valid"
        return self

    FAMILIES = {"iid": 1, "massart": 2, "flip": 3, "switching": 4}

    def generate_family(self, family, run_seeds=None, stream_ids=None, *, p: float = 0.10,
                        block_len: int = 20):
        """Fill z/y with a sequence_generation.py family (ocx_dev_gen_family): for the
        random families sequence b is _rng(run_seeds[b], T, stream_ids[b])."""
        torch = self.torch
        fam = self.FAMILIES[family] if isinstance(family, str) else int(family)
        rs = si = None
        if fam in (1, 2):
            with self._on_stream():
                rs = torch.as_tensor(np.asarray(run_seeds, dtype=np.uint64).astype(np.int64)
                                     ).to(self.device)
                si = torch.as_tensor(np.asarray(stream_ids, dtype=np.uint64).astype(np.int64)
                                     ).to(self.device)
            if rs.numel() != self.L.B or si.numel() != self.L.B:
                raise ValueError("need one run seed and one stream id per sequence")
        self.rows_clipped = False
        self._bits_state = "invalid"
        self._call("ocx_dev_gen_family", self._lp(), fam,
                  rs.data_ptr() if rs is not None else None,
                  si.data_ptr() if si is not None else None, float(p), int(block_len),
                  self.z.data_ptr(), self._y.data_ptr(), self._sp)
        self._keep_seeds = self._hold(rs, si)
        return self

    def pack(self, z, y):
        """Copy host/device arrays z [B,T,d], y [B,T] into the tiled layout, and the labels into
        the label-bit tile, which is kept only if every label is exactly ±1 (a device flag,
        read back here: pack synchronises the batch's stream)."""
        torch = self.torch
        with self._on_stream():
            zt = torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64)
                                 if isinstance(z, np.ndarray) else z
                                 ).to(self.device, torch.float64).contiguous()
            yt = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float64)
                                 if isinstance(y, np.ndarray) else y
                                 ).to(self.device, torch.float64).contiguous()
        if tuple(zt.shape) != (self.L.B, self.L.T, self.L.d) or tuple(yt.shape) != (self.L.B, self.L.T):
            raise ValueError("z/y shape does not match the batch")
        self.rows_clipped = False
        self._bits_state = "invalid"
        self._call("ocx_dev_pack_bits", self._lp(), zt.data_ptr(), yt.data_ptr(), self.z.data_ptr(),
                  self._y.data_ptr(), self._ybits.data_ptr(), self._bits_flag.data_ptr(), self._sp)
        # kept only if the kernel's flag stayed clear.  The flag is read here, on this batch's
        # stream (the one its kernel ran on), so pack synchronises that stream — it already waits
        # for its host-to-device copies — and simulate_alg never does.
        with self._on_stream():
            not_unit = int(self._bits_flag.item())
        self._bits_state = "invalid" if not_unit else "valid"
        self._keep = self._hold(zt, yt)
        return self

    def simulate_alg(self, alg_flag: int = 0, eta0: float = SQRT2, comparator=None,
                     x_last=None, closed_comparator: Optional[bool] = None, closed_out=None):
        """Launch the FTRL/FTL kernel; results land in self.regret/cum/comp (async).

        ``closed_comparator`` (default: the layout is not a bit-exact mode) takes the
        comparator loss in closed form, T/2 - ||theta_T||, wherever the kernel certifies
        it — every row inside the unit ball, every sub-gradient -y_t/2, checked on device
        per sequence — and so reads z once instead of twice (ocx_dev_simulate_alg_ex,
        OCX_ALG_CLIPPED_ROWS); the regret then equals the reference's up to rounding.  It is
        safe on any data: sequences that fail the check stream the second pass and are
        bit-identical to ``closed_comparator=False``.
        ``closed_out`` ([B] int32 device tensor, optional) receives 1 per sequence that took
        the closed form, 0 where the kernel streamed the second pass.
        While ``label_bits_valid`` the pipelined kernel's instances built for it read the
        label-bit tile instead of ``y`` (ocx_dev_simulate_alg_bits): the same results bit for
        bit; OCX_LABEL_BITS=0 in the environment keeps every launch on ``y``."""
        cp = comparator.data_ptr() if comparator is not None else None
        xp = x_last.data_ptr() if x_last is not None else None
        if closed_comparator is None:
            closed_comparator = not self.exact and comparator is None
        flags = _lib.OCX_ALG_CLIPPED_ROWS if closed_comparator else 0
        bits = (self._ybits.data_ptr() if comparator is None and x_last is None
                and self.label_bits_valid else None)
        self._call("ocx_dev_simulate_alg_bits", self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                  bits, int(alg_flag), float(eta0), cp, self.regret.data_ptr(), self.cum.data_ptr(),
                  self.comp.data_ptr(), xp, flags,
                  closed_out.data_ptr() if closed_out is not None else None, self._sp)
        return self.regret

    def simulate_alg_curve(self, checkpoints, alg_flag: int = 0, eta0: float = SQRT2,
                           closed_comparator: Optional[bool] = None):
        """Regret curves of the resident batch (ocx_dev_simulate_alg_curve, async): FTRL / FTL
        observed at every horizon of ``checkpoints`` (strictly increasing in [0, T], validated
        here) in one pass over z.  Returns device tensors ``regret``, ``cum``, ``comp``
        (float64) and ``closed`` (int32), each [B, K]; column k is what simulate_alg gives on
        the batch truncated at t_k, bit for bit in the same layout.  ``closed_comparator``
        defaults as in simulate_alg; a (sequence, checkpoint) pair the kernel cannot certify
        streams the comparator pass over its prefix."""
        torch = self.torch
        ck = _checkpoints(checkpoints, self.L.T)
        K, B = int(ck.size), int(self.L.B)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLIPPED_ROWS if closed_comparator else 0
        nbytes = int(_lib.load().ocx_curve_workspace_bytes(self._lp(), K))
        if nbytes < 0:
            _lib.check(nbytes, "ocx_curve_workspace_bytes")
        with torch.cuda.device(self.device), self._on_stream():
            ckd = torch.as_tensor(ck).to(self.device)
            out = {k: torch.zeros((B, K), dtype=torch.float64, device=self.device)
                   for k in ("regret", "cum", "comp")}
            out["closed"] = torch.zeros((B, K), dtype=torch.int32, device=self.device)
            ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        self._call("ocx_dev_simulate_alg_curve", self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                   int(alg_flag), float(eta0), ckd.data_ptr() if K else None, K,
                   out["regret"].data_ptr(), out["cum"].data_ptr(), out["comp"].data_ptr(),
                   out["closed"].data_ptr(), flags, ws.data_ptr(), ws.numel() * 8, self._sp)
        self._keep_curve = self._hold(ckd, ws)
        return out

    def simulate_alg_anytime(self, checkpoints=None, alg_flag: int = 0, eta0: float = SQRT2,
                             closed_comparator: Optional[bool] = None, trace: bool = False):
        """Anytime regret of the resident batch: the running max of FTRL / FTL's regret over
        EVERY prefix.  With R_t column t of ``simulate_alg_curve(range(1, T + 1), alg_flag, eta0,
        closed_comparator)``, returns device tensors

          ``sup``       [B, K] float64: max of R_t over t = 1 … t_k,
          ``argsup``    [B, K] int64: the smallest t attaining it,
          ``open_from`` [B] int64: the first t whose prefix the kernel could not certify
                        (T + 1: none),
          ``trace``     [B, T] float64, R_1 … R_T (only with ``trace=True``),

        for the horizons t_k of ``checkpoints`` (default ``[T]``; strictly increasing integers
        in [1, T], validated here; T = 0 allows only an empty list).  ``closed_comparator``
        defaults as in simulate_alg_curve.

        Cost.  With the closed form (ocx_dev_simulate_alg_anytime) the certified prefixes take
        ONE pass over z, no workspace, one extra norm of theta per step: O(T) per sequence.
        The prefixes the kernel cannot certify (t >= open_from: exact ties on the deterministic
        families, edited rows) are completed by simulate_alg_curve on this same batch — the
        same layout, hence the same bits — at every horizon from min(open_from) to the last
        one asked for, in chunks whose curve workspace stays under 1 GiB; each uncertified
        (sequence, t) pair streams its prefix, O(T²) rows per open sequence.  Only the open
        (sequence, t) entries are folded in; on equal values the earlier t wins.
        ``closed_comparator=False`` produces the whole result this way without the new kernel:
        the bit-exact mode, O(T²) for every sequence (open_from is then 1 throughout).
        Synchronises once (open_from is read to decide on the completion).  With K = 0 and no
        trace nothing runs and open_from stays T + 1."""
        torch = self.torch
        T, B = int(self.L.T), int(self.L.B)
        ck = _anytime_checkpoints(checkpoints, T)
        K = int(ck.size)
        if closed_comparator is None:
            closed_comparator = not self.exact
        closed_comparator = bool(closed_comparator)
        G, S = int(self.L.G), int(self.L.S)
        with torch.cuda.device(self.device), self._on_stream():
            ckd = torch.as_tensor(ck).to(self.device)
            sup = torch.full((B, K), -math.inf, dtype=torch.float64, device=self.device)
            argsup = torch.zeros((B, K), dtype=torch.int64, device=self.device)
            open_from = torch.full((B,), T + 1 if closed_comparator else 1, dtype=torch.int64,
                                   device=self.device)
            tt = (torch.full((max(int(self.L.y_elems), 1),), math.nan, dtype=torch.float64,
                             device=self.device) if trace else None)
        out = {"sup": sup, "argsup": argsup, "open_from": open_from}
        if B == 0 or T == 0 or (K == 0 and not trace):
            if trace:
                out["trace"] = torch.zeros((B, T), dtype=torch.float64, device=self.device)
            return out
        if closed_comparator:
            self._call("ocx_dev_simulate_alg_anytime", self._lp(), self.z.data_ptr(),
                       self._y.data_ptr(), int(alg_flag), float(eta0),
                       ckd.data_ptr() if K else None, K, sup.data_ptr(), argsup.data_ptr(),
                       open_from.data_ptr(), tt.data_ptr() if trace else None,
                       _lib.OCX_ALG_CLIPPED_ROWS, self._sp)
            self._keep_anytime = self._hold(ckd, tt)
        with torch.cuda.device(self.device), self._on_stream():
            tr = None
            if trace:  # [G, T, S] -> [G·S, T][:B]: views and one copy, no kernel of ours
                tr = tt[:G * T * S].view(G, T, S).permute(0, 2, 1).reshape(G * S, T)[:B].contiguous()
                out["trace"] = tr
            lo0 = int(open_from.min().item())
        hi0 = T if trace else int(ck[-1])
        if lo0 > hi0:
            return out
        # completion of the open prefixes from the dense curve, a chunk of horizons at a time
        per_ck = max(int(_lib.load().ocx_curve_workspace_bytes(self._lp(), 1)), 1)
        chunk = max(1, (1 << 30) // per_ck)
        with torch.cuda.device(self.device), self._on_stream():
            if K:  # the max over the certified prefix of every sequence that is completed
                run_best, run_arg = sup[:, K - 1].clone(), argsup[:, K - 1].clone()
            else:
                run_best = torch.full((B,), -math.inf, dtype=torch.float64, device=self.device)
                run_arg = torch.zeros((B,), dtype=torch.int64, device=self.device)
        for lo in range(lo0, hi0 + 1, chunk):
            hi = min(lo + chunk - 1, hi0)
            reg = self.simulate_alg_curve(np.arange(lo, hi + 1, dtype=np.int64), alg_flag, eta0,
                                          closed_comparator)["regret"]
            with torch.cuda.device(self.device), self._on_stream():
                run_best, run_arg = _anytime_fold(torch, reg, lo, open_from, ck, sup, argsup,
                                                  run_best, run_arg, tr)
        return out

    def simulate_alg_etas(self, etas, closed_comparator: Optional[bool] = None, *, _group=None):
        """Step-size sweep of the resident batch (ocx_dev_simulate_alg_etas, async): FTRL for
        every eta0 of ``etas`` (a one-dimensional list of real numbers, validated here), each
        pass over z serving ocx_etas_group(L, M) of them.  Returns device tensors ``regret``,
        ``cum``, ``comp`` (float64) and ``closed`` (int32), each [B, M]; column m is what
        simulate_alg(0, etas[m]) gives, bit for bit in the same layout.  ``closed_comparator``
        defaults as in simulate_alg; a (sequence, eta) pair the kernel cannot certify streams
        the comparator pass.  (``_group``: tests and tools/etas_probe.py force the group size
        through include/ocx_testing.h.)"""
        torch = self.torch
        et = _etas(etas)
        M, B = int(et.size), int(self.L.B)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLIPPED_ROWS if closed_comparator else 0
        with torch.cuda.device(self.device), self._on_stream():
            out = {k: torch.zeros((B, M), dtype=torch.float64, device=self.device)
                   for k in ("regret", "cum", "comp")}
            out["closed"] = torch.zeros((B, M), dtype=torch.int32, device=self.device)
        args = (self._lp(), self.z.data_ptr(), self._y.data_ptr(), ptr(et), M,
                out["regret"].data_ptr(), out["cum"].data_ptr(), out["comp"].data_ptr(),
                out["closed"].data_ptr(), flags)
        if _group is None:
            self._call("ocx_dev_simulate_alg_etas", *args, self._sp)
        else:
            self._call("ocx_test_simulate_alg_etas", *args, int(_group), self._sp)
        return out

    def simulate_alg_curve_etas(self, checkpoints, etas,
                                closed_comparator: Optional[bool] = None, *, _group=None):
        """Regret grid of the resident batch (ocx_dev_simulate_alg_curve_etas, async): FTRL for
        every eta0 of ``etas`` (validated as in simulate_alg_etas) observed at every horizon
        of ``checkpoints`` (validated as in simulate_alg_curve), each pass over z serving
        ocx_curve_etas_group(L, M) step sizes.  Returns device tensors ``regret``, ``cum``,
        ``comp`` (float64) and ``closed`` (int32), each [B, M, K]; element (b, m, k) is what
        simulate_alg(0, etas[m]) gives on the batch truncated at t_k, bit for bit in the same
        layout — [:, m, :] is simulate_alg_curve(checkpoints, 0, etas[m]) and, with t_K = T,
        [:, :, -1] is simulate_alg_etas(etas).  ``closed_comparator`` defaults as in
        simulate_alg; a (sequence, eta, checkpoint) triple the kernel cannot certify streams
        the comparator pass over its prefix.  (``_group``: tests and tools/grid_probe.py force
        the group size through include/ocx_testing.h.)"""
        torch = self.torch
        ck = _checkpoints(checkpoints, self.L.T)
        et = _etas(etas)
        K, M, B = int(ck.size), int(et.size), int(self.L.B)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLIPPED_ROWS if closed_comparator else 0
        nbytes = int(_lib.load().ocx_curve_etas_workspace_bytes(self._lp(), K, M))
        if nbytes < 0:
            _lib.check(nbytes, "ocx_curve_etas_workspace_bytes")
        if _group is not None:  # a forced group may hold more columns than the dispatcher's
            nbytes = max(nbytes, int(self.L.G) * K * min(int(_group), M) * 64
                         * (8 * int(self.L.C) + 12))
        with torch.cuda.device(self.device), self._on_stream():
            ckd = torch.as_tensor(ck).to(self.device)
            out = {k: torch.zeros((B, M, K), dtype=torch.float64, device=self.device)
                   for k in ("regret", "cum", "comp")}
            out["closed"] = torch.zeros((B, M, K), dtype=torch.int32, device=self.device)
            ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        head = (self._lp(), self.z.data_ptr(), self._y.data_ptr(), ptr(et), M,
                ckd.data_ptr() if K else None, K, out["regret"].data_ptr(),
                out["cum"].data_ptr(), out["comp"].data_ptr(), out["closed"].data_ptr(), flags)
        tail = (ws.data_ptr(), ws.numel() * 8, self._sp)
        if _group is None:
            self._call("ocx_dev_simulate_alg_curve_etas", *head, *tail)
        else:
            self._call("ocx_test_simulate_alg_curve_etas", *head, int(_group), *tail)
        self._keep_grid = self._hold(ckd, ws)
        return out

    def simulate_smart(self, thresh, eta0: float = SQRT2, switch_step=None,
                       closed_prefix: Optional[bool] = None,
                       closed_comparator: Optional[bool] = None, stats=None):
        """SMART (fast_algorithms.py:118-164) on the resident batch; thresh scalar or [B].

        ``closed_prefix`` (default: not a bit-exact layout) runs in O(T·d): the pre-switch
        prefix loss in closed form, deciding the switch only outside a rounding guard band
        and re-scanning the prefix inside it (the reference's switch steps; see
        include/ocx.h, OCX_SMART_CLOSED_PREFIX).  ``closed_comparator`` (same default) takes
        the final comparator loss in closed form where certified.  ``stats`` ([2] uint64
        (int64) device tensor, optional) accumulates re-scanned steps and closed-comparator
        sequences."""
        with self._on_stream():
            th = self.torch.as_tensor(np.broadcast_to(np.asarray(thresh, dtype=np.float64),
                                                      (self.L.B,)).copy()).to(self.device)
        sp = switch_step.data_ptr() if switch_step is not None else None
        if closed_prefix is None:
            closed_prefix = not self.exact
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = ((_lib.OCX_SMART_CLOSED_PREFIX if closed_prefix else 0) |
                 (_lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0))
        self._call("ocx_dev_simulate_smart_ex", self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                  th.data_ptr(), float(eta0), self.regret.data_ptr(), sp, flags,
                  stats.data_ptr() if stats is not None else None, self._sp)
        self._keep_th = self._hold(th)
        return self.regret

    def simulate_smart_thresholds(self, thresholds, eta0: float = SQRT2, *,
                                  closed_prefix: Optional[bool] = None,
                                  closed_comparator: Optional[bool] = None, stats=None,
                                  _group=None, _wave=None):
        """Threshold sweep of the resident batch (ocx_dev_simulate_smart_thresholds, async):
        SMART for every switch threshold of ``thresholds`` ([M], or [B, M] per sequence;
        validated here, NaN and ±inf are legal), each pass over z serving
        ocx_smart_thresholds_group(L, M) of them.  In a bit-exact layout, in the re-scan mode
        (both flags off) without ``stats``, at d <= 64 and B <= 32768 the call runs the
        one-wave-per-sequence kernel (ocx_smart_wave_cols.hip: one prefix re-scan per step for
        up to eight columns; the same bits), elsewhere the lane-group kernel;
        ``OCX_SMART_KERNEL=lanes`` holds it on the latter.  Returns device tensors ``regret`` [B, M]
        float64 and ``switch_step`` [B, M] int64 (-1 = never); column m is what
        simulate_smart(thresholds[..., m], eta0, stats=...) gives, bit for bit in the same
        layout.  ``thresh = +inf`` makes a column FTL's regret, with the same adds and the same
        comparator; ``sqrt(2T)`` and the empirical g(T) are the drivers' SMART and EMP.
        ``closed_prefix`` / ``closed_comparator`` default as in simulate_smart; ``stats``
        ([2] int64 device tensor, optional) accumulates, per pass, the (sequence, step) pairs
        that re-scanned — once per step however many columns needed it — and the sequences
        that took the closed comparator.  (``_group``: tests and tools/thresholds_probe.py
        force the group size through include/ocx_testing.h; ``_wave``: tests and
        tools/smart_wave_cols_probe.py force the one-wave-per-sequence kernel with that group
        size, 1, 2, 4 or 8, in any layout — re-scan mode only.)"""
        torch = self.torch
        B = int(self.L.B)
        tha = _thresholds(thresholds, B)
        M = int(tha.shape[1])
        if _wave is not None and (closed_prefix or closed_comparator or _group is not None):
            raise ValueError("_wave runs the re-scan mode only, and excludes _group")
        if closed_prefix is None:
            closed_prefix = not self.exact
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = ((_lib.OCX_SMART_CLOSED_PREFIX if closed_prefix else 0) |
                 (_lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0))
        with torch.cuda.device(self.device), self._on_stream():
            th = torch.as_tensor(tha).to(self.device)
            out = {"regret": torch.zeros((B, M), dtype=torch.float64, device=self.device),
                   "switch_step": torch.full((B, M), -1, dtype=torch.int64, device=self.device)}
        args = (self._lp(), self.z.data_ptr(), self._y.data_ptr(), th.data_ptr() if B * M else None,
                M, float(eta0), out["regret"].data_ptr() if B * M else None,
                out["switch_step"].data_ptr() if B * M else None, flags,
                stats.data_ptr() if stats is not None else None)
        if _wave is not None:
            self._call("ocx_test_simulate_smart_wave_cols", *args[:3], None, *args[3:8], args[9],
                       int(_wave), self._sp)
        elif _group is None:
            self._call("ocx_dev_simulate_smart_thresholds", *args, self._sp)
        else:
            self._call("ocx_test_simulate_smart_thresholds", *args, int(_group), self._sp)
        self._keep_th = self._hold(th)
        return out

    def simulate_smart_curve(self, horizons, thresholds=None, eta0: float = SQRT2, *,
                             closed_prefix: Optional[bool] = None,
                             closed_comparator: Optional[bool] = None, stats=None,
                             _group=None, _wave=None):
        """SMART regret curves of the resident batch (ocx_dev_simulate_smart_curve, async):
        SMART for K pairs (horizon t_k, threshold), each pass over z serving
        ocx_smart_curve_group(L, K) consecutive pairs and stopping at their last horizon.
        The one-wave-per-sequence kernel runs where simulate_smart_thresholds says it does.
        ``horizons`` [K]: integers, non-decreasing in [0, T] (validated here; equal horizons
        are legal); ``thresholds`` [K] or [B, K] (validated through _thresholds; None: SMART's
        own sqrt(2 t_k)).  Returns device tensors ``regret`` [B, K] float64 and ``switch_step``
        [B, K] int64 (in [0, t_k), or -1 = never); column k is what
        simulate_smart(thresholds[..., k], eta0, stats=...) gives on a batch of the first t_k
        rows, bit for bit in the same layout.  ``closed_prefix`` / ``closed_comparator``
        default as in simulate_smart; the closed comparator is certified per (sequence,
        column) by that column's first t_k steps.  ``stats`` ([2] int64 device tensor,
        optional) accumulates, per pass, the (sequence, step) pairs that re-scanned and the
        (sequence, column) pairs that took the closed comparator.  (``_group``: tests and
        tools/smart_curve_probe.py force the group size through include/ocx_testing.h;
        ``_wave``: as in simulate_smart_thresholds.)"""
        torch = self.torch
        B = int(self.L.B)
        hz = _horizons(horizons, self.L.T)
        tha = _smart_curve_thresholds(thresholds, hz, B)
        K = int(hz.size)
        if _wave is not None and (closed_prefix or closed_comparator or _group is not None):
            raise ValueError("_wave runs the re-scan mode only, and excludes _group")
        if closed_prefix is None:
            closed_prefix = not self.exact
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = ((_lib.OCX_SMART_CLOSED_PREFIX if closed_prefix else 0) |
                 (_lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0))
        with torch.cuda.device(self.device), self._on_stream():
            th = torch.as_tensor(tha).to(self.device)
            out = {"regret": torch.zeros((B, K), dtype=torch.float64, device=self.device),
                   "switch_step": torch.full((B, K), -1, dtype=torch.int64, device=self.device)}
        args = (self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                hz.ctypes.data_as(_lib.c_i64p), th.data_ptr() if B * K else None, K, float(eta0),
                out["regret"].data_ptr() if B * K else None,
                out["switch_step"].data_ptr() if B * K else None, flags,
                stats.data_ptr() if stats is not None else None)
        if _wave is not None:
            self._call("ocx_test_simulate_smart_wave_cols", *args[:9], args[10], int(_wave),
                       self._sp)
        elif _group is None:
            self._call("ocx_dev_simulate_smart_curve", *args, self._sp)
        else:
            self._call("ocx_test_simulate_smart_curve", *args, int(_group), self._sp)
        self._keep_th = self._hold(th)
        return out

    def simulate_smart_grid(self, checkpoints, thresholds, eta0: float = SQRT2, *,
                            closed_prefix: Optional[bool] = None,
                            closed_comparator: Optional[bool] = None, stats=None,
                            _group=None, _wave=None):
        """SMART regret grid of the resident batch (ocx_dev_simulate_smart_grid, async): SMART
        for every switch threshold of ``thresholds`` ([M], or [B, M] per sequence; validated
        through _thresholds, NaN and ±inf are legal) observed at every horizon of
        ``checkpoints`` (strictly increasing in [0, T]; validated through _checkpoints), each
        pass over z serving ocx_smart_grid_group(L, M) thresholds and running once, to t_K.
        In a bit-exact layout, in the re-scan mode (both flags off) without ``stats``, at
        d <= 64 and B <= 32768 the one-wave-per-sequence kernel runs (the same bits).
        Returns device tensors ``regret`` [B, M, K] float64 and ``switch_step`` [B, M, K] int64
        (the full run's switch step where it lies before t_k, else -1); element (b, m, k) is
        what simulate_smart(thresholds[..., m], eta0, stats=...) gives on a batch of the first
        t_k rows, bit for bit in the same layout — [:, m, :] is simulate_smart_curve with that
        threshold at every checkpoint and, with t_K = T, [:, :, -1] is
        simulate_smart_thresholds.  ``closed_prefix`` / ``closed_comparator`` default as in
        simulate_smart; the closed comparator is certified per (sequence, checkpoint).
        ``stats`` ([2] int64 device tensor, optional) accumulates, per pass, the (sequence,
        step) pairs that re-scanned and the (sequence, column, checkpoint) triples that took
        the closed comparator.  (``_group``: tests and tools/smart_grid_probe.py force the
        lane-group kernel's group size through include/ocx_testing.h; ``_wave``: they force the
        one-wave-per-sequence kernel with that group size, 1, 2, 4 or 8, in any layout —
        re-scan mode only.)"""
        torch = self.torch
        B = int(self.L.B)
        ck = _checkpoints(checkpoints, self.L.T)
        tha = _thresholds(thresholds, B)
        K, M = int(ck.size), int(tha.shape[1])
        if _wave is not None and (closed_prefix or closed_comparator or _group is not None):
            raise ValueError("_wave runs the re-scan mode only, and excludes _group")
        if closed_prefix is None:
            closed_prefix = not self.exact
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = ((_lib.OCX_SMART_CLOSED_PREFIX if closed_prefix else 0) |
                 (_lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0))
        n = B * M * K
        with torch.cuda.device(self.device), self._on_stream():
            th = torch.as_tensor(tha).to(self.device)
            ckd = torch.as_tensor(ck).to(self.device)
            out = {"regret": torch.zeros((B, M, K), dtype=torch.float64, device=self.device),
                   "switch_step": torch.full((B, M, K), -1, dtype=torch.int64,
                                             device=self.device)}
        args = (self._lp(), self.z.data_ptr(), self._y.data_ptr(), th.data_ptr() if B * M else None,
                M, ckd.data_ptr() if K else None, K, float(eta0),
                out["regret"].data_ptr() if n else None,
                out["switch_step"].data_ptr() if n else None,
                0 if _wave is not None else flags,
                stats.data_ptr() if stats is not None else None)
        if _wave is not None:
            self._call("ocx_test_simulate_smart_wave_grid", *args, int(_wave), self._sp)
        elif _group is None:
            self._call("ocx_dev_simulate_smart_grid", *args, self._sp)
        else:
            self._call("ocx_test_simulate_smart_grid", *args, int(_group), self._sp)
        self._keep_sgrid = self._hold(th, ckd)
        return out

    def comparison_curves(self, checkpoints, g_emp=None, eta0: float = SQRT2):
        """The four lines of the reference's comparison figure (fast_driver.py:71-127) against
        the horizon, from this resident batch: a dict of [B, K] device tensors ``FTRL``,
        ``FTL``, ``SMART`` (threshold sqrt(2 t_k)) and, when ``g_emp`` ([K], the empirical
        g(t_k)) is given, ``EMP``.  ``checkpoints`` is strictly increasing in [0, T].  FTRL
        comes from simulate_alg_curve; the others from ONE simulate_smart_curve call over the
        2K or 3K pairs sorted by horizon, with thresholds +inf (a column that never switches
        is FTL's regret), sqrt(2 t_k) and g_emp[k].  Column k of each is the regret on the
        batch truncated at t_k."""
        ck = _checkpoints(checkpoints, self.L.T)
        K = int(ck.size)
        cols = [("FTL", np.full(K, np.inf)), ("SMART", np.sqrt(2.0 * ck.astype(np.float64)))]
        if g_emp is not None:
            g = _etas(g_emp)
            if g.shape != (K,):
                raise ValueError(f"g_emp must be [K = {K}], got shape {g.shape}")
            cols.append(("EMP", g))
        n = len(cols)
        hz = np.repeat(ck, n)                                    # t_0 × n, t_1 × n, ...
        th = np.stack([c[1] for c in cols], axis=1).reshape(-1)  # interleaved the same way
        out = {"FTRL": self.simulate_alg_curve(ck, 0, eta0)["regret"]}
        reg = self.simulate_smart_curve(hz, th, eta0)["regret"]
        with self._on_stream():
            for i, (name, _) in enumerate(cols):
                out[name] = reg[:, i::n].contiguous()
        return out

    def simulate_twin32(self, algo: int = 0, eta0: float = SQRT2, thresh=None):
        """The float32 twin (algorithms.py; twin32_batch) on the resident batch, which must
        use the one-lane layout (``lanes_per_seq=-1``): float32 results [B] on device."""
        torch = self.torch
        th = None
        with self._on_stream():
            res = torch.empty(max(self.L.B, 1), dtype=torch.float32, device=self.device)
            if int(algo) == 2:
                th = torch.as_tensor(np.broadcast_to(np.asarray(thresh, dtype=np.float64),
                                                     (self.L.B,)).copy()).to(self.device)
        self._call("ocx_dev_twin32", self._lp(), self.z.data_ptr(), self._y.data_ptr(), int(algo),
                  float(eta0), th.data_ptr() if th is not None else None, res.data_ptr(), None,
                  None, None, self._sp)
        if th is not None:
            self._keep_th = self._hold(th)
        return res

    def simulate_twin32_cols(self, horizons, algos=2, thresholds=None, eta0: float = SQRT2, *,
                             _group=None):
        """Twin sweeps on the resident batch (ocx_dev_twin32_cols, async; one-lane layout,
        ``lanes_per_seq=-1``): the float32 twin for K columns (horizon t_k, algorithm,
        threshold), ocx_twin32_cols_group(L, K) consecutive columns per launch, each launch
        staging the rows of its last horizon once and re-scanning the prefix once per step for
        all its columns.  Arguments as twin32_cols_batch (validated here).  Returns a dict of
        device tensors, each [B, K]: ``result`` float32, ``cum`` float64, ``comp`` float32,
        ``switch_step`` int64 (-1 = never, and every FTRL / FTL column); column k is what
        simulate_twin32(algos[k], eta0, thresholds[..., k]) gives on a batch of the first t_k
        rows, bit for bit.  A last horizon whose rows do not fit the LDS raises
        NotImplementedError.  (``_group``: tests force the columns per launch through
        include/ocx_testing.h.)"""
        torch = self.torch
        B = int(self.L.B)
        hz = _horizons(horizons, self.L.T)
        K = int(hz.size)
        al = _twin32_algos(algos, K)
        tha = _twin32_cols_thresholds(thresholds, hz, al, B)
        with torch.cuda.device(self.device), self._on_stream():
            th = torch.as_tensor(tha).to(self.device) if tha is not None else None
            out = {"result": torch.zeros((B, K), dtype=torch.float32, device=self.device),
                   "cum": torch.zeros((B, K), dtype=torch.float64, device=self.device),
                   "comp": torch.zeros((B, K), dtype=torch.float32, device=self.device),
                   "switch_step": torch.full((B, K), -1, dtype=torch.int64, device=self.device)}
        some = B * K > 0
        args = (self._lp(), self.z.data_ptr(), self._y.data_ptr(), K,
                hz.ctypes.data_as(_lib.c_i64p), al.ctypes.data_as(_lib.c_i32p), float(eta0),
                th.data_ptr() if th is not None and some else None,
                *(out[k].data_ptr() if some else None
                  for k in ("result", "cum", "comp", "switch_step")))
        if _group is None:
            _twin32_cols_call(self._call, "ocx_dev_twin32_cols", *args, self._sp)
        else:
            _twin32_cols_call(self._call, "ocx_test_twin32_cols", *args, int(_group), self._sp)
        if th is not None:
            self._keep_th = self._hold(th)
        return out

    def twin32_comparison_curves(self, checkpoints, g_emp=None, eta0: float = SQRT2):
        """The four lines of driver.py's comparison figure (driver.py:70-136, the float32 twin)
        against the horizon, from this resident batch: a dict of float32 [B, K] device tensors
        ``FTRL``, ``FTL``, ``SMART`` (threshold sqrt(2 t_k)) and, when ``g_emp`` ([K], the
        empirical g(t_k)) is given, ``EMP`` — ONE simulate_twin32_cols call over the 3K or 4K
        columns sorted by horizon.  ``checkpoints`` is strictly increasing in [0, T].  Column
        k of each is the twin's result on the batch truncated at t_k."""
        ck = _checkpoints(checkpoints, self.L.T)
        K = int(ck.size)
        nan = np.full(K, np.nan)
        cols = [("FTRL", 0, nan), ("FTL", 1, nan),
                ("SMART", 2, np.sqrt(2.0 * ck.astype(np.float64)))]
        if g_emp is not None:
            g = _etas(g_emp)
            if g.shape != (K,):
                raise ValueError(f"g_emp must be [K = {K}], got shape {g.shape}")
            cols.append(("EMP", 2, g))
        n = len(cols)
        hz = np.repeat(ck, n)                                    # t_0 × n, t_1 × n, ...
        al = np.tile(np.array([c[1] for c in cols], dtype=np.int32), K)
        th = np.stack([c[2] for c in cols], axis=1).reshape(-1)  # interleaved the same way
        res = self.simulate_twin32_cols(hz, al, th, eta0)["result"]
        with self._on_stream():
            return {name: res[:, i::n].contiguous() for i, (name, _, _) in enumerate(cols)}

    def ftl_exact(self, cmp_action=None, regime=None, norm: str = "l2"):
        """Exact FTL (l2 ball, closed form; see ftl_exact_batch) on the resident batch:
        self.cum / self.comp get the replay and comparator losses, ``cmp_action``
        [B, d] (device, optional) the exact comparator, ``regime`` [B] int32 the
        regime flags (allocated when None).  Returns regime."""
        torch = self.torch
        if regime is None:
            with self._on_stream():
                regime = torch.zeros(max(self.L.B, 1), dtype=torch.int32, device=self.device)
        self._call("ocx_dev_ftl_exact", self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                  _norm_code(norm),
                  self.cum.data_ptr(), self.comp.data_ptr(),
                  cmp_action.data_ptr() if cmp_action is not None else None,
                  regime.data_ptr(), self._sp)
        return regime

    def ftrl_vs_exact(self, eta0: float = SQRT2, comp_ftl=None, cmp_action=None, regime=None,
                      closed_comparator: Optional[bool] = None, norm: str = "l2"):
        """ftrl_vs_exact_batch on the resident batch: self.cum gets FTRL's cumulative loss,
        self.comp the exact comparator's loss, self.cum_exact exact FTL's (allocated on first
        use); ``comp_ftl`` [B] (device, optional) the loss of FTL(theta_ftrl).  Returns the
        regime flags.  ``closed_comparator`` (default: not a bit-exact layout) takes both
        comparator losses in closed form for the sequences the kernel finds in the unit-ball
        regime (ocx_dev_ftrl_vs_exact_ex): one HBM pass instead of two.  Under
        OCX_LANES_BEST the kernel sums with the butterfly (OCX_ALG_TREE_SUMS)."""
        torch = self.torch
        n = max(self.L.B, 1)
        with self._on_stream():
            if self.cum_exact is None:
                self.cum_exact = torch.zeros(n, dtype=torch.float64, device=self.device)
            if regime is None:
                regime = torch.zeros(n, dtype=torch.int32, device=self.device)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0
        if self.best and self.L.chain:
            # OCX_LANES_BEST: chained totals leave this kernel latency-bound (43 vs 28 ms at
            # 32768 x 1e4 x 64, profiles/r02_fused_exact_lanes.jsonl): butterfly sums instead
            flags |= _lib.OCX_ALG_TREE_SUMS
        self._call("ocx_dev_ftrl_vs_exact_ex", self._lp(), self.z.data_ptr(), self._y.data_ptr(),
                  float(eta0), self.cum.data_ptr(), self.cum_exact.data_ptr(),
                  self.comp.data_ptr(), comp_ftl.data_ptr() if comp_ftl is not None else None,
                  cmp_action.data_ptr() if cmp_action is not None else None, regime.data_ptr(),
                  _norm_code(norm), flags, self._sp)
        return regime

    def exact_general(self, norm: str = "l2", all_prefixes: bool = True):
        """The general exact-FTL solver (exact_ball_solve) on the resident batch
        (ocx_dev_exact_ball_solve_tiled, d <= 256): a dict of device tensors ``actions``
        [B, NP, d], ``obj``, ``gap``, ``step_loss`` [B, NP] and ``info`` (int32), NP = T+1
        or 1 (async on self.stream)."""
        torch = self.torch
        B, T, d = self.L.B, self.L.T, self.L.d
        if d > _lib.OCX_EXACT_BALL_MAX_D:
            raise NotImplementedError(f"the general exact-FTL solver takes d <= "
                                      f"{_lib.OCX_EXACT_BALL_MAX_D} (got {d})")
        NP = T + 1 if all_prefixes else 1
        with self._on_stream():
            out = {"actions": torch.zeros((max(B, 1), NP, d), dtype=torch.float64,
                                          device=self.device)}
            for k in ("obj", "gap", "step_loss"):
                out[k] = torch.zeros((max(B, 1), NP), dtype=torch.float64, device=self.device)
            out["info"] = torch.zeros((max(B, 1), NP), dtype=torch.int32, device=self.device)
        self._call("ocx_dev_exact_ball_solve_tiled", self._lp(), self.z.data_ptr(),
                  self._y.data_ptr(), _norm_code(norm), int(bool(all_prefixes)),
                  out["actions"].data_ptr(), out["obj"].data_ptr(), out["gap"].data_ptr(),
                  out["step_loss"].data_ptr(), out["info"].data_ptr(), self._sp)
        return out

    def ftrl_vs_exact_general(self, eta0: float = SQRT2, norm: str = "l2"):
        """ftrl_vs_exact with every sequence's exact side valid: the closed form where the
        kernel finds the regime, the general solver (exact_general) elsewhere.  Leaves
        self.cum (FTRL), self.cum_exact and self.comp as ftrl_vs_exact does; returns the
        regime flags.  Synchronises once (to see whether any sequence left the regime)."""
        torch = self.torch
        regime = self.ftrl_vs_exact(eta0, norm=norm)
        B, T, d = self.L.B, self.L.T, self.L.d
        self.exact_gap_max = 0.0
        with self._on_stream():
            ok = regime[:B].bool()
            if bool(ok.all().item()):
                return regime
            # only the sequences outside the regime: their rows out of the tile, row-major
            bad = torch.nonzero(~ok).flatten()
            zb, yb = tiled_rows(self.z, self._y, self.L, bad)  # read only: the bits stay valid
            nb = int(bad.numel())
            res = {"actions": torch.zeros((nb, T + 1, d), dtype=torch.float64, device=self.device)}
            for k in ("obj", "gap", "step_loss"):
                res[k] = torch.zeros((nb, T + 1), dtype=torch.float64, device=self.device)
            res["info"] = torch.zeros((nb, T + 1), dtype=torch.int32, device=self.device)
            self._call("ocx_dev_exact_ball_solve", zb.data_ptr(), yb.data_ptr(), nb, T, d,
                      _norm_code(norm), 1, res["actions"].data_ptr(), res["obj"].data_ptr(),
                      res["gap"].data_ptr(), res["step_loss"].data_ptr(),
                      res["info"].data_ptr(), self._sp)
            self._hold(zb, yb)
            host = {k: res[k].cpu().numpy() for k in ("obj", "gap", "info", "step_loss")}
            self.exact_gap_max = check_certificates(host["obj"], host["gap"], host["info"])
            # exact FTL's cumulative loss in step order (the host path's and the replay's)
            gcum = np.cumsum(host["step_loss"][:, :T], axis=1)[:, -1] if T > 0 else np.zeros(nb)
            self.cum_exact[bad] = torch.as_tensor(gcum).to(self.device)
            self.comp[bad] = res["obj"][:, T]
        return regime

    def ftrl_vs_exact_curve(self, checkpoints, eta0: float = SQRT2, *, norm: str = "l2",
                            closed_comparator: Optional[bool] = None,
                            with_ftl_comparator: bool = False, with_actions: bool = False):
        """FTRL-vs-exact-FTL regret curves of the resident batch (ocx_dev_ftrl_vs_exact_curve,
        async): both loops of ftrl_vs_exact observed at every horizon of ``checkpoints``
        (strictly increasing in [0, T], validated here) in one pass over z.  Returns a dict of
        [B, K] device tensors: ``ftrl`` and ``exact`` (regrets against the prefix's exact
        comparator), ``cum_ftrl``, ``cum_exact``, ``comp``, ``in_regime`` and ``closed`` (int32;
        closed: both comparator losses in closed form); with ``with_ftl_comparator`` also
        ``comp_ftl``, with ``with_actions`` ``action`` [B, K, d].  Column k is what
        ftrl_vs_exact gives on the batch truncated at t_k, bit for bit in the same layout;
        ``closed_comparator`` and the butterfly sums default as there.  A pair outside the
        regime (``in_regime`` 0) keeps the closed form's numbers, as ftrl_vs_exact does:
        ftrl_vs_exact_curve_general fills those."""
        torch = self.torch
        code = _norm_code(norm)
        ck = _checkpoints(checkpoints, self.L.T)
        K, B, d = int(ck.size), int(self.L.B), int(self.L.d)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0
        if self.best and self.L.chain:
            flags |= _lib.OCX_ALG_TREE_SUMS  # as ftrl_vs_exact
        nbytes = int(_lib.load().ocx_ftrl_exact_curve_workspace_bytes(
            self._lp(), K, int(bool(with_ftl_comparator))))
        if nbytes < 0:
            _lib.check(nbytes, "ocx_ftrl_exact_curve_workspace_bytes")
        with torch.cuda.device(self.device), self._on_stream():
            ckd = torch.as_tensor(ck).to(self.device)
            out = {k: torch.zeros((B, K), dtype=torch.float64, device=self.device)
                   for k in ("cum_ftrl", "cum_exact", "comp")}
            if with_ftl_comparator:
                out["comp_ftl"] = torch.zeros((B, K), dtype=torch.float64, device=self.device)
            if with_actions:
                out["action"] = torch.zeros((B, K, d), dtype=torch.float64, device=self.device)
            for k in ("in_regime", "closed"):
                out[k] = torch.zeros((B, K), dtype=torch.int32, device=self.device)
            ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        if K and B:
            self._call("ocx_dev_ftrl_vs_exact_curve", self._lp(), self.z.data_ptr(),
                       self._y.data_ptr(), float(eta0), ckd.data_ptr(), K,
                       out["cum_ftrl"].data_ptr(), out["cum_exact"].data_ptr(),
                       out["comp"].data_ptr(),
                       out["comp_ftl"].data_ptr() if with_ftl_comparator else None,
                       out["action"].data_ptr() if with_actions else None,
                       out["in_regime"].data_ptr(), out["closed"].data_ptr(), code, flags,
                       ws.data_ptr(), ws.numel() * 8, self._sp)
        with self._on_stream():
            out["ftrl"] = out["cum_ftrl"] - out["comp"]
            out["exact"] = out["cum_exact"] - out["comp"]
        self._keep_exact_curve = self._hold(ckd, ws)
        return out

    def ftrl_vs_exact_curve_general(self, checkpoints, eta0: float = SQRT2, *, norm: str = "l2",
                                    closed_comparator: Optional[bool] = None,
                                    with_ftl_comparator: bool = False,
                                    with_actions: bool = False):
        """ftrl_vs_exact_curve with every pair's exact side valid: the pairs with
        ``in_regime`` 0 get the general solver's numbers — ONE exact_ball_solve-style call over
        all prefixes up to the largest checkpoint, for the sequences with any such pair:
        cum_exact[b, k] = cumsum(step_loss)[t_k - 1] (0 at t_k = 0), comp[b, k] = obj[b, t_k],
        action = actions[b, t_k]; a prefix still in the regime keeps its closed form, as a
        truncated call would.  Certificates are checked (check_certificates; the worst gap is
        left in self.exact_gap_max).  Synchronises once."""
        torch = self.torch
        out = self.ftrl_vs_exact_curve(checkpoints, eta0, norm=norm,
                                       closed_comparator=closed_comparator,
                                       with_ftl_comparator=with_ftl_comparator,
                                       with_actions=with_actions)
        ck = _checkpoints(checkpoints, self.L.T)
        K, d = int(ck.size), int(self.L.d)
        self.exact_gap_max = 0.0
        if K == 0 or self.L.B == 0:
            return out
        self._general_curve_fill(out, ck, norm, with_actions)
        with self._on_stream():
            out["ftrl"] = out["cum_ftrl"] - out["comp"]
            out["exact"] = out["cum_exact"] - out["comp"]
        return out

    def _general_curve_fill(self, out, ck, norm: str, with_actions: bool):
        """The general solver's numbers for the pairs of an exact curve or grid with
        ``in_regime`` 0 (ftrl_vs_exact_curve_general): cum_exact, comp and action of ``out``
        in place, the worst certified gap in self.exact_gap_max.  One solve over all prefixes
        up to ck[-1] of the sequences with any such pair; none when every pair is in the
        regime."""
        torch = self.torch
        d = int(self.L.d)
        with self._on_stream():
            out_of = out["in_regime"] == 0                  # [B, K]
            if not bool(out_of.any().item()):
                return
            bad = torch.nonzero(out_of.any(dim=1)).flatten()
            nb, Tm = int(bad.numel()), int(ck[-1])
            zb, yb = tiled_rows(self.z, self._y, self.L, bad)  # read only: the bits stay valid
            zb, yb = zb[:, :Tm].contiguous(), yb[:, :Tm].contiguous()
            res = {"actions": torch.zeros((nb, Tm + 1, d), dtype=torch.float64,
                                          device=self.device)}
            for k in ("obj", "gap", "step_loss"):
                res[k] = torch.zeros((nb, Tm + 1), dtype=torch.float64, device=self.device)
            res["info"] = torch.zeros((nb, Tm + 1), dtype=torch.int32, device=self.device)
            self._call("ocx_dev_exact_ball_solve", zb.data_ptr(), yb.data_ptr(), nb, Tm, d,
                       _norm_code(norm), 1, res["actions"].data_ptr(), res["obj"].data_ptr(),
                       res["gap"].data_ptr(), res["step_loss"].data_ptr(),
                       res["info"].data_ptr(), self._sp)
            self._hold(zb, yb)
            host = {k: res[k].cpu().numpy() for k in ("obj", "gap", "info", "step_loss")}
            self.exact_gap_max = check_certificates(host["obj"], host["gap"], host["info"])
            gcum, gcomp = _general_curve_columns(host["step_loss"], host["obj"], ck)
            m = out_of[bad]                                 # [nb, K]: only these pairs change
            ckd = torch.as_tensor(ck).to(self.device)
            new_cum = torch.as_tensor(gcum).to(self.device)
            new_comp = torch.as_tensor(gcomp).to(self.device)
            out["cum_exact"][bad] = torch.where(m, new_cum, out["cum_exact"][bad])
            out["comp"][bad] = torch.where(m, new_comp, out["comp"][bad])
            if with_actions:
                acts = res["actions"][:, ckd, :]            # [nb, K, d]
                out["action"][bad] = torch.where(m[:, :, None], acts, out["action"][bad])

    def ftrl_vs_exact_curve_etas(self, checkpoints, etas, *, norm: str = "l2",
                                 closed_comparator: Optional[bool] = None,
                                 with_ftl_comparator: bool = False, with_actions: bool = False,
                                 _group=None):
        """FTRL-vs-exact-FTL regret grid of the resident batch (ocx_dev_ftrl_vs_exact_curve_etas,
        async): ftrl_vs_exact_curve for every eta0 of ``etas`` (validated as in
        simulate_alg_etas), each pass over z serving ocx_ftrl_exact_grid_group(L) FTRL columns
        beside ONE exact-FTL column.  Returns a dict of device tensors: ``ftrl`` and
        ``cum_ftrl`` [B, M, K] (with ``with_ftl_comparator`` also ``comp_ftl``), and ``exact``,
        ``cum_exact``, ``comp``, ``in_regime``, ``closed`` [B, K] (with ``with_actions`` also
        ``action`` [B, K, d]), which do not depend on the step size.  [:, m, :] and the [B, K]
        tensors are ftrl_vs_exact_curve(checkpoints, etas[m], ...) bit for bit in the same
        layout; the other arguments default as there.  (``_group`` forces the columns per pass:
        1, 2 or 4 where the layout has that instance; the results do not depend on it.)"""
        torch = self.torch
        code = _norm_code(norm)
        ck = _checkpoints(checkpoints, self.L.T)
        et = _etas(etas)
        K, M, B, d = int(ck.size), int(et.size), int(self.L.B), int(self.L.d)
        if closed_comparator is None:
            closed_comparator = not self.exact
        flags = _lib.OCX_ALG_CLOSED_COMPARATOR if closed_comparator else 0
        if self.best and self.L.chain:
            flags |= _lib.OCX_ALG_TREE_SUMS  # as ftrl_vs_exact
        nbytes = int(_lib.load().ocx_ftrl_exact_grid_workspace_bytes(
            self._lp(), M, K, int(bool(with_ftl_comparator))))
        if nbytes < 0:
            _lib.check(nbytes, "ocx_ftrl_exact_grid_workspace_bytes")
        with torch.cuda.device(self.device), self._on_stream():
            ckd = torch.as_tensor(ck).to(self.device)
            out = {"cum_ftrl": torch.zeros((B, M, K), dtype=torch.float64, device=self.device)}
            for k in ("cum_exact", "comp"):
                out[k] = torch.zeros((B, K), dtype=torch.float64, device=self.device)
            if with_ftl_comparator:
                out["comp_ftl"] = torch.zeros((B, M, K), dtype=torch.float64, device=self.device)
            if with_actions:
                out["action"] = torch.zeros((B, K, d), dtype=torch.float64, device=self.device)
            for k in ("in_regime", "closed"):
                out[k] = torch.zeros((B, K), dtype=torch.int32, device=self.device)
            ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=self.device)
        if K and B and M:
            self._call("ocx_dev_ftrl_vs_exact_curve_etas", self._lp(), self.z.data_ptr(),
                       self._y.data_ptr(), ptr(et), M, ckd.data_ptr(), K,
                       out["cum_ftrl"].data_ptr(), out["cum_exact"].data_ptr(),
                       out["comp"].data_ptr(),
                       out["comp_ftl"].data_ptr() if with_ftl_comparator else None,
                       out["action"].data_ptr() if with_actions else None,
                       out["in_regime"].data_ptr(), out["closed"].data_ptr(), code, flags,
                       0 if _group is None else int(_group), ws.data_ptr(), ws.numel() * 8,
                       self._sp)
        with self._on_stream():
            out["ftrl"] = out["cum_ftrl"] - out["comp"][:, None, :]
            out["exact"] = out["cum_exact"] - out["comp"]
        self._keep_exact_grid = self._hold(ckd, ws)
        return out

    def ftrl_vs_exact_curve_etas_general(self, checkpoints, etas, *, norm: str = "l2",
                                         closed_comparator: Optional[bool] = None,
                                         with_ftl_comparator: bool = False,
                                         with_actions: bool = False, _group=None):
        """ftrl_vs_exact_curve_etas with every pair's exact side valid, as
        ftrl_vs_exact_curve_general: the pairs with ``in_regime`` 0 get the general solver's
        cum_exact / comp / action — ONE solve over all prefixes up to the largest checkpoint for
        the sequences with any such pair, whatever M is — and ``ftrl`` (every step size) and
        ``exact`` are taken again.  [:, m, :] is ftrl_vs_exact_curve_general(checkpoints,
        etas[m], ...).  Certificates are checked (the worst gap is left in self.exact_gap_max).
        Synchronises once."""
        out = self.ftrl_vs_exact_curve_etas(checkpoints, etas, norm=norm,
                                            closed_comparator=closed_comparator,
                                            with_ftl_comparator=with_ftl_comparator,
                                            with_actions=with_actions, _group=_group)
        self.exact_gap_max = 0.0
        if out["cum_ftrl"].numel() == 0:
            return out
        self._general_curve_fill(out, _checkpoints(checkpoints, self.L.T), norm, with_actions)
        with self._on_stream():
            out["ftrl"] = out["cum_ftrl"] - out["comp"][:, None, :]
            out["exact"] = out["cum_exact"] - out["comp"]
        return out

    def ftrl_vs_exact_etas(self, etas, *, norm: str = "l2",
                           closed_comparator: Optional[bool] = None,
                           with_ftl_comparator: bool = False, with_actions: bool = False,
                           _group=None):
        """Step-size sweep of ftrl_vs_exact on the resident batch: the grid at checkpoints = [T]
        with the horizon axis dropped (the same kernel).  ``ftrl``, ``cum_ftrl`` (``comp_ftl``)
        [B, M]; ``exact``, ``cum_exact``, ``comp``, ``in_regime``, ``closed`` [B] (``action``
        [B, d]); column m is ftrl_vs_exact(etas[m]) bit for bit."""
        out = self.ftrl_vs_exact_curve_etas([self.L.T], etas, norm=norm,
                                            closed_comparator=closed_comparator,
                                            with_ftl_comparator=with_ftl_comparator,
                                            with_actions=with_actions, _group=_group)
        three = ("ftrl", "cum_ftrl", "comp_ftl")
        return {k: (v[:, :, 0] if k in three else v[:, 0]) for k, v in out.items()}

    def exact_comparison_curves(self, checkpoints, eta0: float = SQRT2, norm: str = "l2"):
        """The two lines of the reference's exact comparison figure (exact_ftl_driver.py:
        157-190) against the horizon, from this resident batch: ``FTRL`` and ``FTL (exact)``,
        each a [B, K] device tensor — the regrets of ftrl_vs_exact_curve, the counterpart of
        comparison_curves.  Column k is the regret on the batch truncated at t_k."""
        out = self.ftrl_vs_exact_curve(checkpoints, eta0, norm=norm)
        return {"FTRL": out["ftrl"], "FTL (exact)": out["exact"]}

    def rows_of(self, seqs):
        """z [n, T, d] and y [n, T] (device, row-major, contiguous) of the sequences ``seqs``
        (device int64 tensor of batch indices), gathered out of the tiled layout
        (tiled_rows).  It reads ``y`` through the public name, as any caller from outside
        does, so the label bits turn invalid; the batch's own methods gather from the private
        tensor (tiled_rows(self.z, self._y, ...)) and keep them."""
        return tiled_rows(self.z, self.y, self.L, seqs)

    def generate_simulate(self, base_seed: int = 0, run0: int = 0, nbatch: int = 1,
                          eta0: float = SQRT2, gmax=None, pipelined: bool = True,
                          sub_seqs: int = 0):
        """fast_algorithms.py:230-247's loop over ``nbatch`` resident batches in one call
        (ocx_dev_gen_simulate): batch k holds runs run0 + k*B .. run0 + (k+1)*B - 1,
        generated on device into this batch's z/y and simulated by FTRL.  self.regret gets
        the last batch's regrets; ``gmax`` ([1] float64 device tensor, optional) the max over
        every batch, from 0.0.  ``pipelined`` overlaps generation of one sub-batch with the
        FTRL pass over the previous one (d = 64, 8 x 8 / 16 x 4 butterfly layouts; otherwise,
        or with False, batch by batch).  The closed-form comparator is taken as in
        simulate_alg (the bit-exact layouts keep the streamed pass).  Same regrets either way,
        bit for bit."""
        flags = 0 if pipelined else _lib.OCX_GENSIM_SEQUENTIAL
        if self.exact:
            flags |= _lib.OCX_GENSIM_TWO_PASS
        if nbatch > 0:
            # each batch is read once, by FTRL kernels that keep y's doubles beside the
            # generator: the tile is not written, so it no longer describes y
            self._bits_state = "invalid"
        self._call("ocx_dev_gen_simulate", self._lp(), int(base_seed), int(run0), int(nbatch),
                  self.z.data_ptr(), self._y.data_ptr(), float(eta0), self.regret.data_ptr(),
                  gmax.data_ptr() if gmax is not None else None, flags, int(sub_seqs), self._sp)
        self.rows_clipped = True
        return self.regret

    def max_regret(self, out=None):
        torch = self.torch
        if out is None:
            with self._on_stream():
                out = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._call("ocx_dev_max_regret", self.regret.data_ptr(), int(self.L.B), out.data_ptr(),
                  self._sp)
        return out

    @property
    def z_bytes(self) -> int:
        return int(self.L.z_elems) * 8

    @property
    def y_bytes(self) -> int:
        return int(self.L.y_elems) * 8


# HBM that gT_regret_curves' default batch keeps resident: z, y and the curve workspace
GT_CURVE_HBM_BUDGET = 64 << 30


def gT_regret_curves(T: int, runs: int, checkpoints, *, base_seed: int = 0, d: int = 5,
                     eta0: float = SQRT2, run0: int = 0, lanes_per_seq: int = LANES_BEST,
                     device: int = 0, batch: Optional[int] = None, return_closed: bool = False):
    """Regret-against-horizon curves of FTRL on the g(T) sampler: the sequences
    _rng(base_seed, T, run), run in [run0, run0 + runs) (fast_algorithms.py:230-241 at horizon
    T, with a ``d`` parameter), observed at every horizon of ``checkpoints``.  Returns
    regret [runs, K] (and closed [runs, K] int32 with ``return_closed``).

    Generated on device (DeviceBatch.generate_gT) and simulated once (simulate_alg_curve) in
    batches of ``batch`` sequences — by default as many as keep z, y and the curve workspace
    under GT_CURVE_HBM_BUDGET bytes; a short last batch is handled.  The library's cached
    buffers are released first.  Only the [runs, K] result crosses PCIe."""
    import torch
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    T, runs = int(T), int(runs)
    if runs < 0:
        raise ValueError("runs must be >= 0")
    ck = _checkpoints(checkpoints, T)
    K = int(ck.size)
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    if runs == 0 or K == 0:
        empty = np.zeros((runs, K))
        return (empty, np.zeros((runs, K), dtype=np.int32)) if return_closed else empty
    release_buffers(device)
    if batch is None:
        L = _lib.layout(runs, T, d, lanes_per_seq)  # bytes per wave-group of S sequences
        per_group = 8 * (L.z_elems + L.y_elems) // L.G + 64 * K * (8 * L.C + 12)
        batch = max(1, GT_CURVE_HBM_BUDGET // max(per_group, 1)) * L.S
    batch = min(int(batch), runs)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        reg = torch.empty((runs, K), dtype=torch.float64, device=dev)
        closed = torch.empty((runs, K), dtype=torch.int32, device=dev) if return_closed else None
        db = None
        for r0 in range(0, runs, batch):
            n = min(batch, runs - r0)
            if db is None or db.L.B != n:
                db = None  # the short last batch: free the full one first
                db = DeviceBatch(n, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
            db.generate_gT(base_seed, int(run0) + r0)
            res = db.simulate_alg_curve(ck, 0, eta0)
            with db._on_stream():
                reg[r0:r0 + n].copy_(res["regret"])
                if closed is not None:
                    closed[r0:r0 + n].copy_(res["closed"])
        with db._on_stream():
            out = reg.cpu().numpy()
            cl = closed.cpu().numpy() if closed is not None else None
    return (out, cl) if return_closed else out


def _gT_anytime_batches(T, runs, ck, base_seed, d, eta0, run0, lanes_per_seq, device, batch, each):
    """The batch loop of gT_anytime and gT_anytime_max: every batch of the g(T) sampler's
    sequences generated on device and observed at every step (simulate_alg_anytime);
    ``each(db, r0, n, res)`` receives the batch's device results.  ``batch`` None: as many
    sequences as keep z and y under GT_CURVE_HBM_BUDGET bytes (the anytime kernel has no
    workspace).  Returns the last DeviceBatch (its stream orders the results)."""
    release_buffers(device)
    if batch is None:
        L = _lib.layout(runs, T, d, lanes_per_seq)  # bytes per wave-group of S sequences
        per_group = 8 * (L.z_elems + L.y_elems) // L.G
        batch = max(1, GT_CURVE_HBM_BUDGET // max(per_group, 1)) * L.S
    batch = min(int(batch), runs)
    db = None
    for r0 in range(0, runs, batch):
        n = min(batch, runs - r0)
        if db is None or db.L.B != n:
            db = None  # the short last batch: free the full one first
            db = DeviceBatch(n, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
        db.generate_gT(base_seed, int(run0) + r0)
        each(db, r0, n, db.simulate_alg_anytime(ck, 0, eta0))
    return db


def _gT_anytime_args(T, runs, checkpoints, base_seed, batch):
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    T, runs = int(T), int(runs)
    if runs < 0:
        raise ValueError("runs must be >= 0")
    ck = _anytime_checkpoints(checkpoints, T)
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    return T, runs, ck


def gT_anytime(T: int, runs: int, checkpoints=None, *, base_seed: int = 0, d: int = 5,
               eta0: float = SQRT2, run0: int = 0, lanes_per_seq: int = LANES_BEST,
               device: int = 0, batch: Optional[int] = None):
    """FTRL's anytime regret on the g(T) sampler: for the sequences _rng(base_seed, T, run),
    run in [run0, run0 + runs) (the rows gT_regret_curves observes), ``sup`` [runs, K] — the
    largest regret any prefix of at most t_k steps reached — and ``argsup`` [runs, K] int64, the
    first step at which it was reached.  ``checkpoints`` defaults to [T].  sup[:, k] bounds
    gT_regret_curves(...)[:, k] from above and is non-decreasing in k.

    Generated on device and observed at every step in one pass (simulate_alg_anytime), in
    batches of ``batch`` sequences — by default as many as keep z and y under
    GT_CURVE_HBM_BUDGET bytes; a short last batch is handled.  Only the two [runs, K] results
    cross PCIe."""
    import torch
    T, runs, ck = _gT_anytime_args(T, runs, checkpoints, base_seed, batch)
    K = int(ck.size)
    if runs == 0 or K == 0:
        return np.zeros((runs, K)), np.zeros((runs, K), dtype=np.int64)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        sup = torch.empty((runs, K), dtype=torch.float64, device=dev)
        arg = torch.empty((runs, K), dtype=torch.int64, device=dev)

        def each(db, r0, n, res):
            with db._on_stream():
                sup[r0:r0 + n].copy_(res["sup"])
                arg[r0:r0 + n].copy_(res["argsup"])

        db = _gT_anytime_batches(T, runs, ck, base_seed, d, eta0, run0, lanes_per_seq, device,
                                 batch, each)
        with db._on_stream():
            return sup.cpu().numpy(), arg.cpu().numpy()


def gT_anytime_max(T: int, runs: int, checkpoints=None, *, base_seed: int = 0, d: int = 5,
                   eta0: float = SQRT2, run0: int = 0, lanes_per_seq: int = LANES_BEST,
                   device: int = 0, batch: Optional[int] = None):
    """g[K] = max(0, max over runs of gT_anytime(...)[0][:, k]): the anytime envelope of g(T) —
    the largest regret FTRL reached at ANY step t <= t_k over the g(T) sampler's runs —
    reduced on device batch by batch (ocx_dev_max_regret_cols); only K doubles cross PCIe.
    Non-decreasing in k, and >= the checkpoint envelope gT_surface reads at the same t_k."""
    import torch
    T, runs, ck = _gT_anytime_args(T, runs, checkpoints, base_seed, batch)
    K = int(ck.size)
    if runs == 0 or K == 0:
        return np.zeros(K)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        g = torch.zeros(K, dtype=torch.float64, device=dev)

        def each(db, r0, n, res):
            db._call("ocx_dev_max_regret_cols", res["sup"].data_ptr(), n, K, g.data_ptr(),
                     1 if r0 else 0, db._sp)
            db._hold(res["sup"], g)

        db = _gT_anytime_batches(T, runs, ck, base_seed, d, eta0, run0, lanes_per_seq, device,
                                 batch, each)
        with db._on_stream():
            return g.cpu().numpy()


def gT_regrets_etas(T: int, runs: int, etas, *, base_seed: int = 0, d: int = 5, run0: int = 0,
                    lanes_per_seq: int = LANES_BEST, device: int = 0,
                    batch: Optional[int] = None, return_closed: bool = False):
    """FTRL's regrets on the g(T) sampler for every eta0 of ``etas``: the sequences
    _rng(base_seed, T, run), run in [run0, run0 + runs) (fast_algorithms.py:230-241 with a
    ``d`` parameter).  Returns regret [runs, M] (and closed [runs, M] int32 with
    ``return_closed``); column m is gT_regrets(..., eta0=etas[m]).

    Each batch is generated once on device (DeviceBatch.generate_gT) and simulated for all M
    step sizes (simulate_alg_etas), in batches of ``batch`` sequences — by default as many as
    keep z and y under GT_CURVE_HBM_BUDGET bytes; a short last batch is handled.  The
    library's cached buffers are released first.  Only the [runs, M] result crosses PCIe."""
    import torch
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    T, runs = int(T), int(runs)
    if runs < 0:
        raise ValueError("runs must be >= 0")
    et = _etas(etas)
    M = int(et.size)
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    if runs == 0 or M == 0:
        empty = np.zeros((runs, M))
        return (empty, np.zeros((runs, M), dtype=np.int32)) if return_closed else empty
    release_buffers(device)
    if batch is None:
        L = _lib.layout(runs, T, d, lanes_per_seq)  # bytes per wave-group of S sequences
        per_group = 8 * (L.z_elems + L.y_elems) // L.G
        batch = max(1, GT_CURVE_HBM_BUDGET // max(per_group, 1)) * L.S
    batch = min(int(batch), runs)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        reg = torch.empty((runs, M), dtype=torch.float64, device=dev)
        closed = torch.empty((runs, M), dtype=torch.int32, device=dev) if return_closed else None
        db = None
        for r0 in range(0, runs, batch):
            n = min(batch, runs - r0)
            if db is None or db.L.B != n:
                db = None  # the short last batch: free the full one first
                db = DeviceBatch(n, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
            db.generate_gT(base_seed, int(run0) + r0)
            res = db.simulate_alg_etas(et)
            with db._on_stream():
                reg[r0:r0 + n].copy_(res["regret"])
                if closed is not None:
                    closed[r0:r0 + n].copy_(res["closed"])
        with db._on_stream():
            out = reg.cpu().numpy()
            cl = closed.cpu().numpy() if closed is not None else None
    return (out, cl) if return_closed else out


def _gT_grid_batches(T, runs, ck, et, base_seed, d, run0, lanes_per_seq, device, batch, each):
    """The batch loop of gT_regret_curves_etas and gT_surface: every batch of the g(T)
    sampler's sequences generated once (DeviceBatch.generate_gT) and simulated for every step
    size and horizon (simulate_alg_curve_etas); ``each(db, r0, n, res)`` receives the batch's
    device results.  ``batch`` None: as many sequences as keep z, y and the grid workspace
    under GT_CURVE_HBM_BUDGET bytes.  Returns the last DeviceBatch (its stream orders the
    results)."""
    K, M = int(ck.size), int(et.size)
    release_buffers(device)
    if batch is None:
        L = _lib.layout(runs, T, d, lanes_per_seq)  # bytes per wave-group of S sequences
        ne = min(max(int(_lib.load().ocx_curve_etas_group(ctypes.byref(L), M)), 1), M)
        per_group = 8 * (L.z_elems + L.y_elems) // L.G + 64 * K * ne * (8 * L.C + 12)
        batch = max(1, GT_CURVE_HBM_BUDGET // max(per_group, 1)) * L.S
    batch = min(int(batch), runs)
    db = None
    for r0 in range(0, runs, batch):
        n = min(batch, runs - r0)
        if db is None or db.L.B != n:
            db = None  # the short last batch: free the full one first
            db = DeviceBatch(n, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
        db.generate_gT(base_seed, int(run0) + r0)
        each(db, r0, n, db.simulate_alg_curve_etas(ck, et))
    return db


def _gT_grid_args(T, runs, checkpoints, etas, base_seed, batch):
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    T, runs = int(T), int(runs)
    if runs < 0:
        raise ValueError("runs must be >= 0")
    ck = _checkpoints(checkpoints, T)
    et = _etas(etas)
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    return T, runs, ck, et


def gT_regret_curves_etas(T: int, runs: int, checkpoints, etas, *, base_seed: int = 0,
                          d: int = 5, run0: int = 0, lanes_per_seq: int = LANES_BEST,
                          device: int = 0, batch: Optional[int] = None,
                          return_closed: bool = False):
    """FTRL's regret grid on the g(T) sampler: the sequences _rng(base_seed, T, run), run in
    [run0, run0 + runs) (fast_algorithms.py:230-241 at horizon T, with a ``d`` parameter), for
    every eta0 of ``etas`` observed at every horizon of ``checkpoints``.  Returns regret
    [runs, M, K] (and closed [runs, M, K] int32 with ``return_closed``); [:, m, :] is
    gT_regret_curves(..., eta0=etas[m]) and, with t_K = T, [:, :, -1] is gT_regrets_etas.

    Each batch is generated once on device and simulated for every step size and horizon
    (simulate_alg_curve_etas), in batches of ``batch`` sequences — by default as many as keep
    z, y and the grid workspace under GT_CURVE_HBM_BUDGET bytes; a short last batch is
    handled.  The library's cached buffers are released first.  Only the [runs, M, K] result
    crosses PCIe."""
    import torch
    T, runs, ck, et = _gT_grid_args(T, runs, checkpoints, etas, base_seed, batch)
    K, M = int(ck.size), int(et.size)
    if runs == 0 or K == 0 or M == 0:
        empty = np.zeros((runs, M, K))
        return (empty, np.zeros((runs, M, K), dtype=np.int32)) if return_closed else empty
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        reg = torch.empty((runs, M, K), dtype=torch.float64, device=dev)
        closed = (torch.empty((runs, M, K), dtype=torch.int32, device=dev)
                  if return_closed else None)

        def each(db, r0, n, res):
            with db._on_stream():
                reg[r0:r0 + n].copy_(res["regret"])
                if closed is not None:
                    closed[r0:r0 + n].copy_(res["closed"])

        db = _gT_grid_batches(T, runs, ck, et, base_seed, d, run0, lanes_per_seq, device, batch,
                              each)
        with db._on_stream():
            out = reg.cpu().numpy()
            cl = closed.cpu().numpy() if closed is not None else None
    return (out, cl) if return_closed else out


def gT_surface(T: int, runs: int, checkpoints, etas, *, base_seed: int = 0, d: int = 5,
               run0: int = 0, lanes_per_seq: int = LANES_BEST, device: int = 0,
               batch: Optional[int] = None):
    """g[M, K] = max(0, max over runs of gT_regret_curves_etas(...)[:, m, k]): the largest
    regret of FTRL with eta0 = etas[m] at horizon t_k over the g(T) sampler's runs, reduced on
    device batch by batch (ocx_dev_max_regret_cols); only M·K doubles cross PCIe.

    What it is: the ANYTIME regret on the longest horizon's rows — every horizon of
    ``checkpoints`` is read off the same sequences _rng(base_seed, T, run).  It is not the
    reference's g(T) at T = t_k, which draws a fresh sequence per T (the generator is seeded
    with the horizon); column K-1 at t_K = T is gT_max(T, runs, eta0=etas[m])."""
    import torch
    T, runs, ck, et = _gT_grid_args(T, runs, checkpoints, etas, base_seed, batch)
    K, M = int(ck.size), int(et.size)
    if runs == 0 or K == 0 or M == 0:
        return np.zeros((M, K))
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        g = torch.zeros((M, K), dtype=torch.float64, device=dev)

        def each(db, r0, n, res):
            db._call("ocx_dev_max_regret_cols", res["regret"].data_ptr(), n, M * K,
                     g.data_ptr(), 1 if r0 else 0, db._sp)
            db._hold(res["regret"], g)

        db = _gT_grid_batches(T, runs, ck, et, base_seed, d, run0, lanes_per_seq, device, batch,
                              each)
        with db._on_stream():
            out = g.cpu().numpy()
    return out


def gT_smart_grids(T: int, runs: int, checkpoints, thresholds, *, base_seed: int = 0,
                   d: int = 5, eta0: float = SQRT2, run0: int = 0,
                   lanes_per_seq: int = LANES_BEST, device: int = 0,
                   batch: Optional[int] = None, return_switch: bool = False):
    """SMART's regret grid on the g(T) sampler: the sequences _rng(base_seed, T, run), run in
    [run0, run0 + runs) (fast_algorithms.py:230-241 at horizon T, with a ``d`` parameter), for
    every switch threshold of ``thresholds`` ([M]: every run the same) observed at every
    horizon of ``checkpoints``.  Returns regret [runs, M, K] (and switch_step [runs, M, K]
    int64 with ``return_switch``); [:, m, :] is SMART with thresholds[m] on the first t_k rows
    of every run.

    What it is: the ANYTIME regret on the longest horizon's rows — every horizon of
    ``checkpoints`` is read off the same sequences.  It is not SMART on the reference's g(T)
    sequences at T = t_k, which are drawn afresh per T.

    Each batch is generated once on device (DeviceBatch.generate_gT) and simulated for every
    threshold and horizon (simulate_smart_grid), in batches of ``batch`` sequences — by
    default as many as keep z and y under GT_CURVE_HBM_BUDGET bytes; a short last batch is
    handled.  The library's cached buffers are released first.  The result does not depend on
    ``batch``.  Only the [runs, M, K] results cross PCIe."""
    import torch
    if base_seed < 0 or base_seed >= 2 ** 64:
        raise ValueError("base_seed must be in [0, 2**64)")
    T, runs = int(T), int(runs)
    if runs < 0:
        raise ValueError("runs must be >= 0")
    ck = _checkpoints(checkpoints, T)
    th = np.asarray(_thresholds(thresholds, 1))
    if np.asarray(thresholds).ndim != 1:
        raise ValueError("thresholds must be [M]: one list for every run")
    th = th[0]
    if batch is not None and int(batch) < 1:
        raise ValueError("batch must be >= 1")
    K, M = int(ck.size), int(th.size)
    if runs == 0 or K == 0 or M == 0:
        empty = np.zeros((runs, M, K))
        return (empty, np.full((runs, M, K), -1, dtype=np.int64)) if return_switch else empty
    release_buffers(device)
    if batch is None:
        L = _lib.layout(runs, T, d, lanes_per_seq)  # bytes per wave-group of S sequences
        per_group = 8 * (L.z_elems + L.y_elems) // L.G
        batch = max(1, GT_CURVE_HBM_BUDGET // max(per_group, 1)) * L.S
    batch = min(int(batch), runs)
    dev = torch.device("cuda", int(device))
    with torch.cuda.device(dev):
        reg = torch.empty((runs, M, K), dtype=torch.float64, device=dev)
        sw = torch.empty((runs, M, K), dtype=torch.int64, device=dev) if return_switch else None
        db = None
        for r0 in range(0, runs, batch):
            n = min(batch, runs - r0)
            if db is None or db.L.B != n:
                db = None  # the short last batch: free the full one first
                db = DeviceBatch(n, T, d, lanes_per_seq=lanes_per_seq, device=int(device))
            db.generate_gT(base_seed, int(run0) + r0)
            res = db.simulate_smart_grid(ck, th, eta0)
            with db._on_stream():
                reg[r0:r0 + n].copy_(res["regret"])
                if sw is not None:
                    sw[r0:r0 + n].copy_(res["switch_step"])
        with db._on_stream():
            out = reg.cpu().numpy()
            so = sw.cpu().numpy() if sw is not None else None
    return (out, so) if return_switch else out
