"""The label-bit tile (include/ocx.h): its producers (the g(T) generator, pack) against the
NumPy reference built from y_tiled, and its consumer — the persistent instance of the pipelined
FTRL / FTL step, which reads labels as bits; reached at small sizes through the forced-waves
test entry — against the float64 path on the same resident batch, bit for bit: regret, cum,
comp and the closed flags.  Through DeviceBatch.simulate_alg none of these small batches reaches
that instance (it takes more wave-groups than one round holds: the bench batch, whose dumped
regrets are compared with the parent's); they launch a form that keeps y's doubles, so those
comparisons pin the plumbing and the fallback.  The float64 path of a DeviceBatch is reached by
reading ``db.y`` (which marks the bits invalid) or through the entry points without a bit
tile."""
import ctypes
import math

import numpy as np
import pytest

from tests import _label_bits as LB

pytestmark = pytest.mark.gpu

SQ2 = math.sqrt(2)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    assert _lib.device_count() >= 1
    return engine


def bits_of(db) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return db._ybits.cpu().numpy().view(np.uint64)[:LB.words(db.L)]


def ytiled_of(db) -> np.ndarray:
    import torch
    torch.cuda.synchronize()
    return db._y.cpu().numpy()[:db.L.y_elems]


def same_bits(got, want):
    return all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              w.view(np.uint64) if w.dtype == np.float64 else w)
               for g, w in zip(got, want))


def simulate(db, ftl, closed):
    """DeviceBatch.simulate_alg's (regret, cum, comp, closed_out) as host arrays."""
    import torch
    flags = torch.full((db.L.B,), 7, dtype=torch.int32, device=db.device)
    db.simulate_alg(ftl, SQ2, closed_comparator=bool(closed), closed_out=flags)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (db.regret, db.cum, db.comp, flags))


def both_paths(db, ftl, closed):
    """(from bits, from float64) on the batch as it stands; the bits must be valid before."""
    assert db.label_bits_valid
    with_bits = simulate(db, ftl, closed)
    saved = db._bits_state
    _ = db.y  # any outside access marks the bits invalid: the float64 path
    assert not db.label_bits_valid
    without = simulate(db, ftl, closed)
    db._bits_state = saved  # nothing was written: the tile still describes y
    return with_bits, without


# ------------------------------------------------------------------ producers
@pytest.mark.parametrize("B", [1, 8, 24, 2048 + 3])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_generator_bits_equal_y_tiled(eng, T, B):
    """d = 64: the words equal y_tiled == 1.0 word for word — a partial last block, a partial
    group and padding sequences (bits 0) included — and y_tiled holds ±1 / 0 as before."""
    db = eng.DeviceBatch(B, T, 64).generate_gT(base_seed=5, run0=3)
    assert db.label_bits_valid
    yt = ytiled_of(db)
    got, want = bits_of(db), LB.tile_from_tiled(yt, db.L)
    assert np.array_equal(got, want), int((got != want).sum())
    live = LB.rows_from_tile(got, db.L)
    from tests._tiles import untile_y
    assert np.array_equal(live, untile_y(yt, db.L))  # every live label is ±1 and is its bit


@pytest.mark.parametrize("form", ["lr", "default"])
def test_generator_bits_in_both_forms(eng, monkeypatch, form):
    """The few-stream and the default generator form (OCX_GEN_FORM), a partial group."""
    monkeypatch.setenv("OCX_GEN_FORM", form)
    db = eng.DeviceBatch(2048 + 3, 130, 64).generate_gT(base_seed=1, run0=0)
    assert np.array_equal(bits_of(db), LB.tile_from_tiled(ytiled_of(db), db.L))


@pytest.mark.parametrize("P", [8, 16])
def test_pack_bits_equal_y_tiled(eng, P):
    rng = np.random.default_rng(P)
    B, T = 27, 130
    z = rng.standard_normal((B, T, 64)) / 9.0
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=P).pack(z, y)
    assert (db.L.P, db.L.C) == (P, 64 // P)
    assert db.label_bits_valid
    got = bits_of(db)
    assert np.array_equal(got, LB.tile_from_tiled(ytiled_of(db), db.L))
    assert np.array_equal(got, LB.tile_from_rows(y, db.L))


# ------------------------------------------------------------------ consumer: the product call
@pytest.fixture(scope="module", params=[65, 130])
def gt88(request, eng):
    T = request.param
    # G = 8, the last group 3 live + 5 padding sequences
    db = eng.DeviceBatch(59, T, 64, lanes_per_seq=8).generate_gT(base_seed=11, run0=2)
    assert (db.L.P, db.L.C, db.L.G, db.L.chain) == (8, 8, 8, 0)
    return db


@pytest.mark.parametrize("closed", [0, 1])
@pytest.mark.parametrize("ftl", [0, 1])
def test_simulate_from_bits_equals_float64(gt88, ftl, closed):
    a, b = both_paths(gt88, ftl, closed)
    assert same_bits(a, b), (ftl, closed, gt88.L.T)
    if closed:
        assert np.all(a[3] == 1)
    else:
        assert np.all(a[3] == 0)


# ------------------------------------------------------------------ consumer: forced instances
def persistent(db, bits, ftl, onepass, nwaves):
    import torch
    from online_convex_optimization_amd import _lib
    B = db.L.B
    out = [torch.full((B,), SENTINEL, dtype=torch.float64, device=db.device) for _ in range(3)]
    closed = torch.full((B,), 7, dtype=torch.int32, device=db.device)
    torch.cuda.synchronize()
    with torch.cuda.device(db.device):
        rc = _lib.load().ocx_test_alg_pipe_persistent_bits(
            ctypes.byref(db.L), db.z.data_ptr(), db._y.data_ptr(),
            db._ybits.data_ptr() if bits else None, ftl, SQ2, onepass, nwaves,
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), closed.data_ptr(),
            ctypes.c_void_p(db.stream.cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, _lib.last_error()
    return tuple(t.cpu().numpy() for t in (*out, closed))


@pytest.fixture(scope="module", params=[63, 64, 65, 130, 1000])
def gt88_pers(request, eng):
    # T = 63, 64: one block, its word also the clamped look-ahead; 65: a second block of one
    # step; 130, 1000: several blocks, the last partial — in every group of a wave's loop
    db = eng.DeviceBatch(59, request.param, 64, lanes_per_seq=8).generate_gT(base_seed=11, run0=2)
    assert db.label_bits_valid
    return db


@pytest.mark.parametrize("nwaves", [1, 3])
@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("ftl", [0, 1])
def test_persistent_from_bits(gt88_pers, ftl, onepass, nwaves):
    """One wave running all eight groups, and three waves with shares 3 / 3 / 2."""
    db = gt88_pers
    a = persistent(db, True, ftl, onepass, nwaves)
    b = persistent(db, False, ftl, onepass, nwaves)
    assert same_bits(a, b), (ftl, onepass, nwaves)
    assert not np.any(a[0] == SENTINEL)


# ------------------------------------------------------------------ packed batches
def packed(eng, label=None, norm=None):
    rng = np.random.default_rng(23)
    B, T = 59, 130
    z = rng.standard_normal((B, T, 64))
    z /= np.maximum(np.linalg.norm(z, axis=2, keepdims=True), 1.0) * 1.0000001
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    if norm is not None:
        z[5, 70] *= norm / np.linalg.norm(z[5, 70])
    if label is not None:
        y[9, 100] = label
    return eng.DeviceBatch(B, T, 64, lanes_per_seq=8).pack(z, y), z, y


def test_packed_batch_streams_the_second_pass_from_bits(eng):
    """±1 labels and one user row of norm 1.5: sequence 5 fails the certificate, so its wave
    streams the second comparator pass — from bits."""
    db, _, _ = packed(eng, norm=1.5)
    assert db.label_bits_valid
    for ftl in (0, 1):
        a, b = both_paths(db, ftl, 1)
        assert same_bits(a, b), ftl
        assert a[3][5] == 0 and a[3].sum() == db.L.B - 1
        for nwaves in (1, 3):  # the instance that reads bits: group 0's wave streams the pass
            p = persistent(db, True, ftl, 1, nwaves)
            assert same_bits(p, b), (ftl, nwaves)


def direct_ex(db, ftl, closed):
    """ocx_dev_simulate_alg_ex itself: the float64 entry point, as before this tile existed."""
    import torch
    from online_convex_optimization_amd import _lib
    out = [torch.full((db.L.B,), SENTINEL, dtype=torch.float64, device=db.device) for _ in range(3)]
    flags = torch.full((db.L.B,), 7, dtype=torch.int32, device=db.device)
    torch.cuda.synchronize()
    with torch.cuda.device(db.device):
        _lib.call("ocx_dev_simulate_alg_ex", ctypes.byref(db.L), db.z.data_ptr(),
                  db._y.data_ptr(), ftl, SQ2, None, out[0].data_ptr(), out[1].data_ptr(),
                  out[2].data_ptr(), None, _lib.OCX_ALG_CLIPPED_ROWS if closed else 0,
                  flags.data_ptr(), ctypes.c_void_p(db.stream.cuda_stream))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (*out, flags))


def test_fallback_on_a_label_that_is_not_unit(eng):
    """A 0.5 label: pack's flag is raised, the bits are dropped, the results are today's."""
    db, _, _ = packed(eng, label=0.5)
    assert not db.label_bits_valid
    for closed in (0, 1):
        assert same_bits(simulate(db, 0, closed), direct_ex(db, 0, closed))
    assert simulate(db, 0, 1)[3][9] == 0  # |y| != 1: no closed form for that sequence


def test_fallback_on_a_stream_that_is_not_current(eng):
    """A batch on a stream of its own, a 0.5 label: pack's flag is written by a kernel on that
    stream and must be read there — the bits are dropped, the regrets are the float64 path's."""
    import torch
    rng = np.random.default_rng(7)
    B, T = 59, 130
    z = rng.standard_normal((B, T, 64)) / 9.0
    y = np.where(rng.random((B, T)) < 0.5, -1.0, 1.0)
    y[B - 1, T - 1] = 0.5  # the last label the pack kernel reaches
    side = torch.cuda.Stream()
    # a long kernel queued first on the side stream: the flag's kernel runs well after pack's
    # host code has moved on
    with torch.cuda.stream(side):
        busy = torch.randn(4096, 4096, device="cuda")
        for _ in range(20):
            busy = busy @ busy
            busy = busy / busy.norm()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=side).pack(z, y)
    assert torch.cuda.current_stream() != side
    assert not db.label_bits_valid
    flags = torch.full((B,), 7, dtype=torch.int32, device=db.device)
    with torch.cuda.stream(side):
        db.simulate_alg(0, SQ2, closed_comparator=True, closed_out=flags)
    side.synchronize()
    got = (db.regret.cpu().numpy().copy(), db.cum.cpu().numpy().copy(), db.comp.cpu().numpy().copy(),
           flags.cpu().numpy())
    want = direct_ex(db, 0, 1)
    assert same_bits(got, want)
    assert got[3][B - 1] == 0
    y[B - 1, T - 1] = 1.0  # and with unit labels the same batch keeps its bits
    assert eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=side).pack(z, y).label_bits_valid


def test_reading_y_invalidates_the_bits(eng):
    import torch
    db = eng.DeviceBatch(59, 130, 64, lanes_per_seq=8).generate_gT(base_seed=11, run0=2)
    assert db.label_bits_valid
    db.y[(0 * 130 + 7) * 8 + 2] = 0.5  # sequence 2, step 7: written in place through the property
    assert not db.label_bits_valid
    got = simulate(db, 0, 1)
    assert same_bits(got, direct_ex(db, 0, 1))
    assert got[3][2] == 0
    db.generate_gT(base_seed=11, run0=2)  # the next producer call validates them again
    assert db.label_bits_valid
    assert np.all(simulate(db, 0, 1)[3] == 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ pipelines
def test_pipelines_stay_bit_identical(eng):
    """generate_simulate pipelined (sub-batches of 1 024) and sequential (both on y's doubles:
    the tile is not written beside the pipelines, so it is marked invalid), and generate_gT
    followed by simulate_alg with the tile valid, at 4 096 x 130 x 64 — 512 wave-groups, below
    one round, so that launch too reads y's doubles: the three agree through the same kernels'
    arithmetic, and the tile only rides along."""
    import torch
    B, T = 4096, 130
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8)
    regs, gms = [], []
    for mode in (True, False):
        g = torch.zeros(1, dtype=torch.float64, device=db.device)
        db.generate_simulate(base_seed=9, run0=5, nbatch=2, gmax=g, pipelined=mode, sub_seqs=1024)
        torch.cuda.synchronize()
        assert not db.label_bits_valid
        regs.append(db.regret[:B].cpu().numpy().copy())
        gms.append(float(g.item()))
    db.generate_gT(base_seed=9, run0=5 + B)
    assert db.label_bits_valid
    regs.append(simulate(db, 0, 1)[0])
    assert same_bits(regs[:1], regs[1:2]) and same_bits(regs[:1], regs[2:])
    assert gms[0] == gms[1]
    _ = db.y
    assert same_bits((simulate(db, 0, 1)[0],), regs[:1])  # and the float64 path's regrets
