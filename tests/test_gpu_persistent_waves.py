"""The pipelined FTRL/FTL kernel's persistent instance (ocx_test_alg_pipe_persistent): waves
that loop over wave-groups w, w + nwaves, ... instead of owning one.  Every comparison is bit
for bit — regret, cum, comp, closed_out — against the product call on the same resident data,
which at these sizes launches one wave per group."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SQ2 = math.sqrt(2)
OCX_E_UNSUPPORTED = -3
SENTINEL = -7.25


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    assert _lib.device_count() >= 1
    return engine


def product(db, ftl, onepass):
    """The product call's (regret, cum, comp, closed_out) as host arrays."""
    import torch
    closed = torch.full((db.L.B,), 7, dtype=torch.int32, device=db.device)
    db.simulate_alg(ftl, SQ2, closed_comparator=bool(onepass), closed_out=closed)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in (db.regret, db.cum, db.comp, closed))


def persistent(db, ftl, onepass, nwaves):
    """The hook's outputs as host arrays (sentinel-filled first: every live sequence is
    written), or its error code."""
    import torch
    from online_convex_optimization_amd import _lib
    B = db.L.B
    out = [torch.full((B,), SENTINEL, dtype=torch.float64, device=db.device) for _ in range(3)]
    closed = torch.full((B,), 7, dtype=torch.int32, device=db.device)
    torch.cuda.synchronize()
    with torch.cuda.device(db.device):
        rc = _lib.load().ocx_test_alg_pipe_persistent(
            ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), ftl, SQ2, onepass, nwaves,
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), closed.data_ptr(),
            ctypes.c_void_p(db.stream.cuda_stream))
    torch.cuda.synchronize()
    if rc != 0:
        return rc
    return tuple(t.cpu().numpy() for t in (*out, closed))


def same_bits(got, want):
    return all(np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              w.view(np.uint64) if w.dtype == np.float64 else w)
               for g, w in zip(got, want))


# ------------------------------------------------------------------ 8 x 8, g(T) rows
B8, T8 = 59, 130  # G = 8, the last group 3 live + 5 padding sequences; T crosses the 64-step
#                   refresh twice and is no multiple of the ring


@pytest.fixture(scope="module")
def gt88(eng):
    db = eng.DeviceBatch(B8, T8, 64, lanes_per_seq=8).generate_gT(base_seed=11, run0=2)
    assert (db.L.P, db.L.C, db.L.G, db.L.chain) == (8, 8, 8, 0)
    want = {(ftl, op): product(db, ftl, op) for ftl in (0, 1) for op in (0, 1)}
    return db, want


@pytest.mark.parametrize("nwaves", [1, 3, 8, 16])
@pytest.mark.parametrize("onepass", [0, 1])
@pytest.mark.parametrize("ftl", [0, 1])
def test_persistent_matches_product_8x8(gt88, ftl, onepass, nwaves):
    """One wave running all eight groups, three waves with 3/3/2, one group each, and more
    waves than groups: FTRL and FTL, streamed and closed-form comparator."""
    db, want = gt88
    w = want[(ftl, onepass)]
    if onepass:
        assert np.all(w[3] == 1)  # the sampler's rows are all certified
    got = persistent(db, ftl, onepass, nwaves)
    assert not isinstance(got, int), got
    assert same_bits(got, w), (ftl, onepass, nwaves)


def test_persistent_matches_oracle(gt88):
    """One case against the CPU oracle, at the closed form's bar of tests/test_gpu_parity.py:
    |diff| <= max(1e-12 * max(1, |ref|), 4 eps T^1.5)."""
    db, _ = gt88
    got = persistent(db, 0, 1, 3)
    assert not isinstance(got, int), got
    ref = np.array([O.simulate_alg(*O.gT_sample(11, T8, 2 + b, 64), 0, SQ2) for b in range(B8)])
    tol = np.maximum(1e-12 * np.maximum(1.0, np.abs(ref)), 4 * 2.22e-16 * float(T8) ** 1.5)
    assert np.all(np.abs(got[0] - ref) <= tol), np.abs(got[0] - ref).max()


# ------------------------------------------------------------------ 16 x 4
@pytest.mark.parametrize("nwaves", [1, 4])
def test_persistent_16x4(eng, nwaves):
    """FTRL, closed-form comparator: the product call's bits if the layout has a persistent
    instance, OCX_E_UNSUPPORTED if not."""
    from online_convex_optimization_amd import _lib
    db = eng.DeviceBatch(21, 70, 64, lanes_per_seq=16).generate_gT(base_seed=4, run0=9)
    assert (db.L.P, db.L.C, db.L.chain) == (16, 4, 0)
    want = product(db, 0, 1)
    got = persistent(db, 0, 1, nwaves)
    if isinstance(got, int):
        assert got == OCX_E_UNSUPPORTED, (got, _lib.last_error())
    else:
        assert same_bits(got, want), nwaves


# ------------------------------------------------------------------ uncertified rows
def test_persistent_uncertified_rows(eng):
    """Unnormalised random rows, closed form requested: no sequence is certified, so every
    group of a wave streams the second pass — `clean` or `comp` leaking from the wave's
    previous group would show.  closed_out is 0 exactly where the product call's is."""
    rng = np.random.default_rng(23)
    z = rng.standard_normal((B8, T8, 64))
    y = np.where(rng.random((B8, T8)) < 0.5, -1.0, 1.0)
    db = eng.DeviceBatch(B8, T8, 64, lanes_per_seq=8).pack(z, y)
    assert (db.L.P, db.L.C, db.L.G) == (8, 8, 8)
    want = product(db, 0, 1)
    assert np.all(want[3] == 0)
    got = persistent(db, 0, 1, 3)
    assert not isinstance(got, int), got
    assert np.array_equal(got[3] == 0, want[3] == 0)
    assert same_bits(got, want)
