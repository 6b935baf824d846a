"""Step-size sweeps (ocx_dev_simulate_alg_etas and the layers above it): FTRL for M values of
eta0 in passes over z that each serve a group of them.

The reference of every check is the C oracle or the existing single-eta kernels, never the
sweep code: bit for bit against the oracle in the exact modes, bit for bit per column against
DeviceBatch.simulate_alg in the same layout for every forced group size, and `close_closed`
against the oracle where the closed form was taken.  The `beam` family (tests/_etas_cases.py,
conditions asserted in tests/test_etas_cpu.py) gives every step size its own θ trajectory."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _etas_cases as E
from tests import _families as F
from tests.test_gpu_curve import close_closed

pytestmark = pytest.mark.gpu

B, T = E.B, E.T
SQ2 = E.SQ2


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    _lib.load()
    return engine


@functools.lru_cache(maxsize=None)
def family(name, d):
    """Shared between tests: never written to."""
    if name == "beam":
        return E.beam(d)
    return F.make(name, B, T, d, 100 + d)


@functools.lru_cache(maxsize=None)
def oracle(name, d, eta):
    f = family(name, d)
    return O.simulate_alg_batch(f.z, f.y, 0, eta, nthreads=4)[:3]


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100)]


@pytest.mark.parametrize("name", ("beam", "gt_like"))
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle(eng, P, d, name):
    f = family(name, d)
    reg, cum, comp, closed = eng.simulate_alg_etas_batch(f.z, f.y, E.ETAS, lanes_per_seq=P,
                                                         return_all=True)
    assert reg.shape == cum.shape == comp.shape == closed.shape == (B, len(E.ETAS))
    assert np.all(closed == 0)   # streamed comparator for every pair
    for m, eta in enumerate(E.ETAS):
        ref = oracle(name, d, eta)
        for got, want, what in ((reg, ref[0], "regret"), (cum, ref[1], "cum"),
                                (comp, ref[2], "comp")):
            assert np.array_equal(got[:, m], want), (P, d, name, eta, what)
    # the plain call returns the same regrets
    assert np.array_equal(eng.simulate_alg_etas_batch(f.z, f.y, E.ETAS, lanes_per_seq=P), reg)


# ------------------------------------------------------------------ 2. every layout, every group
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 5), (-4, 16), (1, 64)]
KEYS = ("regret", "cum", "comp", "closed")


def existing(eng, db, etas, cc):
    """[B, M] per output of the existing single-eta path on the packed batch."""
    import torch
    Bn = int(db.L.B)
    ref = {k: np.zeros((Bn, len(etas)), dtype=np.int32 if k == "closed" else np.float64)
           for k in KEYS}
    for m, eta in enumerate(etas):
        cl = torch.full((Bn,), 7, dtype=torch.int32, device=db.device)
        db.simulate_alg(0, eta, closed_comparator=cc, closed_out=cl)
        torch.cuda.synchronize()
        for k, t in (("regret", db.regret), ("cum", db.cum), ("comp", db.comp), ("closed", cl)):
            ref[k][:, m] = t[:Bn].cpu().numpy()
    return ref


@pytest.mark.parametrize("name", ("beam", "gt_like", "straddle", "always"))
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_columns_equal_the_existing_kernels_for_every_group(eng, P, d, name):
    from online_convex_optimization_amd import _lib
    f = family(name, d)   # straddle / always: their rows only, the step sizes are ETAS7
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    C = int(db.L.C)
    for cc in (False, True):
        ref = existing(eng, db, E.ETAS7, cc)
        ok = []
        for group in (1, 2, 4):
            must = group == 1 or C <= 8 or (group == 2 and C == 16)
            try:
                got = host(db.simulate_alg_etas(E.ETAS7, closed_comparator=cc, _group=group))
            except _lib.OCXError as e:
                assert not must and "unsupported" in str(e), (P, d, group, str(e))
                continue
            ok.append(group)
            for k in KEYS:
                assert np.array_equal(got[k], ref[k]), (P, d, name, cc, group, k)
        pub = host(db.simulate_alg_etas(E.ETAS7, closed_comparator=cc))
        for k in KEYS:
            assert np.array_equal(pub[k], ref[k]), (P, d, name, cc, "public", k)
            assert np.array_equal(pub[k][:, 2], pub[k][:, 3]), (P, d, name, cc, "duplicate", k)
        assert _lib.load().ocx_etas_group(ctypes.byref(db.L), 7) in ok
        if not cc:
            assert np.all(pub["closed"] == 0)
        elif name == "gt_like":
            assert np.all(pub["closed"] == 1)
    if name == "beam":   # the columns are different runs
        assert not np.array_equal(pub["cum"][:, 0], pub["cum"][:, 1])


# ------------------------------------------------------------------ 3. certificates per (sequence, eta)
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_certificates_per_sequence_and_step_size(eng, P, d):
    f, edits, two = E.cert_etas_case(d)
    etas = E.CERT_ETAS   # sqrt 2, 4 sqrt 2, 1
    Bc, Tc = f.y.shape
    ora = [O.simulate_alg_batch(f.z, f.y, 0, eta, nthreads=4)[:3] for eta in etas]
    # the exact host entry: streamed everywhere, the oracle's bits, and the two edited
    # sequences do run differently at 4 sqrt 2
    reg, cum, comp, closed = eng.simulate_alg_etas_batch(f.z, f.y, etas, lanes_per_seq=1,
                                                         return_all=True)
    assert np.all(closed == 0)
    for m in range(len(etas)):
        for got, want in zip((reg, cum, comp), ora[m]):
            assert np.array_equal(got[:, m], want), (d, m)
    for b in two:
        assert ora[1][1][b] != ora[0][1][b]

    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    want = existing(eng, db, etas, True)
    zero = host(db.simulate_alg_etas(etas, closed_comparator=False))
    assert np.all(zero["closed"] == 0)
    S = int(db.L.S)
    shared = [b for b in range(Bc) if b not in edits and b not in two
              and any(e // S == b // S for e in list(edits) + list(two))]
    assert shared or S == 1
    groups = [g for g in (1, 2, 4) if g == 1 or db.L.C <= 8 or (g == 2 and db.L.C == 16)]
    for group in groups + [None]:
        one = host(db.simulate_alg_etas(etas, closed_comparator=True, _group=group))
        assert np.array_equal(one["closed"], want["closed"]), (P, d, group)
        for b in two:   # closed at sqrt 2 and 1, not at 4 sqrt 2
            assert list(one["closed"][b]) == [1, 0, 1], (P, d, group, b)
        assert np.all(one["closed"][shared] == 1)
        op = one["closed"] == 0
        for k in ("regret", "cum", "comp"):
            assert np.array_equal(one[k], want[k]), (P, d, group, k)
            assert np.array_equal(one[k][op], zero[k][op]), (P, d, group, k)
        assert np.array_equal(one["cum"], zero["cum"])
        for m in range(len(etas)):
            cl = one["closed"][:, m] == 1
            for i, k in enumerate(("regret", "cum", "comp")):
                assert close_closed(one[k][cl, m], ora[m][i][cl], Tc), (P, d, group, m, k)


# ------------------------------------------------------------------ 4. degenerate cases
def test_degenerate_cases(eng):
    f = family("beam", 5)
    # M = 0, host and device
    got = eng.simulate_alg_etas_batch(f.z, f.y, [], lanes_per_seq=1, return_all=True)
    assert all(g.shape == (B, 0) for g in got)
    assert eng.simulate_alg_etas_batch(f.z, f.y, []).shape == (B, 0)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    assert all(v.shape == (B, 0) for v in host(db.simulate_alg_etas([])).values())
    # M = 1: the single-eta call
    got = eng.simulate_alg_etas_batch(f.z, f.y, [2.0], lanes_per_seq=1, return_all=True)
    ref = eng.simulate_alg_batch(f.z, f.y, 0, 2.0, lanes_per_seq=1, return_all=True)
    for g, r in zip(got[:3], ref[:3]):
        assert g.shape == (B, 1) and np.array_equal(g[:, 0], r)
    # T = 0: zeros
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    for lanes in (1, 0):
        got = eng.simulate_alg_etas_batch(z0, y0, E.ETAS, lanes_per_seq=lanes, return_all=True)
        assert all(g.shape == (B, len(E.ETAS)) and np.all(g == 0.0) for g in got[:3])
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_alg_etas(E.ETAS))
    assert all(np.all(out[k] == 0.0) for k in ("regret", "cum", "comp"))
    # B = 1
    got = eng.simulate_alg_etas_batch(f.z[:1], f.y[:1], E.ETAS, lanes_per_seq=1, return_all=True)
    for m, eta in enumerate(E.ETAS):
        ref = O.simulate_alg_full(f.z[0], f.y[0], 0, eta)
        assert (got[0][0, m], got[1][0, m], got[2][0, m]) == tuple(ref[:3]), eta
    # etas that are not a one-dimensional list of real numbers
    for bad in ([[1.0, 2.0]], ["a", "b"], [None], 1.0, [1.0 + 2.0j]):
        with pytest.raises(ValueError):
            eng.simulate_alg_etas_batch(f.z, f.y, bad)
        with pytest.raises(ValueError):
            db.simulate_alg_etas(bad)
        with pytest.raises(ValueError):
            eng.gT_regrets_etas(10, 2, bad)


# ------------------------------------------------------------------ 5. capture
def test_device_call_is_capture_safe(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = family("beam", 64)
    s = torch.cuda.Stream()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=s).pack(f.z, f.y)
    et = np.ascontiguousarray(E.ETAS, dtype=np.float64)
    M = et.size

    def buffers():
        with torch.cuda.stream(s):
            o = [torch.zeros((B, M), dtype=torch.float64, device=db.device) for _ in range(3)]
            o.append(torch.zeros((B, M), dtype=torch.int32, device=db.device))
        return o

    def run(o):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_alg_etas", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), _lib.ptr(et), M, o[0].data_ptr(), o[1].data_ptr(),
                      o[2].data_ptr(), o[3].data_ptr(), _lib.OCX_ALG_CLOSED_COMPARATOR,
                      ctypes.c_void_p(s.cuda_stream))

    eager, cap = buffers(), buffers()
    run(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run(cap)
    torch.cuda.synchronize()
    for t in cap:
        t.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        assert torch.equal(a, b)
    assert not torch.equal(eager[1][:, 0], eager[1][:, 4])   # it did run, column by column
    for m, eta in enumerate(E.ETAS):                          # and it is the existing kernel's
        db.simulate_alg(0, eta, closed_comparator=True)
        torch.cuda.synchronize()
        assert torch.equal(db.regret[:B], cap[0][:, m])


# ------------------------------------------------------------------ 6. g(T) layer
def test_gT_regrets_etas_exact(eng):
    got = eng.gT_regrets_etas(200, 20, E.ETAS, d=5, lanes_per_seq=1, batch=8)   # 8 + 8 + 4
    assert got.shape == (20, len(E.ETAS))
    for m, eta in enumerate(E.ETAS):
        assert np.array_equal(got[:, m], eng.gT_regrets(200, 20, eta0=eta, lanes_per_seq=1)), eta
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 5)
        for m, eta in enumerate(E.ETAS):
            assert got[r, m] == O.simulate_alg_full(z, y, 0, eta)[0], (r, eta)


def test_gT_regrets_etas_closed_form(eng):
    got, closed = eng.gT_regrets_etas(200, 20, E.ETAS, d=64, lanes_per_seq=eng.LANES_BEST,
                                      batch=8, return_closed=True)
    assert got.shape == closed.shape == (20, len(E.ETAS)) and np.all(closed == 1)
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 64)
        for m, eta in enumerate(E.ETAS):
            assert close_closed(got[r, m], O.simulate_alg_full(z, y, 0, eta)[0], 200), (r, eta)
