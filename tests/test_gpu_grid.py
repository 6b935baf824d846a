"""Regret grids (ocx_dev_simulate_alg_curve_etas and the layers above it): FTRL for M values of
eta0, each observed at K checkpoint horizons, in passes over z that each serve a group of step
sizes.

The reference of every check is the C oracle on the TRUNCATED input or the existing
simulate_alg_curve / simulate_alg_etas / simulate_alg calls, never the grid code: bit for bit
against the oracle in the exact modes, bit for bit per step size against
DeviceBatch.simulate_alg_curve in the same layout for every forced group size, and
`close_closed` against the oracle where the closed form was taken.  The `beam` family
(tests/_etas_cases.py; tests/test_grid_cpu.py asserts the condition per prefix) gives every step
size its own θ trajectory within every checkpoint from 63 up."""
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
# the ring depth, the 64-step boundaries of the U refresh and of the scale table, the last step
# and both ends
CHECKPOINTS = [0, 1, 2, 63, 64, 65, 128, 129, 256, 257]
CERT_CHECKPOINTS = [1, 63, 64, 65, 129, 130]
KEYS = ("regret", "cum", "comp", "closed")


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
def oracle(name, d, eta, t):
    """(regret, cum, comp) of the C oracle on the first t steps of a family at step size eta."""
    f = family(name, d)
    return O.simulate_alg_batch(f.z[:, :t], f.y[:, :t], 0, eta, nthreads=4)[:3]


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def instance(L, group):
    """Whether the group-`group` form exists for layout L: the step-size sweep's set less the
    two chained instances DESIGN.md §3.16 records as dropped."""
    C, P, chain = int(L.C), int(L.P), int(L.chain)
    if chain and C == 8 and (P, group) in ((32, 4), (64, 2)):
        return False
    return group == 1 or (group == 2 and C <= 16) or (group == 4 and C <= 8)


# ------------------------------------------------------------------ 1. exact modes vs the oracle
EXACT = [(P, d) for d in (5, 16, 64) for P in (1, -1, -4)] + [(1, 100)]


@pytest.mark.parametrize("name", ("beam", "gt_like"))
@pytest.mark.parametrize("P,d", EXACT)
def test_exact_modes_equal_the_oracle_on_every_prefix(eng, P, d, name):
    f = family(name, d)
    reg, cum, comp, closed = eng.simulate_alg_curve_etas_batch(
        f.z, f.y, CHECKPOINTS, E.ETAS, lanes_per_seq=P, return_all=True)
    shape = (B, len(E.ETAS), len(CHECKPOINTS))
    assert reg.shape == cum.shape == comp.shape == closed.shape == shape
    assert np.all(closed == 0)   # streamed comparator for every triple
    for m, eta in enumerate(E.ETAS):
        for k, t in enumerate(CHECKPOINTS):
            ref = oracle(name, d, eta, t)
            for got, want, what in ((reg, ref[0], "regret"), (cum, ref[1], "cum"),
                                    (comp, ref[2], "comp")):
                assert np.array_equal(got[:, m, k], want), (P, d, name, eta, t, what)
    # the plain call returns the same regrets
    assert np.array_equal(eng.simulate_alg_curve_etas_batch(f.z, f.y, CHECKPOINTS, E.ETAS,
                                                            lanes_per_seq=P), reg)


# ------------------------------------------------------------------ 2. every layout, every group
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 5), (-4, 16), (1, 64)]


@pytest.mark.parametrize("name", ("beam", "gt_like", "straddle", "always"))
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_columns_equal_the_existing_kernels_for_every_group(eng, P, d, name):
    columns_equal_the_existing_kernels(eng, P, d, name)


# the two chained layouts with an instance DESIGN.md §3.16 records as dropped (8 coordinates on
# 32 and on 64 lanes): their groups run the next instance up, a forced group is refused
@pytest.mark.parametrize("name", ("beam", "gt_like"))
@pytest.mark.parametrize("P,d,dropped", [(-32, 256, 4), (-64, 512, 2)])
def test_dropped_instances_fall_back(eng, P, d, dropped, name):
    L = columns_equal_the_existing_kernels(eng, P, d, name)
    assert (int(L.P), int(L.C), int(L.chain)) == (-P, 8, 1)
    assert not instance(L, dropped) and all(instance(L, g) for g in (1, 2, 4) if g != dropped)
    if dropped == 2:   # 4 + 2 step sizes at group 4: the tail of two runs the 4-column instance
        f = family(name, d)
        db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
        etas = E.ETAS7[:6]
        got = host(db.simulate_alg_curve_etas(CHECKPOINTS, etas, closed_comparator=True, _group=4))
        for m, eta in enumerate(etas):
            ref = host(db.simulate_alg_curve(CHECKPOINTS, 0, eta, closed_comparator=True))
            for k in KEYS:
                assert np.array_equal(got[k][:, m, :], ref[k]), (P, d, name, m, k)


def columns_equal_the_existing_kernels(eng, P, d, name):
    from online_convex_optimization_amd import _lib
    f = family(name, d)   # straddle / always: their rows only, the step sizes are ETAS7
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    K = len(CHECKPOINTS)
    assert CHECKPOINTS[-1] == T
    for cc in (False, True):
        curves = [host(db.simulate_alg_curve(CHECKPOINTS, 0, eta, closed_comparator=cc))
                  for eta in E.ETAS7]
        sweep = host(db.simulate_alg_etas(E.ETAS7, closed_comparator=cc))

        def check(got, tag):
            for k in KEYS:
                assert got[k].shape == (B, len(E.ETAS7), K), (P, d, name, cc, tag, k)
                for m in range(len(E.ETAS7)):
                    assert np.array_equal(got[k][:, m, :], curves[m][k]), (P, d, name, cc, tag, k, m)
                assert np.array_equal(got[k][:, :, K - 1], sweep[k]), (P, d, name, cc, tag, k)
                assert np.array_equal(got[k][:, 2], got[k][:, 3]), (P, d, name, cc, tag, "dup", k)

        ok = []
        for group in (1, 2, 4):
            try:
                got = host(db.simulate_alg_curve_etas(CHECKPOINTS, E.ETAS7, closed_comparator=cc,
                                                      _group=group))
            except _lib.OCXError as e:
                assert not instance(db.L, group) and "unsupported" in str(e), (P, d, group, str(e))
                continue
            assert instance(db.L, group), (P, d, group)
            ok.append(group)
            check(got, group)
        pub = host(db.simulate_alg_curve_etas(CHECKPOINTS, E.ETAS7, closed_comparator=cc))
        check(pub, "public")
        assert _lib.load().ocx_curve_etas_group(ctypes.byref(db.L), 7) in ok
        if not cc:
            assert np.all(pub["closed"] == 0)
        elif name == "gt_like":
            assert np.all(pub["closed"] == 1)
    if name == "beam":   # the columns are different runs
        assert not np.array_equal(pub["cum"][:, 0, K - 1], pub["cum"][:, 1, K - 1])
    return db.L


# ------------------------------------------------------------------ 3. certificates per (sequence, eta, prefix)
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_certificates_per_sequence_step_size_and_prefix(eng, P, d):
    """An edited sequence is closed at exactly the checkpoints before its edit, for every step
    size; sequences 2 and 22 are open at 4 sqrt 2 from t_k = 2 on and closed at sqrt 2 and 1;
    no wave neighbour is taken along; open triples carry the bits of the flags = 0 call."""
    f, edits, two = E.cert_etas_case(d)
    etas = E.CERT_ETAS   # sqrt 2, 4 sqrt 2, 1
    Bc, Tc = f.y.shape
    M, K = len(etas), len(CERT_CHECKPOINTS)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    want = np.ones((Bc, M, K), dtype=np.int32)
    for b, (_, _, te) in edits.items():
        want[b, :, :] = [0 if te < t else 1 for t in CERT_CHECKPOINTS]
    for b in two:
        want[b, 1, :] = [0 if t >= 2 else 1 for t in CERT_CHECKPOINTS]
    per_eta = [host(db.simulate_alg_curve(CERT_CHECKPOINTS, 0, eta, closed_comparator=True))
               for eta in etas]
    for m in range(M):
        assert np.array_equal(per_eta[m]["closed"], want[:, m, :]), (P, d, m)
    zero = host(db.simulate_alg_curve_etas(CERT_CHECKPOINTS, etas, closed_comparator=False))
    assert np.all(zero["closed"] == 0)
    ora = [[O.simulate_alg_batch(f.z[:, :t], f.y[:, :t], 0, eta, nthreads=4)[:3]
            for t in CERT_CHECKPOINTS] for eta in etas]
    S = int(db.L.S)
    shared = [b for b in range(Bc) if b not in edits and b not in two
              and any(e // S == b // S for e in list(edits) + list(two))]
    assert shared or S == 1
    groups = [g for g in (1, 2, 4) if instance(db.L, g)]
    for group in groups + [None]:
        one = host(db.simulate_alg_curve_etas(CERT_CHECKPOINTS, etas, closed_comparator=True,
                                              _group=group))
        assert np.array_equal(one["closed"], want), (P, d, group)
        assert np.all(one["closed"][shared] == 1)
        op = one["closed"] == 0
        for k in ("regret", "cum", "comp"):
            assert np.array_equal(one[k][op], zero[k][op]), (P, d, group, k)
            for m in range(M):
                assert np.array_equal(one[k][:, m, :], per_eta[m][k]), (P, d, group, k, m)
        assert np.array_equal(one["cum"], zero["cum"])
        for m in range(M):
            for kk, t in enumerate(CERT_CHECKPOINTS):
                cl = one["closed"][:, m, kk] == 1
                for i, k in enumerate(("regret", "cum", "comp")):
                    assert close_closed(one[k][cl, m, kk], ora[m][kk][i][cl], t), \
                        (P, d, group, m, t, k)


# ------------------------------------------------------------------ 4. degenerate cases
def test_degenerate_cases(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = family("beam", 5)
    db = eng.DeviceBatch(B, T, 5, lanes_per_seq=1).pack(f.z, f.y)
    # M = 0, K = 0, both: host and device
    for ck, et in ((CHECKPOINTS, []), ([], E.ETAS), ([], [])):
        shape = (B, len(et), len(ck))
        got = eng.simulate_alg_curve_etas_batch(f.z, f.y, ck, et, lanes_per_seq=1, return_all=True)
        assert all(g.shape == shape for g in got)
        assert eng.simulate_alg_curve_etas_batch(f.z, f.y, ck, et).shape == shape
        assert all(v.shape == shape for v in host(db.simulate_alg_curve_etas(ck, et)).values())
        assert eng.gT_regret_curves_etas(10, 3, ck[:1], et).shape == (3, len(et), len(ck[:1]))
        assert eng.gT_surface(10, 3, ck[:1], et).shape == (len(et), len(ck[:1]))
    # T = 0: zeros
    z0, y0 = np.zeros((B, 0, 5)), np.zeros((B, 0))
    for lanes in (1, 0):
        got = eng.simulate_alg_curve_etas_batch(z0, y0, [0], E.ETAS, lanes_per_seq=lanes,
                                                return_all=True)
        assert all(g.shape == (B, len(E.ETAS), 1) and np.all(g == 0.0) for g in got[:3])
    out = host(eng.DeviceBatch(B, 0, 64, lanes_per_seq=8).simulate_alg_curve_etas([0], E.ETAS))
    assert all(np.all(out[k] == 0.0) for k in ("regret", "cum", "comp"))
    # B = 1: the oracle on each prefix
    cks = [0, 1, 64, 200, T]
    got = eng.simulate_alg_curve_etas_batch(f.z[:1], f.y[:1], cks, E.ETAS, lanes_per_seq=1,
                                            return_all=True)
    for m, eta in enumerate(E.ETAS):
        for k, t in enumerate(cks):
            ref = O.simulate_alg_full(f.z[0, :t], f.y[0, :t], 0, eta)
            assert (got[0][0, m, k], got[1][0, m, k], got[2][0, m, k]) == tuple(ref[:3]), (eta, t)
    # M = K = 1: the single call
    got = eng.simulate_alg_curve_etas_batch(f.z, f.y, [T], [2.0], lanes_per_seq=1, return_all=True)
    ref = eng.simulate_alg_batch(f.z, f.y, 0, 2.0, lanes_per_seq=1, return_all=True)
    for g, r in zip(got[:3], ref[:3]):
        assert g.shape == (B, 1, 1) and np.array_equal(g[:, 0, 0], r)
    # etas / checkpoints that are not valid lists
    for bad in ([[1.0, 2.0]], ["a", "b"], [None], 1.0, [1.0 + 2.0j]):
        with pytest.raises(ValueError):
            eng.simulate_alg_curve_etas_batch(f.z, f.y, CHECKPOINTS, bad)
        with pytest.raises(ValueError):
            db.simulate_alg_curve_etas(CHECKPOINTS, bad)
        with pytest.raises(ValueError):
            eng.gT_regret_curves_etas(10, 2, [5, 10], bad)
        with pytest.raises(ValueError):
            eng.gT_surface(10, 2, [5, 10], bad)
    for bad in ([5, 5], [7, 3], [-1, 4], [3, T + 1], [[1, 2]], [1.5, 2.0], 3):
        with pytest.raises(ValueError):
            eng.simulate_alg_curve_etas_batch(f.z, f.y, bad, E.ETAS)
        with pytest.raises(ValueError):
            db.simulate_alg_curve_etas(bad, E.ETAS)
        with pytest.raises(ValueError):
            eng.gT_regret_curves_etas(T, 2, bad, E.ETAS)
    # the C host entry validates the checkpoints itself, before any device is touched
    lib = _lib.load()
    et = np.ascontiguousarray(E.ETAS, dtype=np.float64)
    M = et.size
    for bad in ([5, 5], [7, 3], [-1, 4], [3, T + 1]):
        ck = np.asarray(bad, dtype=np.int64)
        rc = lib.ocx_simulate_alg_curve_etas_batch(
            _lib.ptr(f.z), _lib.ptr(f.y), B, T, 5, _lib.ptr(et), M,
            ck.ctypes.data_as(_lib.c_i64p), ck.size, None, None, None, None, 1, 0)
        assert rc == -1, bad
    assert lib.ocx_simulate_alg_curve_etas_batch(
        _lib.ptr(f.z), _lib.ptr(f.y), B, T, 5, _lib.ptr(et), -1, None, 0, None, None, None, None,
        1, 0) == -1
    # an undersized workspace: OCX_E_INVALID (which _lib.check raises as its invalid-argument
    # error), nothing launched, the outputs untouched
    ck = np.asarray(CHECKPOINTS, dtype=np.int64)
    K = ck.size
    need = int(lib.ocx_curve_etas_workspace_bytes(ctypes.byref(db.L), K, M))
    group = int(lib.ocx_curve_etas_group(ctypes.byref(db.L), M))
    assert need == int(db.L.G) * K * min(group, M) * 64 * (8 * int(db.L.C) + 12) > 0
    ckd = torch.as_tensor(ck).to(db.device)
    outs = [torch.full((B, M, K), 7.0, dtype=torch.float64, device=db.device) for _ in range(3)]
    outs.append(torch.full((B, M, K), 7, dtype=torch.int32, device=db.device))
    ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=db.device)
    args = lambda nbytes: (ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), _lib.ptr(et), M,
                           ckd.data_ptr(), K, outs[0].data_ptr(), outs[1].data_ptr(),
                           outs[2].data_ptr(), outs[3].data_ptr(), 0, ws.data_ptr(), nbytes,
                           db._sp)
    with torch.cuda.device(db.device):
        assert lib.ocx_dev_simulate_alg_curve_etas(*args(need - 1)) == -1   # OCX_E_INVALID
        with pytest.raises((ValueError, _lib.OCXError), match="workspace"):
            _lib.call("ocx_dev_simulate_alg_curve_etas", *args(need - 1))
        torch.cuda.synchronize()
        assert all(bool(torch.all(o == 7)) for o in outs)
        _lib.call("ocx_dev_simulate_alg_curve_etas", *args(need))            # exactly enough
    torch.cuda.synchronize()
    py = eng.simulate_alg_curve_etas_batch(f.z, f.y, CHECKPOINTS, E.ETAS, lanes_per_seq=1,
                                           return_all=True)
    for o, want in zip(outs, py):
        assert np.array_equal(o.cpu().numpy(), want)
    # a direct ctypes call of the host entry equals the Python path
    raw = [np.full((B, M, K), 7.0) for _ in range(3)] + [np.full((B, M, K), 7, dtype=np.int32)]
    rc = lib.ocx_simulate_alg_curve_etas_batch(
        _lib.ptr(f.z), _lib.ptr(f.y), B, T, 5, _lib.ptr(et), M, ck.ctypes.data_as(_lib.c_i64p), K,
        _lib.ptr(raw[0]), _lib.ptr(raw[1]), _lib.ptr(raw[2]),
        raw[3].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, 0)
    assert rc == 0
    for r, want in zip(raw, py):
        assert np.array_equal(r, want)


# ------------------------------------------------------------------ 5. capture
def test_device_call_is_capture_safe(eng):
    import torch
    from online_convex_optimization_amd import _lib
    f = family("beam", 64)
    s = torch.cuda.Stream()
    db = eng.DeviceBatch(B, T, 64, lanes_per_seq=8, stream=s).pack(f.z, f.y)
    assert (db.L.P, db.L.C) == (8, 8)
    et = np.ascontiguousarray(E.ETAS, dtype=np.float64)
    M, K = et.size, len(CHECKPOINTS)
    need = int(_lib.load().ocx_curve_etas_workspace_bytes(ctypes.byref(db.L), K, M))
    with torch.cuda.stream(s):
        ckd = torch.as_tensor(np.asarray(CHECKPOINTS, dtype=np.int64)).to(db.device)
        ws = torch.empty(need // 8 + 1, dtype=torch.float64, device=db.device)

    def buffers():
        with torch.cuda.stream(s):
            o = [torch.zeros((B, M, K), dtype=torch.float64, device=db.device) for _ in range(3)]
            o.append(torch.zeros((B, M, K), dtype=torch.int32, device=db.device))
        return o

    def run(o):
        with torch.cuda.device(db.device):
            _lib.call("ocx_dev_simulate_alg_curve_etas", ctypes.byref(db.L), db.z.data_ptr(),
                      db.y.data_ptr(), _lib.ptr(et), M, ckd.data_ptr(), K, o[0].data_ptr(),
                      o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                      _lib.OCX_ALG_CLOSED_COMPARATOR, ws.data_ptr(), ws.numel() * 8,
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
    assert not torch.equal(eager[1][:, 0, K - 1], eager[1][:, 4, K - 1])   # column by column
    for m, eta in enumerate(E.ETAS):                                       # the existing kernels'
        ref = db.simulate_alg_curve(CHECKPOINTS, 0, eta, closed_comparator=True)
        torch.cuda.synchronize()
        for i, k in enumerate(KEYS):
            assert torch.equal(ref[k], cap[i][:, m, :]), (eta, k)


# ------------------------------------------------------------------ 6. g(T) layer
GT_CKS = [50, 100, 200]


def test_gT_regret_curves_etas_exact(eng):
    got = eng.gT_regret_curves_etas(200, 20, GT_CKS, E.ETAS, d=5, lanes_per_seq=1, batch=8)
    assert got.shape == (20, len(E.ETAS), 3)   # 8 + 8 + 4
    for m, eta in enumerate(E.ETAS):
        assert np.array_equal(got[:, m, :], eng.gT_regret_curves(200, 20, GT_CKS, d=5, eta0=eta,
                                                                 lanes_per_seq=1, batch=8)), eta
    assert np.array_equal(got[:, :, 2], eng.gT_regrets_etas(200, 20, E.ETAS, d=5, lanes_per_seq=1,
                                                            batch=8))
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 5)
        for m, eta in enumerate(E.ETAS):
            for k, t in enumerate(GT_CKS):
                assert got[r, m, k] == O.simulate_alg_full(z[:t], y[:t], 0, eta)[0], (r, eta, t)
    surf = eng.gT_surface(200, 20, GT_CKS, E.ETAS, d=5, lanes_per_seq=1, batch=8)   # three batches
    assert surf.shape == (len(E.ETAS), 3)
    assert np.array_equal(surf, np.maximum(0.0, got.max(axis=0)))
    for m, eta in enumerate(E.ETAS):
        assert surf[m, 2] == eng.gT_max(200, 20, eta0=eta, d=5, lanes_per_seq=1), eta


def test_gT_regret_curves_etas_closed_form(eng):
    lanes = eng.LANES_BEST
    got, closed = eng.gT_regret_curves_etas(200, 20, GT_CKS, E.ETAS, d=64, lanes_per_seq=lanes,
                                            batch=8, return_closed=True)
    assert got.shape == closed.shape == (20, len(E.ETAS), 3) and np.all(closed == 1)
    for r in range(20):
        z, y = O.gT_sample(0, 200, r, 64)
        for m, eta in enumerate(E.ETAS):
            for k, t in enumerate(GT_CKS):
                ref = O.simulate_alg_full(z[:t], y[:t], 0, eta)[0]
                assert close_closed(got[r, m, k], ref, t), (r, eta, t)
    surf = eng.gT_surface(200, 20, GT_CKS, E.ETAS, d=64, lanes_per_seq=lanes, batch=8)
    assert np.array_equal(surf, np.maximum(0.0, got.max(axis=0)))
    for m, eta in enumerate(E.ETAS):
        assert surf[m, 2] == eng.gT_max(200, 20, eta0=eta, d=64, lanes_per_seq=lanes), eta


# ------------------------------------------------------------------ 7. the column-wise maximum
def test_max_regret_cols(eng):
    import torch
    from online_convex_optimization_amd import _lib
    rng = np.random.default_rng(7)
    r = rng.standard_normal((37, 5))
    r[:, 1] = -np.abs(r[:, 1]) - 0.5          # all negative: +0.0
    r[11, 3] = np.nan                         # ignored
    want = np.array([max(0.0, np.nanmax(r[:, n])) for n in range(5)])
    assert want[1] == 0.0 and want[3] > 0.0
    dev = torch.device("cuda", 0)
    rd = torch.as_tensor(r).to(dev)
    g = torch.full((5,), -3.0, dtype=torch.float64, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.call("ocx_dev_max_regret_cols", rd.data_ptr(), 37, 5, g.data_ptr(), 0, sp)
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    assert np.array_equal(got, want) and not np.signbit(got[1])
    # accumulating onto a previous result: the maximum of both batches
    r2 = rng.standard_normal((37, 5)) * 2.0
    r2[:, 1] = -1.0
    r2[5, 0] = np.nan
    rd2 = torch.as_tensor(r2).to(dev)
    with torch.cuda.device(dev):
        _lib.call("ocx_dev_max_regret_cols", rd2.data_ptr(), 37, 5, g.data_ptr(), 1, sp)
    torch.cuda.synchronize()
    both = np.concatenate([r, r2])
    want2 = np.array([max(0.0, np.nanmax(both[:, n])) for n in range(5)])
    got2 = g.cpu().numpy()
    assert np.array_equal(got2, want2) and not np.signbit(got2[1])
    assert np.any(want2 != want)              # the second batch did raise a column
    # B = 0 fresh gives zeros; N = 0 is valid
    with torch.cuda.device(dev):
        _lib.call("ocx_dev_max_regret_cols", None, 0, 5, g.data_ptr(), 0, sp)
        _lib.call("ocx_dev_max_regret_cols", rd.data_ptr(), 37, 0, None, 0, sp)
    torch.cuda.synchronize()
    assert np.all(g.cpu().numpy() == 0.0)
