"""Anytime regret (ocx_dev_simulate_alg_anytime and the layers above it): the running max of
FTRL / FTL's regret over every prefix, its first argmax, and the dense trace, in one pass.

The reference of every check is existing code, never the anytime code: the dense regret curve
`simulate_alg_curve(range(1, T + 1), ..., closed_comparator=True)` on the SAME DeviceBatch (the
same layout, so the same arithmetic: bit for bit), and the C oracle on the truncated input in
the bit-exact mode."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import _families as F

pytestmark = pytest.mark.gpu

# ring depth, the 64-step boundaries of the scale table and of the U refresh; T = 257 ends
# mid-block and its checkpoint is the post-loop emission
CHECKPOINTS = [1, 2, 63, 64, 65, 128, 129, 256, 257]
CERT_CHECKPOINTS = [1, 63, 64, 65, 129, 130]
B, T = F.PIPE_B, 257


@pytest.fixture(scope="module")
def eng():
    from online_convex_optimization_amd import _lib, engine
    _lib.load()
    return engine


@functools.lru_cache(maxsize=None)
def family(name, d):
    return F.make(name, B, T, d, 100 + d)   # shared between tests: never written to


def host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def dense_reference(db, flag, eta0, cks):
    """sup, argsup, open_from and trace from the dense curve of the same batch."""
    Tn = int(db.L.T)
    out = host(db.simulate_alg_curve(np.arange(1, Tn + 1), flag, eta0, closed_comparator=True))
    return reference_of(out["regret"], out["closed"], cks)


def reference_of(reg, closed, cks):
    Bn, Tn = reg.shape
    sup = np.zeros((Bn, len(cks)))
    arg = np.zeros((Bn, len(cks)), dtype=np.int64)
    for k, t in enumerate(cks):
        sup[:, k] = reg[:, :t].max(axis=1)
        arg[:, k] = reg[:, :t].argmax(axis=1) + 1   # the first one
    opened = closed == 0
    open_from = np.where(opened.any(axis=1), opened.argmax(axis=1) + 1, Tn + 1)
    return {"sup": sup, "argsup": arg, "open_from": open_from.astype(np.int64), "trace": reg}


def assert_same(got, want, key):
    assert set(got) == set(want), key
    for what in ("sup", "argsup", "open_from", "trace"):
        assert got[what].dtype == want[what].dtype, key + (what,)
        assert np.array_equal(got[what], want[what], equal_nan=False), key + (what,)


# ------------------------------------------------------------------ 1. every layout, bit for bit
LAYOUTS = list(F.PIPE_SHAPES) + [(0, 5), (0, 64), (128, 5), (128, 64), (1, 5), (-4, 64), (-1, 16)]


@pytest.mark.parametrize("name", ("gt_like", "always", "pairs", "small"))
@pytest.mark.parametrize("P,d", LAYOUTS)
def test_every_layout_equals_the_dense_curve(eng, P, d, name):
    f = family(name, d)
    db = eng.DeviceBatch(B, T, d, lanes_per_seq=P).pack(f.z, f.y)
    got = host(db.simulate_alg_anytime(CHECKPOINTS, f.flag, f.eta0, closed_comparator=True,
                                       trace=True))
    want = dense_reference(db, f.flag, f.eta0, CHECKPOINTS)
    assert got["sup"].shape == got["argsup"].shape == (B, len(CHECKPOINTS))
    assert got["open_from"].shape == (B,) and got["trace"].shape == (B, T)
    assert_same(got, want, (P, d, name))
    if name in ("gt_like", "always", "small"):   # certified throughout: the kernel alone
        assert np.all(got["open_from"] == T + 1)
    # without the trace: the hot instance, the same numbers
    lean = host(db.simulate_alg_anytime(CHECKPOINTS, f.flag, f.eta0, closed_comparator=True))
    assert set(lean) == {"sup", "argsup", "open_from"}
    for what in lean:
        assert np.array_equal(lean[what], want[what]), (P, d, name, what)


@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("P", (0, 8))
def test_flip_sequence_equals_the_dense_curve(eng, P, flag):
    """The flip sequence (theta returns to exactly 0 at every other step) in the closed-form
    mode: its regret values repeat exactly, which exercises the first-argmax rule; whatever
    prefixes open are completed from the curve."""
    from online_convex_optimization_amd import sequence_generation as SG
    Tn, Bn = 40, 9
    z1, y1, _ = SG.flip_sequence(Tn, 5)
    z = np.repeat(z1[None].astype(np.float64), Bn, axis=0)
    y = np.repeat(y1[None].astype(np.float64), Bn, axis=0)
    db = eng.DeviceBatch(Bn, Tn, 5, lanes_per_seq=P).pack(z, y)
    cks = [1, 2, 7, 39, 40]
    got = host(db.simulate_alg_anytime(cks, flag, eng.SQRT2, closed_comparator=True, trace=True))
    want = dense_reference(db, flag, eng.SQRT2, cks)
    assert_same(got, want, (P, flag))


# ------------------------------------------------------------------ 2. certificates
@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("P,d", F.CERT_SHAPES)
def test_certificates_per_prefix(eng, P, d, flag):
    """A sequence whose certificate breaks at step t_e opens at t_e + 1 and never takes a wave
    neighbour with it; the raw device call covers its steps t <= t_e only, and the completed
    result is the dense curve's."""
    import torch
    from online_convex_optimization_amd import _lib
    f, edits, _ = F.cert_case(d)
    Bc, Tc = f.y.shape
    assert (Bc, Tc) == (37, 130)
    db = eng.DeviceBatch(Bc, Tc, d, lanes_per_seq=P).pack(f.z, f.y)
    assert (db.L.P, db.L.chain) == (P, 0)
    out = host(db.simulate_alg_curve(np.arange(1, Tc + 1), flag, f.eta0, closed_comparator=True))
    want = reference_of(out["regret"], out["closed"], CERT_CHECKPOINTS)
    want_open = np.full(Bc, Tc + 1, dtype=np.int64)
    for b, (_, _, te) in edits.items():
        want_open[b] = te + 1
    assert np.array_equal(want["open_from"], want_open)   # the reference agrees with the edits

    # the raw device call
    K = len(CERT_CHECKPOINTS)
    with torch.cuda.device(db.device), db._on_stream():
        ckd = torch.as_tensor(np.asarray(CERT_CHECKPOINTS, dtype=np.int64)).to(db.device)
        sup = torch.full((Bc, K), 7.0, dtype=torch.float64, device=db.device)
        arg = torch.full((Bc, K), -7, dtype=torch.int64, device=db.device)
        opn = torch.full((Bc,), -7, dtype=torch.int64, device=db.device)
    db._call("ocx_dev_simulate_alg_anytime", db._lp(), db.z.data_ptr(), db._y.data_ptr(), flag,
             float(f.eta0), ckd.data_ptr(), K, sup.data_ptr(), arg.data_ptr(), opn.data_ptr(),
             None, _lib.OCX_ALG_CLOSED_COMPARATOR, db._sp)
    raw = host({"sup": sup, "argsup": arg, "open_from": opn})
    assert np.array_equal(raw["open_from"], want_open)
    S = db.L.S
    shared = [b for b in range(Bc) if b not in edits and any(e // S == b // S for e in edits)]
    assert shared or S == 1
    assert np.all(raw["open_from"][shared] == Tc + 1)
    reg = out["regret"]
    for b in range(Bc):
        for k, t in enumerate(CERT_CHECKPOINTS):
            n = min(t, int(want_open[b]) - 1)   # an edited sequence: t <= t_e only
            if n == 0:
                assert raw["sup"][b, k] == -np.inf and raw["argsup"][b, k] == 0, (b, t)
            else:
                assert raw["sup"][b, k] == reg[b, :n].max(), (b, t)
                assert raw["argsup"][b, k] == reg[b, :n].argmax() + 1, (b, t)

    # the completed result
    got = host(db.simulate_alg_anytime(CERT_CHECKPOINTS, flag, f.eta0, closed_comparator=True,
                                       trace=True))
    assert_same(got, want, (P, d, flag))


# ------------------------------------------------------------------ 3. bit-exact mode vs the C oracle
def _oracle_check(eng, z, y, flag, eta0):
    Bn, Tn = y.shape
    got = eng.simulate_alg_anytime_batch(z, y, None, flag, eta0, lanes_per_seq=1,
                                         return_trace=True)
    assert got["sup"].shape == got["argsup"].shape == (Bn, 1)
    ref = np.array([[O.simulate_alg_full(z[b, :t], y[b, :t], flag, eta0)[0]
                     for t in range(1, Tn + 1)] for b in range(Bn)])
    assert np.array_equal(got["trace"], ref, equal_nan=False)
    assert np.array_equal(got["sup"][:, 0], ref.max(axis=1))
    assert np.array_equal(got["argsup"][:, 0], ref.argmax(axis=1) + 1)


@pytest.mark.parametrize("flag", (0, 1))
def test_bit_exact_mode_equals_the_oracle(eng, flag):
    f = F.make("gt_like" if flag == 0 else "small", 9, 40, 5, 77)
    _oracle_check(eng, f.z, f.y, flag, f.eta0)


@pytest.mark.parametrize("flag", (0, 1))
def test_bit_exact_mode_on_the_flip_sequence(eng, flag):
    from online_convex_optimization_amd import sequence_generation as SG
    z1, y1, _ = SG.flip_sequence(40, 5)
    z = np.repeat(z1[None].astype(np.float64), 9, axis=0)
    y = np.repeat(y1[None].astype(np.float64), 9, axis=0)
    _oracle_check(eng, z, y, flag, eng.SQRT2)


# ------------------------------------------------------------------ 4. padding and short horizons
@pytest.mark.parametrize("Tn", (1, 2, 67))
@pytest.mark.parametrize("Bn", (9, 70))
def test_padding_and_short_horizons(eng, Bn, Tn):
    """8 x 8 holds eight sequences per wave: the last group is partly padding.  K = 1 with the
    default [T]."""
    f = F.make("gt_like", Bn, Tn, 64, 900 + Bn)
    db = eng.DeviceBatch(Bn, Tn, 64, lanes_per_seq=8).pack(f.z, f.y)
    assert (db.L.P, db.L.S) == (8, 8) and Bn % 8 != 0
    got = host(db.simulate_alg_anytime(None, 0, f.eta0, trace=True))
    assert got["sup"].shape == (Bn, 1)
    assert_same(got, dense_reference(db, 0, f.eta0, [Tn]), (Bn, Tn))
    assert np.all(got["open_from"] == Tn + 1)


def test_no_horizon(eng):
    db = eng.DeviceBatch(9, 0, 64, lanes_per_seq=8)
    for cks in ([], None):
        got = host(db.simulate_alg_anytime(cks, trace=True))
        assert got["sup"].shape == got["argsup"].shape == (9, 0)
        assert got["trace"].shape == (9, 0) and np.all(got["open_from"] == 1)
    with pytest.raises(ValueError):
        db.simulate_alg_anytime([0])
    # K = 0 at T > 0: the trace alone
    f = F.make("gt_like", 9, 5, 64, 3)
    db = eng.DeviceBatch(9, 5, 64, lanes_per_seq=8).pack(f.z, f.y)
    got = host(db.simulate_alg_anytime([], 0, f.eta0, trace=True))
    want = dense_reference(db, 0, f.eta0, [])
    assert got["sup"].shape == (9, 0)
    assert np.array_equal(got["trace"], want["trace"])
    assert np.array_equal(got["open_from"], want["open_from"])


# ------------------------------------------------------------------ 5. g(T) layer
def test_gT_anytime(eng):
    cks = [50, 100, 200]
    sup, arg = eng.gT_anytime(200, 20, cks, d=64, batch=8)   # 8 + 8 + 4 runs
    assert sup.shape == arg.shape == (20, 3) and arg.dtype == np.int64
    for r0, n in ((0, 8), (8, 8), (16, 4)):
        db = eng.DeviceBatch(n, 200, 64)
        db.generate_gT(0, r0)
        res = host(db.simulate_alg_anytime(cks))
        assert np.all(res["open_from"] == 201)
        assert np.array_equal(sup[r0:r0 + n], res["sup"])
        assert np.array_equal(arg[r0:r0 + n], res["argsup"])
        want = dense_reference(db, 0, eng.SQRT2, cks)
        assert np.array_equal(res["sup"], want["sup"])
        assert np.array_equal(res["argsup"], want["argsup"])
    curves = eng.gT_regret_curves(200, 20, cks, d=64, batch=8)
    assert np.all(sup >= curves)
    assert np.all(np.diff(sup, axis=1) >= 0) and np.all(np.diff(arg, axis=1) >= 0)
    assert np.all((arg >= 1) & (arg <= np.asarray(cks)[None, :]))
    env = eng.gT_anytime_max(200, 20, cks, d=64, batch=8)
    assert env.shape == (3,)
    assert np.array_equal(env, np.maximum(0.0, sup.max(axis=0)))
    assert np.all(np.diff(env) >= 0)
