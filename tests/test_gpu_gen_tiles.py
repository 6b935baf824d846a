"""Conformance of the g(T) generator (csrc/ocx_gen_wave.hip): every byte of z_tiled, y_tiled
and y_bits against tiles built on the host from NumPy's own streams (tests/_tiles.py), with
the launch shrunk to a handful of waves so that every wave runs many sequences.

A launch spreads G*S sequence slots over `resident` = CUs x waves-per-CU waves and wave w runs
slots w, w + nwaves, ...; on a whole device `resident` is in the thousands, so at test sizes
the per-sequence loop makes one trip.  OCX_GEN_CUS and OCX_GEN_WAVES_PER_SIMD (read by the
launcher at every launch) shrink `resident` to 4 (CUS=1) or 12 (CUS=3): the second and later
trips — the reset of the ring and lane states, the re-seeding, the padding-sequence branch
with its staged label rounds, the label-bit words of a later sequence, the d = 1024 spill
move — are then compared with NumPy byte for byte.

Every assertion on generator output is equality of 64-bit patterns over the whole buffer
(prefilled with a payload NaN / all-ones), so a -0.0 or a stale word in padding fails.

Two test-only entry points (include/ocx_testing.h) reach the launchers that the product only
reaches through pipelines: ocx_test_gen_gT_range (one launch of the overlapped pipeline's
sub-batch generator: forms 3, 4 and the few-stream 6) and ocx_test_gen_gT_rows (one launch of
the trailing pipeline's row-range generator with resumed streams)."""
import ctypes
import functools

import numpy as np
import pytest

from tests._tiles import expected_gT_tiles, gT_rows, slots_y, slots_z

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF80000DEADBEEF  # a quiet NaN no kernel produces: the prefill of z and y
ONES = -1                      # the prefill of y_bits and of the stream-state buffers (int64)


@pytest.fixture(scope="module")
def ocx():
    from online_convex_optimization_amd import _lib, engine
    assert _lib.device_count() >= 1
    return {"lib": _lib, "engine": engine}


# ---------------------------------------------------------------- host side
@functools.lru_cache(maxsize=2)
def _rows(base_seed, run0, B, T, d):
    z, y = gT_rows(base_seed, run0, B, T, d)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def expected(base_seed, run0, L):
    """The three tiles as int64 patterns (the rows shared by the cases of one shape)."""
    zt, yt, bits = expected_gT_tiles(base_seed, run0, L,
                                     rows=_rows(base_seed, run0, int(L.B), int(L.T), int(L.d)))
    return zt.view(np.int64), yt.view(np.int64), bits.view(np.int64)


def forced_waves(L, cus, form):
    """Waves of a launch_wave_df launch under OCX_GEN_CUS=cus, OCX_GEN_WAVES_PER_SIMD=1 (the
    launcher's arithmetic: 4 resident waves per CU, whole blocks of 4 waves, 8 in the default
    d = 64 form).  For the failure report and the table of forced shares only."""
    knw = 8 if (L.d == 64 and L.P * L.C == 64 and form != "lr") else 4
    nseq = int(L.G * L.S)
    per_wave = -(-nseq // (4 * cus))
    return -(-(-(-nseq // per_wave)) // knw) * knw


def slots_bits(w, L):
    """y_bits [g][k][s] → [G*S, ceil(T/64)]."""
    G, S, KB = int(L.G), int(L.S), (int(L.T) + 63) // 64
    return np.asarray(w)[:G * KB * S].reshape(G, KB, S).transpose(0, 2, 1).reshape(G * S, KB)


def assert_tiles_equal(got, want, L, nwaves=None, what=""):
    """got / want: (z, y, bits) int64 patterns over the whole buffers (bits may be None)."""
    for name, g, w, slots in (("z_tiled", got[0], want[0], slots_z), ("y_tiled", got[1], want[1], slots_y),
                              ("y_bits", got[2], want[2], slots_bits)):
        if g is None:
            continue
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if np.array_equal(g, w):
            continue
        gs, ws = slots(g, L), slots(w, L)
        idx = np.argwhere(gs != ws)
        b = int(idx[0][0])
        where = dict(zip(("sequence", "step" if name != "y_bits" else "block", "coordinate"),
                         (int(v) for v in idx[0])))
        trip = ("one-trip launch" if nwaves is None
                else f"trip {b // nwaves} of wave {b % nwaves} ({nwaves} waves)")
        pytest.fail(f"{what}{name}: {len(idx)} of {gs.size} words differ in {len(set(idx[:, 0].tolist()))} "
                    f"sequence slots; first at {where} ({'padding' if b >= L.B else 'real'} sequence, "
                    f"{trip}): got {int(gs[tuple(idx[0])]):#018x}, want {int(ws[tuple(idx[0])]):#018x}")


def read_back(db):
    return (db.z.cpu().numpy().view(np.int64), db._y.cpu().numpy().view(np.int64),
            db._ybits.cpu().numpy())


def new_batch(ocx, B, T, d, lanes, P, C):
    import torch
    db = ocx["engine"].DeviceBatch(B, T, d, lanes_per_seq=lanes)
    assert (db.L.P, db.L.C) == (P, C), db.L
    assert db.z.numel() == db.L.z_elems and db._y.numel() == db.L.y_elems
    db.z.view(torch.int64).fill_(NAN_BITS)
    db._y.view(torch.int64).fill_(NAN_BITS)
    db._ybits.fill_(ONES)
    torch.cuda.synchronize()
    return db


def set_knobs(monkeypatch, cus, form=None):
    monkeypatch.setenv("OCX_GEN_ROUNDS", "0")
    if form is not None:
        monkeypatch.setenv("OCX_GEN_FORM", form)
    else:
        monkeypatch.delenv("OCX_GEN_FORM", raising=False)
    if cus is None:
        monkeypatch.delenv("OCX_GEN_CUS", raising=False)
        monkeypatch.delenv("OCX_GEN_WAVES_PER_SIMD", raising=False)
    else:
        monkeypatch.setenv("OCX_GEN_CUS", str(cus))
        monkeypatch.setenv("OCX_GEN_WAVES_PER_SIMD", "1")


# ---------------------------------------------------------------- the single-launch forms
# Per form (the dispatch of launch_wave): layouts (d, lanes_per_seq, P, C, B), the T edges (the
# rows-per-batch boundaries of the form and the label rounds: 128 labels per round, the
# buffered half-draw at odd T), one extra shape of >= 1e6 normals where the others stay below
# (the ziggurat tail: a few hundred draws per 1e6), and the B = 1 shape.  B: 70 at S = 64, 32,
# 16 and 4, 203 at S = 8, 71 at S = 2, 37 at S = 1 — B % S != 0 (padding sequences) and G*S at
# least three times the 12 (16) forced waves of CUS=3; G*S odd at S = 1, so no staged labels.
# C is what ocx_layout_init gives: butterfly layouts round ceil(d / P) up to a supported width
# (2, 4, 6, 8, 12, 16, 24, 32, 48, 64), so 9 coordinates per lane are held in 12, 13 in 16.
FORMS = {
    # DF = 0, d < 8: one lane per row, 32-row batches
    "df0_lt8": dict(layouts=[(1, -1, 1, 2, 70), (5, -1, 1, 6, 70), (5, -4, 4, 2, 70), (7, -1, 1, 8, 70)],
                    Ts=[1, 31, 32, 33, 97, 129], extra=[(5, -4, 4, 2, 2006, 129), (5, -1, 1, 6, 1, 33)]),
    # DF = 0, 8 <= d <= 32: leaf sums, 8-row batches, RP > 1 stores
    "df0_8to32": dict(layouts=[(8, 4, 4, 2, 70), (8, -1, 1, 8, 70), (9, -1, 1, 12, 70), (12, 2, 2, 6, 70),
                               (16, 16, 16, 2, 70)],
                      Ts=[1, 7, 8, 9, 128, 257], extra=[(8, 4, 4, 2, 550, 257), (8, 4, 4, 2, 1, 9)]),
    # DF = 0, 32 < Dp <= 64: RP == 1 stores
    "df0_33to64": dict(layouts=[(33, 4, 4, 12, 70)], Ts=[1, 9, 130],
                       extra=[(33, 4, 4, 12, 250, 130), (33, 4, 4, 12, 1, 9)]),
    # DF = 0, Dp > 64: zaddr stores, 2-row batches up to d = 128
    "df0_gt64": dict(layouts=[(64, 64, 64, 2, 37), (65, 8, 8, 12, 203), (100, 8, 8, 16, 203),
                              (127, 8, 8, 16, 203), (128, 8, 8, 16, 203)],
                     Ts=[1, 2, 3, 129], extra=[(65, 8, 8, 12, 1, 3)]),
    # DF = 0, d > 128: pairwise stack, one row per batch
    "df0_gt128": dict(layouts=[(129, 16, 16, 12, 70), (130, 16, 16, 12, 70), (257, 32, 32, 12, 71),
                               (1000, 32, 32, 32, 71)],
                      Ts=[1, 2, 65], extra=[(129, 16, 16, 12, 1, 2)]),
    # DF = 16 / 32: 512-normal batches of 32 / 16 rows
    "df16_32": dict(layouts=[(16, 8, 8, 2, 203), (16, 4, 4, 4, 70), (16, -1, 1, 16, 70), (32, 8, 8, 4, 203),
                             (32, 2, 2, 16, 70)],
                    Ts=[1, 15, 16, 17, 31, 32, 33, 129, 300], extra=[(16, 8, 8, 2, 1, 17)]),
    # DF = 64, both forms (OCX_GEN_FORM)
    "df64": dict(layouts=[(64, -4, 4, 16, 70), (64, 8, 8, 8, 203), (64, 16, 16, 4, 70), (64, 32, 32, 2, 71)],
                 Ts=[1, 7, 8, 9, 127, 128, 129, 300], extra=[(64, 8, 8, 8, 1, 9)],
                 gen_forms=["default", "lr"]),
    # DF = 1024: the P <= 32 store map and the P = 64 branch, the spill move between rows
    "df1024": dict(layouts=[(1024, 16, 16, 64, 9), (1024, 32, 32, 32, 9), (1024, 64, 64, 16, 9),
                            (1024, 16, 16, 64, 40), (1024, 32, 32, 32, 40), (1024, 64, 64, 16, 40)],
                   Ts=[1, 2, 9, 130], extra=[(1024, 32, 32, 32, 1, 9)]),
}
# the knobs-unset run of each form (today's one-trip launch): a failure of the forced runs
# beside a pass here isolates the trip loop
UNSET = {"df0_lt8": (5, -4, 4, 2, 70, 129), "df0_8to32": (12, 2, 2, 6, 70, 257),
         "df0_33to64": (33, 4, 4, 12, 70, 130), "df0_gt64": (100, 8, 8, 16, 203, 129),
         "df0_gt128": (257, 32, 32, 12, 71, 65), "df16_32": (32, 8, 8, 4, 203, 300),
         "df64": (64, 8, 8, 8, 203, 300), "df1024": (1024, 32, 32, 32, 40, 130)}


def _single_launch_cases():
    out = []
    for name, f in FORMS.items():
        shapes = [(d, lanes, P, C, B, T) for (d, lanes, P, C, B) in f["layouts"] for T in f["Ts"]]
        shapes += f["extra"]
        for gen_form in f.get("gen_forms", [None]):
            tag = name + ("_" + gen_form if gen_form else "")
            for (d, lanes, P, C, B, T) in shapes:
                for cus in (1, 3):
                    out.append(pytest.param(d, lanes, P, C, B, T, gen_form, cus,
                                            id=f"{tag}-d{d}P{P}C{C}-B{B}-T{T}-cus{cus}"))
            d, lanes, P, C, B, T = UNSET[name]
            out.append(pytest.param(d, lanes, P, C, B, T, gen_form, None,
                                    id=f"{tag}-d{d}P{P}C{C}-B{B}-T{T}-unset"))
    return out


@pytest.mark.parametrize("d,lanes,P,C,B,T,gen_form,cus", _single_launch_cases())
def test_generator_tiles_equal_numpy(ocx, monkeypatch, d, lanes, P, C, B, T, gen_form, cus):
    import torch
    db = new_batch(ocx, B, T, d, lanes, P, C)
    set_knobs(monkeypatch, cus, gen_form)
    base_seed, run0 = 5, 7
    db.generate_gT(base_seed, run0)
    torch.cuda.synchronize()
    nwaves = None if cus is None else forced_waves(db.L, cus, gen_form)
    assert_tiles_equal(read_back(db), expected(base_seed, run0, db.L), db.L, nwaves)


# ---------------------------------------------------------------- the sub-batch range launcher
def three_ranges(L):
    """G*S split into three unequal ranges, offsets and sizes multiples of 4, launched out of
    order."""
    n = int(L.G * L.S)
    assert n > 68 and n % 4 == 0
    return [(68, n - 68), (0, 64), (64, 4)]


RANGE_LAYOUTS = [(64, 8, 8, 8, 203), (64, 16, 16, 4, 202), (32, 8, 8, 4, 203), (16, 8, 8, 2, 203)]


@pytest.mark.parametrize("T", [1, 130, 257])
@pytest.mark.parametrize("form", [3, 4, 6])
@pytest.mark.parametrize("d,lanes,P,C,B", RANGE_LAYOUTS)
def test_range_launches_fill_their_slots_only(ocx, monkeypatch, d, lanes, P, C, B, form, T):
    lib = ocx["lib"]
    set_knobs(monkeypatch, None)
    db = new_batch(ocx, B, T, d, lanes, P, C)
    L = db.L
    assert L.G * L.S > B  # padding sequences in the last range
    base_seed, run0 = 11, 3
    ptrs = (db.z.data_ptr(), db._y.data_ptr(), db._ybits.data_ptr(), None)
    if form == 6 and d != 64:
        # the few-stream range launcher is the d = 64 form's: an error, nothing written
        with pytest.raises(ValueError):
            lib.call("ocx_test_gen_gT_range", ctypes.byref(L), base_seed, run0, 0, 64, form, *ptrs)
        assert_untouched(read_back(db), L, np.zeros(L.G * L.S, dtype=bool))
        return
    want = expected(base_seed, run0, L)
    done = np.zeros(L.G * L.S, dtype=bool)
    for b_off, nseq in three_ranges(L):
        lib.call("ocx_test_gen_gT_range", ctypes.byref(L), base_seed, run0, b_off, nseq, form, *ptrs)
        done[b_off:b_off + nseq] = True
        got = read_back(db)
        assert_untouched(got, L, done)
    assert done.all()
    assert_tiles_equal(got, want, L, what=f"form {form}: ")


def assert_untouched(got, L, done):
    """Every slot of the sequences not yet launched still holds the prefill."""
    z, y, bits = slots_z(got[0], L), slots_y(got[1], L), slots_bits(got[2], L)
    rest = ~done
    assert (z[rest] == NAN_BITS).all(), ("z slots of unlaunched sequences written",
                                         np.argwhere(z[rest] != NAN_BITS)[:3].tolist())
    assert (y[rest] == NAN_BITS).all(), "y slots of unlaunched sequences written"
    assert (bits[rest] == ONES).all(), "label-bit words of unlaunched sequences written"


@pytest.mark.parametrize("form", [3, 4, 6])
def test_range_launcher_rejections_write_nothing(ocx, monkeypatch, form):
    lib = ocx["lib"]
    set_knobs(monkeypatch, None)
    db = new_batch(ocx, 203, 130, 64, 8, 8, 8)
    L = db.L
    nothing = np.zeros(L.G * L.S, dtype=bool)
    ptrs = (db.z.data_ptr(), db._y.data_ptr(), db._ybits.data_ptr(), None)
    # b_off % 4, nseq % 4 (the launcher's), a range past the layout's slots (the entry point's)
    for b_off, nseq in ((2, 64), (64, 6), (3, 5), (204, 8), (-4, 8), (0, 212)):
        with pytest.raises(ValueError):
            lib.call("ocx_test_gen_gT_range", ctypes.byref(L), 1, 2, b_off, nseq, form, *ptrs)
    with pytest.raises(ValueError):  # not a form
        lib.call("ocx_test_gen_gT_range", ctypes.byref(L), 1, 2, 0, 64, 5, *ptrs)
    assert_untouched(read_back(db), L, nothing)
    # a d = 64 layout whose lanes the row does not fill (P*C = 128 != d)
    dw = new_batch(ocx, 37, 130, 64, 64, 64, 2)
    with pytest.raises(ValueError):
        lib.call("ocx_test_gen_gT_range", ctypes.byref(dw.L), 1, 2, 0, 36, form, dw.z.data_ptr(),
                 dw._y.data_ptr(), dw._ybits.data_ptr(), None)
    assert_untouched(read_back(dw), dw.L, np.zeros(dw.L.G * dw.L.S, dtype=bool))


# ---------------------------------------------------------------- the row-range launcher
CUTS_64 = {300: [0, 64, 128, 256, 300], 130: [0, 64, 128, 130]}      # the trailing pipeline's kind
CUTS_ODD = {300: [0, 1, 8, 65, 299, 300], 130: [0, 1, 8, 65, 129, 130]}
# (d, lanes, P, C, B, T, OCX_GEN_FORM)
ROWS_LAYOUTS = [(64, 8, 8, 8, 203, 300, "default"), (64, 16, 16, 4, 70, 300, "lr"),
                (5, -4, 4, 2, 70, 130, None), (16, 8, 8, 2, 203, 130, None),
                (1024, 32, 32, 32, 9, 130, None)]


@pytest.mark.parametrize("cus", [None, 1], ids=["unset", "cus1"])
@pytest.mark.parametrize("cuts", ["cuts64", "cutsodd"])
@pytest.mark.parametrize("d,lanes,P,C,B,T,gen_form", ROWS_LAYOUTS)
def test_row_ranges_resume_the_streams(ocx, monkeypatch, d, lanes, P, C, B, T, gen_form, cuts, cus):
    """The trailing pipeline's chain (ocx_run_gen_sim_trailing): the first launch seeds fresh
    streams, each later one resumes from the state the one before saved (two alternating
    buffers), only the last draws the labels and it saves no state."""
    import torch
    lib = ocx["lib"]
    set_knobs(monkeypatch, cus, gen_form)
    db = new_batch(ocx, B, T, d, lanes, P, C)
    L = db.L
    base_seed, run0 = 2, 9
    want = expected(base_seed, run0, L)
    wz = slots_z(want[0], L)
    nwaves = None if cus is None else forced_waves(L, cus, gen_form)
    states = [torch.full((6 * int(L.G * L.S),), ONES, dtype=torch.int64, device=db.device)
              for _ in range(2)]
    edges = (CUTS_64 if cuts == "cuts64" else CUTS_ODD)[T]
    n = len(edges) - 1
    for i in range(n):
        t0, t1 = edges[i], edges[i + 1]
        last = i == n - 1
        st_in = states[(i + 1) % 2].data_ptr() if i > 0 else None
        st_out = states[i % 2].data_ptr() if not last else None
        lib.call("ocx_test_gen_gT_rows", ctypes.byref(L), base_seed, run0, t0, t1 - t0, st_in, st_out,
                 1 if last else 0, db.z.data_ptr(), db._y.data_ptr(), None)
        if last:
            break
        gz, gy, _ = read_back(db)
        z = slots_z(gz, L)
        assert (z[:, t1:] == NAN_BITS).all(), f"launch {i} wrote rows past {t1}"
        assert (gy == NAN_BITS).all(), f"launch {i} (labels = 0) wrote the label tile"
        if not np.array_equal(z[:, :t1], wz[:, :t1]):
            idx = np.argwhere(z[:, :t1] != wz[:, :t1])
            pytest.fail(f"rows [0, {t1}) after launch {i} [{t0}, {t1}): {len(idx)} words differ, first "
                        f"at (sequence, step, coordinate) {idx[0].tolist()}")
    gz, gy, _ = read_back(db)
    assert_tiles_equal((gz, gy, None), want, L, nwaves, what=f"cuts {edges}: ")


def test_row_range_rejections_write_nothing(ocx, monkeypatch):
    lib = ocx["lib"]
    set_knobs(monkeypatch, None)
    db = new_batch(ocx, 70, 130, 5, -4, 4, 2)
    L = db.L
    for t_off, nrows in ((-1, 8), (128, 3), (131, 1)):
        with pytest.raises(ValueError):
            lib.call("ocx_test_gen_gT_rows", ctypes.byref(L), 1, 2, t_off, nrows, None, None, 1,
                     db.z.data_ptr(), db._y.data_ptr(), None)
    with pytest.raises(ValueError):  # labels is a flag
        lib.call("ocx_test_gen_gT_rows", ctypes.byref(L), 1, 2, 0, 8, None, None, 2, db.z.data_ptr(),
                 db._y.data_ptr(), None)
    gz, gy, _ = read_back(db)
    assert (gz == NAN_BITS).all() and (gy == NAN_BITS).all()
