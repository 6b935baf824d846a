"""Regret-grid timing probe: what M step sizes x K checkpoints cost through
simulate_alg_curve_etas, for every forced group size, next to existing code on the same
resident batch.  One JSON line per case, appended to profiles/grid_ab.jsonl (or --out).

Baselines, never the grid:
  loop   M calls of simulate_alg_curve (what the grid replaces);
  etas   simulate_alg_etas at the same M with no checkpoints (the observer's own cost).
Every timed grid's columns are compared bit for bit with the loop's at the timed size.

Shapes (tools/etas_probe.py's classes):
  a  the bench batch 32 768 x 1e4 x 64 at 8 x 8: M = 2 and 4 with K = 10 (1000 … 10 000), and
     K = 100 once (M = 4);
  b  65 536 x 1e3 x 5 in OCX_LANES_BEST and in exact mode, and 65 536 x 1e3 x 16: M = 4,
     K = 10 (100 … 1000);
  d  one chained exact class (4 x 16 at d = 64), the few-wave 3 328 x 1e5 x 64 at 16 x 4;
  e  the further layout classes of tools/etas_probe.py's case d: M = 4, K = 10;
  u  uncertified triples: `beam`-like rows (norm 1.6) at 8 192 x 2 000 x 64, closed form
     requested, so every triple streams its prefix through the comparator kernel;
  c  gT_regret_curves_etas(1e4, 32 768, 10 checkpoints, 4 step sizes, d = 64) against four
     gT_regret_curves calls (host clock around synchronous calls, the sides one after the
     other: each keeps a 170 GB batch resident).

One process; device events on the batch's stream around every repetition; every shape warmed
up; the sides of a comparison alternate repetition by repetition.  --small runs toy sizes (a
rehearsal of the script, not a measurement)."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from etas_probe import ETAS8, alternate, stats  # noqa: E402
from online_convex_optimization_amd import _lib, engine  # noqa: E402

KEYS = ("regret", "cum", "comp", "closed")


def beam_rows(db, B, T, d, chunk=256):
    """`beam`-like rows (tests/_etas_cases.py: 1.6 s u + 0.3 n, labels ±1) packed into db, made
    on the device in chunks of sequences."""
    g = torch.Generator(device=db.device).manual_seed(4000 + d)
    z = torch.empty((B, T, d), dtype=torch.float64, device=db.device)
    y = torch.empty((B, T), dtype=torch.float64, device=db.device)
    for b0 in range(0, B, chunk):
        n = min(chunk, B - b0)
        u = torch.randn((n, 1, d), generator=g, dtype=torch.float64, device=db.device)
        u /= u.norm(dim=2, keepdim=True)
        s = torch.where(torch.rand((n, T, 1), generator=g, device=db.device) < 0.5, -1.0, 1.0)
        nz = torch.randn((n, T, d), generator=g, dtype=torch.float64, device=db.device)
        nz /= nz.norm(dim=2, keepdim=True)
        z[b0:b0 + n] = 1.6 * s * u + 0.3 * nz
        y[b0:b0 + n] = torch.where(torch.rand((n, T), generator=g, device=db.device) < 0.5,
                                   -1.0, 1.0)
    db.pack(z, y)
    torch.cuda.synchronize()
    return db


def resident(out, case, B, T, d, reps, lanes, Ms, K, beam=False):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes)
    if beam:
        beam_rows(db, B, T, d)
        cc = True
    else:
        db.generate_gT(base_seed=0)
        cc = not db.exact   # both sides: the batch's default comparator
    lib = _lib.load()
    cks = [T * (k + 1) // K for k in range(K)]
    groups = [g for g in (1, 2, 4) if g == 1 or db.L.C <= 8 or (g == 2 and db.L.C <= 16)]
    for M in Ms:
        etas = ETAS8[:M]
        res = {}

        def loop(etas=etas):
            res["loop"] = [db.simulate_alg_curve(cks, 0, eta, closed_comparator=cc)
                           for eta in etas]

        sides = {"loop": loop,
                 "etas": lambda etas=etas: db.simulate_alg_etas(etas, closed_comparator=cc)}
        for g in groups + [None]:
            name = "auto" if g is None else f"group{g}"
            sides[name] = (lambda g=g, name=name, etas=etas: res.__setitem__(
                name, db.simulate_alg_curve_etas(cks, etas, closed_comparator=cc, _group=g)))
        ms = alternate(sides, reps)
        torch.cuda.synchronize()
        base, sweep = stats(ms["loop"]), stats(ms["etas"])
        closed = res["loop"][0]["closed"]
        rec = {"case": case, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "rows": "beam" if beam else "gT", "closed_comparator": cc, "M": M, "K": K,
               "auto_group": int(lib.ocx_curve_etas_group(ctypes.byref(db.L), M)),
               "closed_share_eta0": float(closed.double().mean()) if closed.numel() else 1.0,
               "loop": base, "etas_no_checkpoints": sweep}
        for name in sides:
            if name in ("loop", "etas"):
                continue
            s = stats(ms[name])
            same = all(torch.equal(res[name][k][:, m, :], res["loop"][m][k])
                       for m in range(M) for k in KEYS)
            rec[name] = dict(s, ratio_median=s["median_ms"] / base["median_ms"],
                             ratio_to_etas=s["median_ms"] / sweep["median_ms"],
                             inside_loop_spread=base["min_ms"] <= s["median_ms"] <= base["max_ms"],
                             columns_equal_the_loop=bool(same))
        out(rec)
        res.clear()
    del db


def case_c(out, T, runs, d, reps):
    etas = ETAS8[:4]
    cks = [T * (k + 1) // 10 for k in range(10)]

    def host_timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def four():
        return np.stack([engine.gT_regret_curves(T, runs, cks, d=d, eta0=eta) for eta in etas],
                        axis=1)

    def grid():
        return engine.gT_regret_curves_etas(T, runs, cks, etas, d=d, return_closed=True)

    host_timed(four)   # warm-up
    a = [host_timed(four) for _ in range(reps)]
    torch.cuda.empty_cache()
    host_timed(grid)   # warm-up
    b = [host_timed(grid) for _ in range(reps)]
    ref, (got, closed) = a[-1][1], b[-1][1]
    base, s = stats([x[0] for x in a]), stats([x[0] for x in b])
    L = _lib.layout(runs, T, d, engine.LANES_BEST)
    out({"case": "c", "runs": runs, "T": T, "d": d, "layout": [L.P, L.C, L.chain], "M": 4, "K": 10,
         "auto_group": int(_lib.load().ocx_curve_etas_group(ctypes.byref(L), 4)),
         "four_gT_regret_curves": base, "gT_regret_curves_etas": s,
         "ratio_median": s["median_ms"] / base["median_ms"],
         "all_closed": bool((closed == 1).all()), "regrets_bit_equal": bool(np.array_equal(got, ref))})
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "grid_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="abdeuc")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def out(rec):
        rec["small"] = a.small
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    def size(B, T):
        return (max(B // 16, 64), max(T // 50, 20)) if a.small else (B, T)

    best = engine.LANES_BEST
    engine.release_buffers(0)
    if "a" in a.cases:
        B, T = size(32768, 10000)
        resident(out, "a", B, T, 64, a.reps, best, (2, 4), 10)
        torch.cuda.empty_cache()
        resident(out, "a", B, T, 64, a.reps, best, (4,), 100 if not a.small else 20)
        torch.cuda.empty_cache()
    if "b" in a.cases:
        B, T = size(65536, 1000)
        for d, lanes in ((5, best), (5, 1), (16, best)):
            resident(out, "b", B, T, d, a.reps, lanes, (4,), 10)
            torch.cuda.empty_cache()
    if "d" in a.cases:
        for B, T, d, lanes in ((32768, 10000, 64, 1), (3328, 100000, 64, 128)):
            B, T = size(B, T)
            resident(out, "d", B, T, d, a.reps, lanes, (4,), 10)
            torch.cuda.empty_cache()
    if "e" in a.cases:
        # further classes of tools/etas_probe.py's table: pipelined 8 x 4, 32 x 8 and 16 x 16;
        # chained 2 x 16, 4 x 2 and the few-wave 8 x 8 chain; butterfly lanes the pipelined form
        # does not take (2 x 4); one lane of 12 coordinates
        for B, T, d, lanes in ((65536, 5000, 32, 8), (8192, 5000, 256, 32), (8192, 10000, 200, 128),
                               (65536, 1000, 32, 128), (65536, 1000, 5, -4), (4900, 20000, 64, 1),
                               (65536, 1000, 5, 2), (65536, 1000, 12, -1)):
            B, T = size(B, T)
            resident(out, "e", B, T, d, a.reps, lanes, (4,), 10)
            torch.cuda.empty_cache()
    if "u" in a.cases:
        B, T = size(8192, 2000)
        resident(out, "u", B, T, 64, a.reps, best, (4,), 10, beam=True)
        torch.cuda.empty_cache()
    if "c" in a.cases:
        case_c(out, *((1000, 4096, 64) if a.small else (10000, 32768, 64)), max(3, a.reps // 2))


if __name__ == "__main__":
    main()
