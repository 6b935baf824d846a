"""SMART regret-grid timing probe: what M thresholds x K checkpoints cost through
simulate_smart_grid, for every forced group size of both kernels, next to existing code on the
same resident generate_gT batch.  One JSON line per case, appended to
profiles/smart_grid_ab.jsonl (or --out).

The yardstick is existing code, never the grid's own group 1: DeviceBatch.simulate_smart_curve
on the M·K (horizon, threshold) pairs sorted by horizon (`pairs`).  Every timed grid is compared
bit for bit with it at the timed size.

  (a) the layout classes of tools/smart_curve_probe.py at 32 768 x 1e3, both closed forms on
      both sides, M in {2, 4, 7}, ten horizons 100 … 1000: lane-group groups 1, 2, 4 (forced
      through include/ocx_testing.h) and the dispatcher's own choice;
  (w) 2 048 x 1e3 x {5, 16, 32} and 32 768 x 1e3 x 5 in the bit-exact one-lane layout with
      flags 0 (the reference's prefix re-scan), M in {2, 4, 7}: the one-wave-per-sequence grid
      at groups 1, 2, 4, 8, the lane-group grid, and the dispatcher's choice;
  (x) 2 048 x 1e3 x 64 in the two exact layouts (one lane; 4 x 16 chained) with flags 0,
      M in {2, 4}: the class in which the sweeps' rule (ocx_smart_wave_cols_worth) keeps M
      columns on the lane-group kernel while the pair list's M·K columns take the wave form;
  (r) the ring refill: K = 100 horizons against K = 10 on the bench-shaped batch
      (32 768 x 1e4 x 64, OCX_LANES_BEST, both closed forms, M = 4).

Thresholds: 0.5 sqrt(T (m + 1) / (M + 1)) — on these rows a threshold th switches near 4 th², so
the columns' switches spread over the horizon; the records carry the mean switch steps.  One
process; device events on the stream around every repetition; two warm-up rounds; the sides of
a comparison alternate repetition by repetition.  The spread reported is the yardstick's in the
same call.  --small runs toy sizes (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smart_curve_probe import SQ2, alternate, stats  # noqa: E402
from online_convex_optimization_amd import _lib, engine  # noqa: E402


def thresholds(T, M):
    return [0.5 * math.sqrt(T * (m + 1) / (M + 1)) for m in range(M)]


def resident(out, case, B, T, d, reps, lanes, closed, Ms, K, wave, lane_groups=(1, 2, 4)):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    lib = _lib.load()
    cks = [T * (k + 1) // K for k in range(K)]
    for M in Ms:
        ths = thresholds(T, M)
        hz = [t for t in cks for _ in range(M)]
        pth = [th for _ in cks for th in ths]
        kw = dict(closed_prefix=closed, closed_comparator=closed)
        res = {}
        sides = {"pairs": lambda: res.__setitem__(
            "pairs", db.simulate_smart_curve(hz, pth, SQ2, **kw))}
        for g in lane_groups:
            if lib.ocx_test_simulate_smart_grid(ctypes.byref(db.L), None, None, None, 0, None, 0,
                                                SQ2, None, None, 0, None, g, None) == 0:
                sides[f"group{g}"] = (lambda g=g: res.__setitem__(
                    f"group{g}", db.simulate_smart_grid(cks, ths, SQ2, _group=g, **kw)))
        if wave:
            for g in (1, 2, 4, 8):
                sides[f"wave{g}"] = (lambda g=g: res.__setitem__(
                    f"wave{g}", db.simulate_smart_grid(cks, ths, SQ2, _wave=g)))
        sides["auto"] = lambda: res.__setitem__("auto", db.simulate_smart_grid(cks, ths, SQ2, **kw))
        ms = alternate(sides, reps)
        torch.cuda.synchronize()
        base = stats(ms["pairs"])
        ref = {k: v.reshape(-1, K, M).transpose(1, 2) for k, v in res["pairs"].items()}
        full_sw = res["auto"]["switch_step"][:B, :, -1]
        rec = {"case": case, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "closed_forms": closed, "M": M, "K": K, "thresholds": ths,
               "auto_group": int(lib.ocx_smart_grid_group(ctypes.byref(db.L), M)),
               "mean_switch_step_per_column": [float(x) for x in
                                               full_sw.double().mean(dim=0).cpu().tolist()],
               "never_switched_per_column": [int(x) for x in (full_sw < 0).sum(dim=0).cpu().tolist()],
               "pairs": base}
        for name in sides:
            if name == "pairs":
                continue
            s = stats(ms[name])
            same = all(torch.equal(res[name][k], ref[k]) for k in ref)
            rec[name] = dict(s, ratio_median=s["median_ms"] / base["median_ms"],
                             inside_pairs_spread=base["min_ms"] <= s["median_ms"] <= base["max_ms"],
                             bit_equal_pairs=bool(same))
        out(rec)
        res.clear()
    del db


def refill(out, B, T, d, reps, lanes, M, Ks):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    ths = thresholds(T, M)
    res = {}
    sides = {}
    for K in Ks:
        cks = [T * (k + 1) // K for k in range(K)]
        sides[f"K{K}"] = (lambda K=K, cks=cks: res.__setitem__(
            K, db.simulate_smart_grid(cks, ths, SQ2, closed_prefix=True, closed_comparator=True)))
    sides["sweep"] = lambda: res.__setitem__(0, db.simulate_smart_thresholds(
        ths, SQ2, closed_prefix=True, closed_comparator=True))
    ms = alternate(sides, reps)
    torch.cuda.synchronize()
    rec = {"case": "r", "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
           "closed_forms": True, "M": M,
           "auto_group": int(_lib.load().ocx_smart_grid_group(ctypes.byref(db.L), M)),
           "last_column_equals_sweep": all(bool(torch.equal(res[K]["regret"][:, :, -1],
                                                            res[0]["regret"])) for K in Ks)}
    for name in sides:
        rec[name] = stats(ms[name])
    rec["ratio_median"] = rec[f"K{Ks[-1]}"]["median_ms"] / rec[f"K{Ks[0]}"]["median_ms"]
    out(rec)
    del db


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "smart_grid_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-w", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="awxr")
    ap.add_argument("--Ms", default="2,4,7")
    ap.add_argument("--no-lane-groups", action="store_true",
                    help="case x without the forced lane-group sides (seconds per call there)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    f = open(a.out, "a")

    def out(rec):
        rec["small"] = a.small
        line = json.dumps(rec)
        print(line, flush=True)
        f.write(line + "\n")
        f.flush()

    engine.release_buffers(0)
    k = 16 if a.small else 1
    T = 1000 // (4 if a.small else 1)
    Ms = tuple(int(m) for m in a.Ms.split(","))
    best = engine.LANES_BEST
    if "a" in a.cases:
        # tools/smart_curve_probe.py's cases a and c: the dispatcher's layout classes
        for B, d, lanes in [(32768, 5, best), (32768, 64, best), (32768, 16, best),
                            (32768, 16, -4), (32768, 64, 1), (32768, 64, -8), (16384, 128, 16),
                            (16384, 128, 8), (32768, 64, 16), (32768, 16, 8), (32768, 16, 2),
                            (32768, 5, -1), (32768, 8, -1), (32768, 12, -1)]:
            resident(out, "a", B // k, T, d, a.reps, lanes, True, Ms, 10, False)
            torch.cuda.empty_cache()
    if "w" in a.cases:
        for B, d in ((2048, 5), (2048, 16), (2048, 32), (32768, 5)):
            resident(out, "w", B // k, T, d, a.reps_w, -1, False, Ms, 10, True)
            torch.cuda.empty_cache()
    if "x" in a.cases:
        for lanes in (-1, 1):
            resident(out, "x", 2048 // k, T, 64, a.reps_w, lanes, False, (2, 4), 10, True,
                     () if a.no_lane_groups else (1, 2, 4))
            torch.cuda.empty_cache()
    if "r" in a.cases:
        refill(out, 32768 // k, 10 * T, 64, a.reps, best, 4, (10, 100))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
