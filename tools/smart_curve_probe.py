"""SMART regret-curve timing probe: what K (horizon, threshold) pairs cost through
simulate_smart_curve, for every forced group size, next to K calls of simulate_smart on K
resident batches that hold the first t_k rows of the same data.  One JSON line per case,
appended to profiles/smart_curve_ab.jsonl (or --out).

  (a) generate_gT batches 32 768 x 1e3 x 5 and 32 768 x 1e3 x 64 (OCX_LANES_BEST), both closed
      forms on both sides, horizons 100, 200 … 1000, thresholds sqrt(2 t_k): group in
      {1, 2, 4} (forced through include/ocx_testing.h) and the dispatcher's own choice;
  (b) 2 048 x 1e3 x 5 in the bit-exact one-lane layout (1 x 6) with flags 0, the reference's
      prefix re-scan at every step (sqrt(2 t_k) is never reached on these rows): the existing
      side is the one-wave-per-sequence kernel, the curve re-scans in lane-group form;
  (c) the grid of (a) on further members of the dispatcher's classes (loop form x coordinates
      per lane), both closed forms, see main().

The baseline is existing code — K launches of the threshold sweep kernel's one-column
instance (a), of the one-wave kernel (b) — never the curve kernel's own group-1 form.  The
truncated batches are packed from the full batch's rows (DeviceBatch.rows_of), so column k of
the curve and call k of the loop see the same numbers; every record reports whether they gave
the same switch steps and the largest regret difference.  One process; device events on the
stream around every repetition; every shape warmed up; the sides of a comparison alternate
repetition by repetition.  The spread reported is that of the loop in the same call.  --small
runs toy sizes (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from online_convex_optimization_amd import _lib, engine  # noqa: E402

SQ2 = math.sqrt(2)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(sides, reps, warm=2):
    """{name: [ms] * reps}, the sides taking turns."""
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    return ms


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
            "stdev_ms": statistics.pstdev(v), "reps": len(v)}


def resident(out, case, B, T, d, reps, lanes, closed, horizons, scale):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    groups = [g for g in (1, 2, 4) if g == 1 or db.L.C <= 8 or (g == 2 and db.L.C <= 16)]
    K = len(horizons)
    ths = [scale * math.sqrt(2 * t) for t in horizons]
    # the truncated batches, from the same rows
    zr, yr = db.rows_of(torch.arange(B, device=db.device))
    cut = []
    for t in horizons:
        c = engine.DeviceBatch(B, t, d, lanes_per_seq=lanes).pack(zr[:, :t], yr[:, :t])
        assert (c.L.P, c.L.C, c.L.chain) == (db.L.P, db.L.C, db.L.chain)
        cut.append(c)
    torch.cuda.synchronize()
    del zr, yr
    for c in cut:
        c._keep = None
    torch.cuda.empty_cache()
    sws = [torch.zeros(B, dtype=torch.int64, device=db.device) for _ in horizons]
    res = {}

    def loop():
        for c, th, sw in zip(cut, ths, sws):
            c.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=closed,
                             closed_comparator=closed)

    sides = {"loop": loop}
    for g in groups + [None]:
        name = "auto" if g is None else f"group{g}"
        sides[name] = (lambda g=g, name=name: res.__setitem__(
            name, db.simulate_smart_curve(horizons, ths, SQ2, closed_prefix=closed,
                                          closed_comparator=closed, _group=g)))
    ms = alternate(sides, reps)
    base = stats(ms["loop"])
    torch.cuda.synchronize()
    loop_sw = torch.stack(sws, dim=1)
    loop_reg = torch.stack([c.regret[:B] for c in cut], dim=1)
    rec = {"case": case, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
           "closed_forms": closed, "K": K, "horizons": list(horizons), "thresholds": ths,
           "auto_group": int(_lib.load().ocx_smart_curve_group(ctypes.byref(db.L), K)),
           "mean_switch_step_per_column": [float(x) for x in
                                           loop_sw.double().mean(dim=0).cpu().tolist()],
           "never_switched_per_column": [int(x) for x in (loop_sw < 0).sum(dim=0).cpu().tolist()],
           "loop": base}
    for name in sides:
        if name == "loop":
            continue
        s = stats(ms[name])
        rec[name] = dict(s, ratio_median=s["median_ms"] / base["median_ms"],
                         inside_loop_spread=base["min_ms"] <= s["median_ms"] <= base["max_ms"],
                         switch_steps_equal=bool(torch.equal(res[name]["switch_step"], loop_sw)),
                         max_abs_diff=float((res[name]["regret"] - loop_reg).abs().max()))
    out(rec)
    del db, cut


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "smart_curve_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-b", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--cases", default="abc")
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
    horizons = [T * i // 10 for i in range(1, 11)]
    if "a" in a.cases:
        for d in (5, 64):
            resident(out, "a", 32768 // k, T, d, a.reps, engine.LANES_BEST, True, horizons, 1.0)
            torch.cuda.empty_cache()
    if "b" in a.cases:
        resident(out, "b", 2048 // k, T, 5, a.reps_b, -1, False, horizons, 1.0)
        torch.cuda.empty_cache()
    if "c" in a.cases:
        # the classes tools/thresholds_probe.py walks: chained 2 x 8 (d = 16), 4 x 4 (d = 16 on
        # 4 lanes), 4 x 16 (d = 64 in the exact mode) and the long chain 8 x 8; butterfly
        # 16 x 8 and 8 x 16 (d = 128), 16 x 4 (d = 64), 8 x 2 (d = 16) and 2 x 8 (d = 16); one
        # lane of 6, 8 and 12 coordinates
        extra = [(32768, 16, engine.LANES_BEST), (32768, 16, -4), (32768, 64, 1),
                 (32768, 64, -8), (16384, 128, 16), (16384, 128, 8), (32768, 64, 16),
                 (32768, 16, 8), (32768, 16, 2), (32768, 5, -1), (32768, 8, -1),
                 (32768, 12, -1)]
        for B, d, lanes in extra:
            resident(out, "c", B // k, T, d, a.reps, lanes, True, horizons, 1.0)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
