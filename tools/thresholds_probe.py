"""Threshold sweep timing probe: what M switch thresholds cost through
simulate_smart_thresholds, for every forced group size, next to M separate calls of
simulate_smart on the same resident data.  One JSON line per case, appended to
profiles/thresholds_ab.jsonl (or --out).

  (a) generate_gT batches 32 768 x 1e3 x 5 and 32 768 x 1e3 x 64 (OCX_LANES_BEST), both closed
      forms on both sides: M x simulate_smart() against the sweep with M in {2, 4, 7}, group
      in {1, 2, 4} (forced through include/ocx_testing.h) and the dispatcher's own choice;
  (b) 2 048 x 1e3 x 5 in the exact layout with flags 0, the reference's prefix re-scan: the
      existing side is the one-wave-per-sequence kernel, the sweep re-scans in lane-group form;
  (c) M in {2, 4} on further members of the dispatcher's classes (loop form x coordinates per
      lane), see main().

The committed records were taken when simulate_smart() with the closed forms ran a
single-threshold kernel of its own: there the baseline was the existing code, never the sweep
code.  That call is now one launch of the sweep kernel's one-column instance, so in cases (a)
and (c) the "loop" side runs the same kernel as group 1 and their ratio measures the sweep
wrapper's host path only (tools/smart_single_probe.py has the single call across the merge);
the committed records stay as the evidence of that earlier commit.  In case (b) the loop side
is still another kernel.  Thresholds are sqrt(2T) and
fractions of it, so the switches are spread over the horizon.  One process; device events on
the batch's stream around every repetition; every shape warmed up; the sides of a comparison
alternate repetition by repetition, so both see the same neighbours on the machine.  The
spread reported is that of the existing path in the same call.  --small runs toy sizes (a
rehearsal of the script, not a measurement)."""
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
# of sqrt(2T): on sampler rows FTL's regret so far stays far below sqrt(2T), so the fractions
# are small (each record reports where its columns switched)
FRACTIONS = [1.0, 0.02, 0.05, 0.1, 0.2, 0.01, 0.5]


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


def resident(out, case, B, T, d, reps, lanes, closed, Ms):
    db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
    groups = [g for g in (1, 2, 4) if g == 1 or db.L.C <= 8 or (g == 2 and db.L.C <= 16)]
    sw = torch.zeros(B, dtype=torch.int64, device=db.device)
    for M in Ms:
        ths = [f * math.sqrt(2 * T) for f in FRACTIONS[:M]]
        res = {}

        def loop(ths=ths):
            for th in ths:
                db.simulate_smart(th, SQ2, switch_step=sw, closed_prefix=closed,
                                  closed_comparator=closed)

        sides = {"loop": loop}
        for g in groups + [None]:
            name = "auto" if g is None else f"group{g}"
            sides[name] = (lambda g=g, name=name, ths=ths: res.__setitem__(
                name, db.simulate_smart_thresholds(ths, SQ2, closed_prefix=closed,
                                                   closed_comparator=closed, _group=g)))
        ms = alternate(sides, reps)
        base = stats(ms["loop"])
        torch.cuda.synchronize()   # db.regret and sw hold the last threshold's run
        swh = res["auto"]["switch_step"]
        rec = {"case": case, "B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C, db.L.chain],
               "closed_forms": closed, "M": M, "thresholds": ths,
               "auto_group": int(_lib.load().ocx_smart_thresholds_group(ctypes.byref(db.L), M)),
               "mean_switch_step_per_column": [float(x) for x in
                                               swh.double().mean(dim=0).cpu().tolist()],
               "never_switched_per_column": [int(x) for x in (swh < 0).sum(dim=0).cpu().tolist()],
               "loop": base}
        for name in sides:
            if name == "loop":
                continue
            s = stats(ms[name])
            rec[name] = dict(s, ratio_median=s["median_ms"] / base["median_ms"],
                             inside_loop_spread=base["min_ms"] <= s["median_ms"] <= base["max_ms"],
                             last_column_switch_steps_equal=bool(
                                 torch.equal(res[name]["switch_step"][:, -1], sw)),
                             last_column_max_abs_diff=float(
                                 (res[name]["regret"][:, -1] - db.regret[:B]).abs().max()))
        out(rec)
    del db


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "thresholds_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=20)
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
    if "a" in a.cases:
        for d in (5, 64):
            resident(out, "a", 32768 // k, 1000 // (4 if a.small else 1), d, a.reps,
                     engine.LANES_BEST, True, (2, 4, 7))
            torch.cuda.empty_cache()
    if "b" in a.cases:
        resident(out, "b", 2048 // k, 1000 // (4 if a.small else 1), 5, a.reps, 1, False, (2, 4, 7))
        torch.cuda.empty_cache()
    if "c" in a.cases:
        # further members of the classes (loop form x coordinates per lane), both closed forms:
        # chained 2 x 8 (d = 16), 4 x 4 (d = 16 on 4 lanes), 4 x 16 (d = 64 in the exact mode)
        # and the long chain 8 x 8; butterfly 16 x 8 and 8 x 16 (d = 128), 16 x 4 (d = 64),
        # 8 x 2 (d = 16) and 2 x 8 (d = 16); one lane of 6, 8 and 12 coordinates
        extra = [(32768, 1000, 16, engine.LANES_BEST), (32768, 1000, 16, -4),
                 (32768, 1000, 64, 1), (32768, 1000, 64, -8), (16384, 1000, 128, 16),
                 (16384, 1000, 128, 8), (32768, 1000, 64, 16), (32768, 1000, 16, 8),
                 (32768, 1000, 16, 2), (32768, 1000, 5, -1), (32768, 1000, 8, -1),
                 (32768, 1000, 12, -1)]
        for B, T, d, lanes in extra:
            resident(out, "c", B // k, T // (4 if a.small else 1), d, a.reps, lanes, True, (2, 4))
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
