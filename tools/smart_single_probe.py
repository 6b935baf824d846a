"""Single-threshold SMART timing probe: DeviceBatch.simulate_smart on resident generate_gT
data, one library per process, for comparing two builds of libocx.so.

    OCX_LIB=<library> python tools/smart_single_probe.py time --label parent --out runs.jsonl
    python tools/smart_single_probe.py compare runs.jsonl --parent parent --new new

`time` appends one record per case to --out: device events on the batch's stream around
every repetition, 2 warm-up rounds, 20 repetitions (tools/thresholds_probe.py's method).
Two builds cannot share a process, so a comparison is runs in turn (parent, new, parent,
new); `compare` reads them and appends one record per case to --out (default
profiles/smart_single_ab.jsonl): the medians of every run, the parent's margin (the min-max
half-width of its slower run) and whether the new build's slower median is at or below the
parent's slower median plus that margin.  --small runs toy sizes (a rehearsal of the script,
not a measurement).

--mode closed (the default): both closed forms, in the layouts of CASES.  The threshold is
sqrt(2T)/10, which spreads the switches over the horizon on sampler rows (the record reports
where they fell).

--mode rescan: neither closed form and no stats tensor, lanes_per_seq = 1, the sizes of
RESCAN_CASES: the reference's prefix re-scan, which at these sizes runs the
one-wave-per-sequence kernel (ocx_launch_smart_wave).  Two thresholds
per size: sqrt(2T), never reached on sampler rows (every step re-scans its prefix, the worst
case), and sqrt(2T)/10."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SQ2 = math.sqrt(2)
BEST = 128  # engine.LANES_BEST
# (name, B, d, lanes_per_seq): B fills the device at T = 1000
CASES = [("2x4 chained", 32768, 5, BEST), ("8x8 butterfly", 32768, 64, BEST),
         ("1x8", 32768, 8, -1), ("1x32", 32768, 32, -1), ("32x32 butterfly", 4096, 1024, BEST),
         ("1x24", 32768, 24, -1), ("8x16 chained", 16384, 128, -8)]
# --mode rescan: (B, d) at T = 1000, lanes_per_seq = 1; the 32 768 batches queue 32 waves per
# SIMD on the one-wave-per-sequence kernel
RESCAN_CASES = [(768, 5), (1, 5), (2048, 5), (2048, 8), (2048, 16), (2048, 32), (2048, 64),
                (32768, 5), (32768, 8), (32768, 16)]
# threshold / sqrt(2T): 1 never switches on sampler rows (the full O(T^2) re-scan), 0.1 spreads
# the switches over the horizon
RESCAN_SCALES = [("never", 1.0), ("spread", 0.1)]


def cases_of(mode):
    """(name, B, d, lanes_per_seq, threshold scale, closed forms) of every record."""
    if mode == "closed":
        return [(name, B, d, lanes, 0.1, True) for name, B, d, lanes in CASES]
    return [(f"rescan {B}x{d} {kind}", B, d, 1, scale, False)
            for B, d in RESCAN_CASES for kind, scale in RESCAN_SCALES]


def time_cases(a):
    import torch
    from online_convex_optimization_amd import _lib, engine
    from thresholds_probe import alternate, stats
    engine.release_buffers(0)
    T = 250 if a.small else 1000
    with open(a.out, "a") as f:
        for name, B, d, lanes, scale, closed in cases_of(a.mode):
            B = max(1, B // 16) if a.small else B
            db = engine.DeviceBatch(B, T, d, lanes_per_seq=lanes).generate_gT(base_seed=0)
            sw = torch.zeros(B, dtype=torch.int64, device=db.device)
            th = scale * math.sqrt(2 * T)
            ms = alternate({"single": lambda: db.simulate_smart(
                th, SQ2, switch_step=sw, closed_prefix=closed, closed_comparator=closed)}, a.reps)
            torch.cuda.synchronize()
            rec = dict(stats(ms["single"]), label=a.label, lib=os.path.basename(_lib.LIB_PATH),
                       case=name, mode=a.mode, B=B, T=T, d=d,
                       layout=[db.L.P, db.L.C, db.L.chain],
                       thresh=th, mean_switch_step=float(sw.double().mean()),
                       never_switched=int((sw < 0).sum()),
                       regret_sum=float(db.regret[:B].sum()).hex(), small=a.small)
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            del db, sw
            torch.cuda.empty_cache()


def compare(a):
    runs = [json.loads(l) for l in open(a.runs)]
    with open(a.out, "a") as f:
        for name in dict.fromkeys(r["case"] for r in runs):   # the runs' cases, in their order
            par = [r for r in runs if r["case"] == name and r["label"] == a.parent]
            new = [r for r in runs if r["case"] == name and r["label"] == a.new]
            slow = max(par, key=lambda r: r["median_ms"])
            margin = (slow["max_ms"] - slow["min_ms"]) / 2
            bound = slow["median_ms"] + margin
            worst = max(r["median_ms"] for r in new)
            base = statistics.mean(r["median_ms"] for r in par)
            rec = {"case": name, "mode": par[0].get("mode", "closed"),
                   **{k: par[0][k] for k in ("B", "T", "d", "layout", "thresh", "small")},
                   "parent_commit": a.parent_commit, "note": a.note,
                   "parent_median_ms": [r["median_ms"] for r in par],
                   "parent_min_max_ms": [[r["min_ms"], r["max_ms"]] for r in par],
                   "new_median_ms": [r["median_ms"] for r in new],
                   "new_min_max_ms": [[r["min_ms"], r["max_ms"]] for r in new],
                   "margin_ms": margin, "bound_ms": bound,
                   "ratio_new_over_parent": [r["median_ms"] / base for r in new],
                   "margin_over_parent": margin / base, "within_margin": worst <= bound,
                   "same_results": len({(r["regret_sum"], r["mean_switch_step"])
                                        for r in par + new}) == 1}
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--label", required=True)
    t.add_argument("--out", required=True)
    t.add_argument("--reps", type=int, default=20)
    t.add_argument("--small", action="store_true")
    t.add_argument("--mode", choices=("closed", "rescan"), default="closed")
    c = sub.add_parser("compare")
    c.add_argument("runs")
    c.add_argument("--parent", default="parent")
    c.add_argument("--new", default="new")
    c.add_argument("--parent-commit", default=None)
    c.add_argument("--note", default=None, help="what the new build is, copied into the records")
    c.add_argument("--out", default=os.path.join(ROOT, "profiles", "smart_single_ab.jsonl"))
    a = ap.parse_args()
    (time_cases if a.cmd == "time" else compare)(a)


if __name__ == "__main__":
    main()
