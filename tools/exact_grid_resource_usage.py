"""Resource report of the FTRL-vs-exact-FTL regret-grid kernels (csrc/ocx_ftrl_exact_grid.hip).

    python tools/exact_grid_resource_usage.py [--out profiles/exact_grid_resource_usage.txt]

Cross-compiles the source for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed)
and lists every instance of the loop kernel and of the comparator kernel: SGPRs, VGPRs, AGPRs,
scratch bytes per lane, waves per SIMD.  The last column of a loop instance with NE > 1 flags
scratch where the NE = 1 instance of the same (C, P, sums) has none (such an
instance must not be offered; the exit status is the number of them).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from online_convex_optimization_amd import _build  # noqa: E402
from grid_resource_usage import FIELDS, parse, report  # noqa: E402

LOOP, COMP = "ocx_ftrl_exact_grid_kernel", "ocx_ftrl_exact_grid_comp_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "exact_grid_resource_usage.txt"))
    ap.add_argument("--log", help="saved compiler remarks of ocx_ftrl_exact_grid.hip")
    a = ap.parse_args()
    res = parse(open(a.log).read()) if a.log else report("ocx_ftrl_exact_grid.hip")
    cols = [k for _, k in FIELDS]
    fmt = lambda v: " ".join(f"{v.get(c, '?'):>5}" for c in cols)  # noqa: E731
    lines = ["# hipcc " + " ".join(_build.CFLAGS) + " -Rpass-analysis=kernel-resource-usage",
             f"# {LOOP} (loop), {COMP} (comp); columns per kernel: " + " ".join(cols),
             "#  C   P chain NB NE | loop                          | comp"
             "                          | flag"]
    bad = 0
    for (name, args), v in sorted(res.items()):
        if name != LOOP:
            continue
        C, P, chain, NB, NE = args
        one = [t for (n, g), t in res.items() if n == LOOP and g[:3] == args[:3] and g[4] == 1]
        comp = res.get((COMP, args), {})
        flag = "-"
        if NE > 1:
            flag = "SCRATCH" if v.get("scratch", 0) > 0 and one and \
                one[0].get("scratch", 0) == 0 else "ok"
            bad += flag == "SCRATCH"
        lines.append(f"{C:4d} {P:3d} {chain:5d} {NB:2d} {NE:2d} | {fmt(v)} | {fmt(comp)} | {flag}")
    lines.append(f"# NE > 1 loop instances with scratch where NE = 1 has none: {bad}")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return bad


if __name__ == "__main__":
    sys.exit(main())
