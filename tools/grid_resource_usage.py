"""Resource report of the regret-grid kernels (csrc/ocx_alg_curve_etas.hip) beside the
step-size kernels they are derived from (csrc/ocx_alg_etas.hip).

    python tools/grid_resource_usage.py [--out profiles/grid_resource_usage.txt]

Cross-compiles both sources for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU
needed) and lists every grid instance next to the step-size instance with the same template
parameters (the ring depth NB aside: it is no part of the arithmetic, and three chained grid
instances run a shallower ring than their twins; the twin's NB is then shown): SGPRs, VGPRs,
AGPRs, scratch bytes per lane, waves per SIMD.  The last column flags
an instance that has scratch where its step-size twin has none (there must be
none).  The comparator kernel has no twin and is listed alone.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from online_convex_optimization_amd import _build  # noqa: E402

FIELDS = (("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"))
TWIN = {"ocx_alg_grid_kernel": "ocx_alg_etas_kernel",
        "ocx_alg_pipe_grid_kernel": "ocx_alg_pipe_etas_kernel"}
NB_AT = {"ocx_alg_grid_kernel": 3, "ocx_alg_pipe_grid_kernel": 2}
PARAMS = {"ocx_alg_grid_kernel": "C P CHAIN NB NE", "ocx_alg_pipe_grid_kernel": "C P NB RT NE",
          "ocx_grid_comp_kernel": "C P CHAIN NB NE"}


def report(src):
    """{(kernel, template args): {field: value}} of one source's resource remarks."""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([_build._hipcc(), *_build.CFLAGS,
                            "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(_build.CSRC, src), "-o", os.path.join(tmp, "o.o")],
                           capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-4000:])
    return parse(r.stderr)


def parse(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: _Z\d+(\w+?)I((?:L[ib]\d+E)+)E", line)
        if m:
            cur = out.setdefault((m.group(1), tuple(int(v) for v in
                                                    re.findall(r"L[ib](\d+)E", m.group(2)))), {})
            continue
        if "Function Name:" in line:
            cur = None
        if cur is None:
            continue
        for label, key in FIELDS:
            m = re.search(re.escape(label) + r": (\d+)", line)
            if m and line.split("remark:")[1].strip().startswith(label):
                cur[key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_resource_usage.txt"))
    ap.add_argument("--grid-log", help="saved compiler remarks of ocx_alg_curve_etas.hip")
    ap.add_argument("--etas-log", help="saved compiler remarks of ocx_alg_etas.hip")
    a = ap.parse_args()
    grid = parse(open(a.grid_log).read()) if a.grid_log else report("ocx_alg_curve_etas.hip")
    etas = parse(open(a.etas_log).read()) if a.etas_log else report("ocx_alg_etas.hip")
    cols = [k for _, k in FIELDS]
    lines = ["# hipcc " + " ".join(_build.CFLAGS) + " -Rpass-analysis=kernel-resource-usage",
             "# grid instance | " + " ".join(cols) + " | step-size twin: " + " ".join(cols) +
             " | flag"]
    bad = 0
    for (name, args), v in sorted(grid.items()):
        if name not in PARAMS:
            continue
        head = f"{name}<{', '.join(f'{p}={x}' for p, x in zip(PARAMS[name].split(), args))}>"
        mine = " ".join(str(v.get(c, "?")) for c in cols)
        if name in TWIN:
            i = NB_AT[name]
            twins = {k[1][i]: t for k, t in etas.items()
                     if k[0] == TWIN[name] and k[1][:i] + k[1][i + 1:] == args[:i] + args[i + 1:]}
            t = twins.get(args[i])
            if t is None and len(twins) == 1:
                (nb, t), = twins.items()
                head += f" (twin NB={nb})"
            if t is None:
                lines.append(f"{head} | {mine} | no twin | MISSING")
                bad += 1
                continue
            flag = "SCRATCH" if v.get("scratch", 0) > 0 and t.get("scratch", 0) == 0 else "ok"
            bad += flag != "ok"
            lines.append(f"{head} | {mine} | {' '.join(str(t.get(c, '?')) for c in cols)} | {flag}")
        else:
            lines.append(f"{head} | {mine} | - | -")
    lines.append(f"# instances with scratch where the step-size twin has none: {bad}")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
