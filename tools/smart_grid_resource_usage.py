"""Resource report of the SMART regret-grid kernels (csrc/ocx_smart_grid.hip,
csrc/ocx_smart_wave_grid.hip) beside the curve kernels they are derived from
(csrc/ocx_smart_curve.hip, csrc/ocx_smart_wave_cols.hip).

    python tools/smart_grid_resource_usage.py [--out profiles/smart_grid_resource_usage.txt]

Cross-compiles the four sources for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU
needed) and lists every grid instance next to the curve instance with the same template
parameters (the ring depth NB aside: it is no part of the arithmetic, and three grid instances
run a shallower ring than their twins; the twin's NB is then shown): SGPRs, VGPRs, AGPRs,
scratch bytes per lane, waves per SIMD, LDS bytes per block.  The last column flags an instance
that has scratch where its curve twin has none (SCRATCH) or fewer waves per SIMD (WAVES):
DESIGN.md §3.17 allows neither.  A curve instance whose grid form is not compiled is listed as
such.  Exit status 1 if any instance is flagged.
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
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"))
TWIN = {"ocx_smart_grid_kernel": ("ocx_smart_curve.hip", "ocx_smart_curve_kernel"),
        "ocx_smart_wave_grid_kernel": ("ocx_smart_wave_cols.hip", "ocx_smart_wave_cols_kernel")}
SOURCE = {"ocx_smart_grid_kernel": "ocx_smart_grid.hip",
          "ocx_smart_wave_grid_kernel": "ocx_smart_wave_grid.hip"}
NB_AT = {"ocx_smart_grid_kernel": 3}
PARAMS = {"ocx_smart_grid_kernel": "C P CHAIN NB NT", "ocx_smart_wave_grid_kernel": "DMAX NT"}


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
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "smart_grid_resource_usage.txt"))
    a = ap.parse_args()
    cols = [k for _, k in FIELDS]
    lines = ["# hipcc " + " ".join(_build.CFLAGS) + " -Rpass-analysis=kernel-resource-usage",
             "# grid instance | " + " ".join(cols) + " | curve twin: " + " ".join(cols) +
             " | flag"]
    bad = 0
    for name in sorted(TWIN):
        grid = report(SOURCE[name])
        twins = report(TWIN[name][0])
        seen = set()
        for (kname, args), v in sorted(grid.items()):
            if kname != name:
                continue
            head = f"{name}<{', '.join(f'{p}={x}' for p, x in zip(PARAMS[name].split(), args))}>"
            mine = " ".join(str(v.get(c, "?")) for c in cols)
            t = twins.get((TWIN[name][1], args))
            seen.add(args)
            if t is None and name in NB_AT:   # a shallower ring than the twin's
                i = NB_AT[name]
                alike = {k[1]: u for k, u in twins.items() if k[0] == TWIN[name][1] and
                         k[1][:i] + k[1][i + 1:] == args[:i] + args[i + 1:]}
                if len(alike) == 1:
                    (targs, t), = alike.items()
                    head += f" (twin NB={targs[i]})"
                    seen.add(targs)
            if t is None:
                lines.append(f"{head} | {mine} | no twin | MISSING")
                bad += 1
                continue
            flag = ("SCRATCH" if v.get("scratch", 0) > 0 and t.get("scratch", 0) == 0 else
                    "WAVES" if v.get("occ", 0) < t.get("occ", 0) else "ok")
            bad += flag != "ok"
            lines.append(f"{head} | {mine} | {' '.join(str(t.get(c, '?')) for c in cols)} | {flag}")
        for (kname, args), t in sorted(twins.items()):
            if kname == TWIN[name][1] and args not in seen:
                head = f"{name}<{', '.join(f'{p}={x}' for p, x in zip(PARAMS[name].split(), args))}>"
                lines.append(f"{head} | not compiled | {' '.join(str(t.get(c, '?')) for c in cols)}"
                             " | -")
    lines.append("# instances with scratch where the curve twin has none, or fewer waves per "
                 f"SIMD: {bad}")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
