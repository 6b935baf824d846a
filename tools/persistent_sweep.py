"""Operating point of the pipelined FTRL kernel's persistent launch (ocx_alg_pipe.hip): ring
depth x resident waves per SIMD x block shape, at the bench batch.

    python tools/persistent_sweep.py --build        # no GPU: the tuning builds + resource reports
    python tools/persistent_sweep.py --run OUT.jsonl   # on the GPU: the sweep table

--build compiles one tuning build of ocx_alg_pipe.hip per (ring slots NB, register budget
512 / MINW) with _build.build_variant into OCX_TUNE_DIR (default tune_pw), the compiler's
kernel-resource-usage remarks beside it, and writes <dir>/sweep_builds.json: per build the
persistent FTRL instance's VGPRs, scratch and occupancy.  A build with scratch, or whose
registers do not admit the occupancy its MINW asks for, is listed as skipped there and its
library removed.

--run times every remaining build at every (waves per SIMD, block shape) it places evenly:
four-wave blocks at any wps up to the build's occupancy (the launch caps blocks per CU with a
dynamic-LDS request), one-wave blocks only at wps = the build's occupancy, where the registers
are the cap.  Each point: FTRL regrets bit-identical to the reference library's (the first of
--ref, default the product library), then the kernel time over --rounds launches (HIP events),
the reference timed again beside every build so each point has its yardstick from the same
minutes.  One JSON line per point, skipped builds included.
"""
import argparse
import concurrent.futures as cf
import ctypes
import json
import math
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TUNE = os.path.join(ROOT, os.environ.get("OCX_TUNE_DIR", "tune_pw"))

NBS = (4, 5, 6, 9)   # ring slots: NB - 2 = 2, 3, 4, 7 steps in flight
MINWS = (4, 2)       # __launch_bounds__ minimum waves per SIMD: <= 128, <= 256 VGPRs
WPS = (1, 2, 4)


def vname(nb, minw):
    return f"nb{nb}w{minw}"


def build_one(nb, minw):
    from online_convex_optimization_amd import _build
    _build.build_variant(vname(nb, minw),
                         [f"OCX_PIPE_PERS_NB={nb}", f"OCX_PIPE_PERS_MINW={minw}",
                          "OCX_PIPE_PERS_TUNE=1"], source="ocx_alg_pipe.hip", out_dir=TUNE)


def resources(report, nb, minw):
    """The persistent FTRL instance <8, 8, nb, false, minw, false, true> in the remarks."""
    want = f"ocx_alg_pipe_kernelILi8ELi8ELi{nb}ELb0ELi{minw}ELb0ELb1EE"
    out, on = {}, False
    for line in report.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            on = want in m.group(1)
            continue
        if not on:
            continue
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"),
                         ("sgprs", r" SGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and key not in out:
                out[key] = int(m.group(1))
    return out


def do_build():
    os.makedirs(TUNE, exist_ok=True)
    from online_convex_optimization_amd import _build
    _build.build(jobs=8)
    env = dict(os.environ, HIPCC_COMPILE_FLAGS_APPEND="-Rpass-analysis=kernel-resource-usage")

    def one(p):
        nb, minw = p
        log = os.path.join(TUNE, vname(nb, minw) + ".resources.txt")
        with open(log, "w") as f:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--build-one",
                                f"{nb},{minw}"], env=env, stderr=f, stdout=f)
        return nb, minw, r.returncode, log

    table = []
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        for nb, minw, rc, log in ex.map(one, [(nb, w) for w in MINWS for nb in NBS]):
            with open(log) as f:
                res = resources(f.read(), nb, minw)
            row = {"build": vname(nb, minw), "NB": nb, "steps_in_flight": nb - 2, "MINW": minw,
                   **res}
            if rc != 0 or not res:
                row["skipped"] = "build failed"
            elif res.get("scratch", 0) > 0:
                row["skipped"] = f"scratch: {res['scratch']} B per lane"
            elif res.get("occupancy", 0) < minw:
                row["skipped"] = (f"{res.get('vgprs')} VGPRs admit {res.get('occupancy')} waves "
                                  f"per SIMD, not the {minw} intended")
            if "skipped" in row:
                lib = os.path.join(TUNE, f"libocx_{vname(nb, minw)}.so")
                if os.path.exists(lib):
                    os.remove(lib)
            table.append(row)
            print(json.dumps(row), flush=True)
    with open(os.path.join(TUNE, "sweep_builds.json"), "w") as f:
        json.dump(table, f, indent=1)


def do_run(out_path, ref_names, rounds, B, T, d):
    import torch
    from online_convex_optimization_amd import _lib, engine

    def lib(name):
        path = (os.path.join(ROOT, "online_convex_optimization_amd", "libocx.so") if name == "main"
                else os.path.join(TUNE, f"libocx_{name}.so"))
        L = ctypes.CDLL(path)
        L.ocx_dev_simulate_alg_ex.argtypes = _lib.SIGNATURES["ocx_dev_simulate_alg_ex"][1]
        return L

    with open(os.path.join(TUNE, "sweep_builds.json")) as f:
        builds = json.load(f)
    st = torch.cuda.current_stream()
    db = engine.DeviceBatch(B, T, d).generate_gT(base_seed=0)
    out = open(out_path, "w")

    def emit(row):
        out.write(json.dumps(row) + "\n")
        out.flush()
        print(json.dumps(row), flush=True)

    def launch(L):
        return L.ocx_dev_simulate_alg_ex(ctypes.byref(db.L), db.z.data_ptr(), db.y.data_ptr(), 0,
                                         math.sqrt(2), None, db.regret.data_ptr(), None, None,
                                         None, _lib.OCX_ALG_CLIPPED_ROWS, None,
                                         ctypes.c_void_p(st.cuda_stream))

    def timed(L):
        ms = []
        for _ in range(rounds):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(st)
            rc = launch(L)
            e.record(st)
            torch.cuda.synchronize()
            if rc != 0:
                return None
            ms.append(s.elapsed_time(e))
        ms.sort()
        return {"kernel_ms_min": ms[0], "kernel_ms_median": ms[len(ms) // 2], "kernel_ms_max": ms[-1]}

    refs = [(n, lib(n)) for n in ref_names]
    assert launch(refs[0][1]) == 0
    torch.cuda.synchronize()
    want = db.regret[:B].clone()
    shape = {"B": B, "T": T, "d": d, "layout": [db.L.P, db.L.C], "groups": db.L.G, "rounds": rounds}

    def ref_rows(tag):
        for n, L in refs:
            launch(L)
            torch.cuda.synchronize()
            same = bool(torch.equal(db.regret[:B], want))
            emit({"lib": n, "role": "reference", "beside": tag, **shape, **(timed(L) or {}),
                  "bitidentical": same})

    ref_rows("start")
    for b in builds:
        if "skipped" in b:
            emit({"lib": b["build"], **{k: b[k] for k in b if k != "build"}, **shape})
            continue
        L = lib(b["build"])
        occ = b["occupancy"]
        points = [(w, 4) for w in WPS if w <= occ] + ([(occ, 1)] if occ in WPS else [])
        for wps, bw in points:
            os.environ["OCX_PIPE_PERS_WPS"] = str(wps)
            os.environ["OCX_PIPE_PERS_BW"] = str(bw)
            row = {"lib": b["build"], "NB": b["NB"], "steps_in_flight": b["NB"] - 2,
                   "MINW": b["MINW"], "vgprs": b.get("vgprs"), "scratch": b.get("scratch"),
                   "occupancy": occ, "waves_per_simd": wps, "block_waves": bw, **shape}
            db.regret.zero_()
            rc = launch(L)
            torch.cuda.synchronize()
            if rc != 0:
                row["skipped"] = "launch refused: " + _lib.last_error()
                emit(row)
                continue
            row["bitidentical"] = bool(torch.equal(db.regret[:B], want))
            row.update(timed(L) or {"skipped": "launch failed"})
            emit(row)
        ref_rows(b["build"])
    out.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--build-one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--run", metavar="OUT.jsonl", default=None)
    ap.add_argument("--ref", default="main", help="reference libraries, the first the yardstick")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--B", type=int, default=32768)
    ap.add_argument("--T", type=int, default=10000)
    ap.add_argument("--d", type=int, default=64)
    a = ap.parse_args()
    if a.build_one:
        nb, minw = (int(x) for x in a.build_one.split(","))
        build_one(nb, minw)
    elif a.build:
        do_build()
    elif a.run:
        do_run(a.run, a.ref.split(","), a.rounds, a.B, a.T, a.d)
    else:
        ap.error("--build or --run")


if __name__ == "__main__":
    main()
