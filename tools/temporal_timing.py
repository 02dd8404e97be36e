"""Cost of the temporal opcodes: what they do to the kernels that share the
expression interpreter, and what they cost themselves.

    python tools/temporal_timing.py resources [--parent REV] [--out FILE]
    python tools/temporal_timing.py ab --parent-lib REL.so [--rows-log2 24] [--rounds 3] [--out FILE]

resources (no GPU): csrc/kernels_basic.hip is compiled for gfx950 with
-Rpass-analysis=kernel-resource-usage twice — from `git archive REV` (REV the
commit before this change; default HEAD) and from the working tree — and
the registers, scratch and occupancy of every kernel that instantiates
run_program (k_eval, which is also the filter kernel, and k_lam_pred / k_lam_map
/ k_lam_reduce) are tabulated.  Verdict: no kernel gains scratch, none loses
an occupancy step.

ab (one GPU): the yardstick uses only what both builds have — over 2^R rows of
two INTEGER columns, the projection (x % 7) + (x / 400) and the filter
x % 7 = 3 AND x / 400 > y — timed with the parent's library and with this
tree's, in child processes that alternate (CAPF_LIB_AB names the parent's
build, a path relative to the package directory; _lib.py).  Every child makes
2 warm-up runs and 4 timed ones, each a host clock around 16 evaluations of
the table operation and the session synchronise that ends them (the figure is
per evaluation); `--rounds` children per library
(3: 12 runs each).  The new library's median is compared with the parent's;
the margin is the parent's own min-to-max spread over its runs.  Then, with
this tree's library only and as information: d.year, d.week, ldt.microsecond
and d + duration('P1M3D') as projections of the same size, beside the
yardstick projection and a plain copy of a column (x + 0), 8 B in and 8 B out
per row each.

One JSON line per measurement goes to stdout; with --out the report is
appended to FILE (profiles/temporal_timing.txt holds one)."""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cypher-for-apache-flink_amd")
KERNELS = ("k_eval", "k_lam_pred", "k_lam_map", "k_lam_reduce")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-pass-failed", "-Wno-unused-result",
         "-munsafe-fp-atomics", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
         "csrc/kernels_basic.hip", "-o", os.devnull]
OPS_PER_RUN = 16  # table operations per timed run (one synchronise ends them): ~10 ms windows, not ~0.5 ms
FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("VGPRs Spill", "vgpr_spill"), ("SGPRs Spill", "sgpr_spill"))


def resource_usage(pkg_dir):
    """{kernel: {field: int}} from the compiler's remarks for kernels_basic.hip under pkg_dir."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc] + FLAGS, cwd=pkg_dir, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        raise SystemExit(p.stderr[-2000:])
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = next((k for k in KERNELS if re.search(r"\d" + k + r"E", m.group(1))), None)
            if cur:
                out[cur] = {}
            continue
        if cur:
            for label, key in FIELDS:
                m = re.search(r"\s" + re.escape(label) + r": (\d+)", line)
                if m:
                    out[cur][key] = int(m.group(1))
    return out


def resources(parent, report):
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "archive", parent, "cypher-for-apache-flink_amd/csrc", "include"], cwd=ROOT,
                            stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=ar.stdout, check=True)
        before = resource_usage(os.path.join(tmp, "cypher-for-apache-flink_amd"))
    after = resource_usage(PKG)
    rev = subprocess.run(["git", "rev-parse", "--short", parent], cwd=ROOT, stdout=subprocess.PIPE, text=True).stdout.strip()
    report(f"kernel resource usage, kernels_basic.hip for gfx950 (parent {rev} -> this tree)")
    report(f"{'kernel':14}" + "".join(f"{k:>16}" for _, k in FIELDS))
    ok = True
    for k in KERNELS:
        b, a = before[k], after[k]
        report(f"{k:14}" + "".join(f"{str(b[f]) + ' -> ' + str(a[f]):>16}" for _, f in FIELDS))
        ok = ok and a["scratch"] <= b["scratch"] and a["occupancy"] >= b["occupancy"]
        print(json.dumps({"kernel": k, "parent": b, "new": a}), flush=True)
    report("verdict: " + ("no kernel gains scratch, none loses an occupancy step" if ok else
                          "A KERNEL GAINED SCRATCH OR LOST OCCUPANCY"))
    return ok


# ------------------------------------------------------------------ run time
def child(what, rows_log2):
    """One process, one library (CAPF_LIB_AB or the tree's): JSON {name: [seconds]}."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import capf_import
    capf_import.load()
    from capf_amd import expr as ex
    from capf_amd.header import RecordHeader
    from capf_amd.table import GpuSession

    n = 1 << rows_log2
    s = GpuSession(0)
    rng = np.random.default_rng(7)
    x = rng.integers(0, 1 << 40, n, dtype=np.int64)
    y = rng.integers(0, 1 << 32, n, dtype=np.int64)
    X, Y, I = ex.Var("x"), ex.Var("y"), ex.IntegerLit
    cols = [("x", ex.T_INT, x, None), ("y", ex.T_INT, y, None)]
    runs = {
        "project": lambda t: t.withColumns((ex.Add(ex.Modulo(X, I(7)), ex.Divide(X, I(400))), "z"), header=H, params={}),
        "filter": lambda t: t.filter(ex.Ands(ex.Equals(ex.Modulo(X, I(7)), I(3)),
                                             ex.GreaterThan(ex.Divide(X, I(400)), Y)), header=H, params={}),
    }
    if what == "new":
        D, L = ex.Var("d"), ex.Var("l")
        cols += [("d", ex.T_DATE, x % 3000000 - 700000, None),
                 ("l", ex.T_LOCALDATETIME, (x % 3000000 - 700000) * 86400000000 + y * 20, None)]
        proj = lambda e: (lambda t: t.withColumns((e, "z"), header=H, params={}))  # noqa: E731
        runs = {
            "project": runs["project"],
            "copy": proj(ex.Add(X, I(0))),
            "d.year": proj(ex.DateProperty(D, "year")),
            "d.week": proj(ex.DateProperty(D, "week")),
            "ldt.microsecond": proj(ex.LocalDateTimeProperty(L, "microsecond")),
            "d + duration('P1M3D')": proj(ex.Add(D, ex.Duration(ex.StringLit("P1M3D")))),
        }
    H = RecordHeader({ex.Var(c[0]): c[0] for c in cols})
    t = s.table(cols).materialize()
    s.sync()
    out = {}
    for name, fn in runs.items():
        ts = []
        for i in range(6):  # 2 warm-ups, 4 timed
            s.sync()
            t0 = time.perf_counter()
            for _ in range(OPS_PER_RUN):
                fn(t).materialize()
            s.sync()
            if i >= 2:
                ts.append((time.perf_counter() - t0) / OPS_PER_RUN)
        out[name] = ts
    print("RESULT " + json.dumps(out), flush=True)


def run_child(what, rows_log2, lib):
    env = dict(os.environ)
    env.pop("CAPF_LIB_AB", None)
    if lib:
        env["CAPF_LIB_AB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", what, str(rows_log2)], env=env,
                       stdout=subprocess.PIPE, text=True, timeout=240)
    if p.returncode:
        raise SystemExit(f"child {what} ({lib or 'tree'}) ended with status {p.returncode}")
    return json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("RESULT "))[7:])


def ab(parent_lib, rows_log2, rounds, report):
    if not os.path.exists(os.path.join(PKG, parent_lib)):
        raise SystemExit(f"{parent_lib}: no such library under the package directory")
    times = {"parent": {}, "new": {}}
    for _ in range(rounds):  # alternating: parent, new, parent, new, ...
        for side, lib in (("parent", parent_lib), ("new", None)):
            for name, ts in run_child("yardstick", rows_log2, lib).items():
                times[side].setdefault(name, []).extend(ts)
    report(f"yardstick over 2^{rows_log2} rows, {4 * rounds} runs per library, alternating processes (ms)")
    ok = True
    for name in times["parent"]:
        p, q = times["parent"][name], times["new"][name]
        pm, qm, spread = statistics.median(p), statistics.median(q), max(p) - min(p)
        good = qm <= pm + spread
        ok = ok and good
        rec = {"yardstick": name, "parent_median_ms": pm * 1e3, "parent_spread_ms": spread * 1e3,
               "new_median_ms": qm * 1e3, "within_margin": good}
        print(json.dumps(rec), flush=True)
        report(f"  {name:8} parent median {pm * 1e3:8.3f}  spread (max - min) {spread * 1e3:7.3f}   "
               f"new median {qm * 1e3:8.3f}   {'within the margin' if good else 'SLOWER THAN THE MARGIN'}")
    report("verdict: " + ("the new library is no slower than the parent's own spread" if ok else "SLOWER"))
    new = run_child("new", rows_log2, None)
    base, cp = statistics.median(new["project"]), statistics.median(new["copy"])
    report(f"new opcodes as projections over 2^{rows_log2} rows, this tree's library (median of 4, ms; information)")
    for name, ts in new.items():
        m = statistics.median(ts)
        print(json.dumps({"projection": name, "median_ms": m * 1e3}), flush=True)
        report(f"  {name:24} {m * 1e3:8.3f}   x{m / base:5.2f} of the yardstick projection, x{m / cp:5.2f} of a column copy,"
               f" {16 * (1 << rows_log2) / m / 1e9:7.1f} GB/s of 8 B in + 8 B out")
    return ok


def main(argv):
    if argv and argv[0] == "child":
        return child(argv[1], int(argv[2]))
    opt = {"--parent": "HEAD", "--out": None, "--parent-lib": None, "--rows-log2": "24", "--rounds": "3"}
    mode, i = (argv[0] if argv else "resources"), 1
    while i < len(argv):
        opt[argv[i]] = argv[i + 1]
        i += 2
    lines = []

    def report(s):
        lines.append(s)
        print(s, flush=True)

    ok = resources(opt["--parent"], report) if mode == "resources" else \
        ab(opt["--parent-lib"], int(opt["--rows-log2"]), int(opt["--rounds"]), report)
    if opt["--out"]:
        with open(opt["--out"], "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
