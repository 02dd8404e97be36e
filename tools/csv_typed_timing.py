"""Timing of the typed CSV ingest (csrc/edge_list.hip k_csv_typed and the
interning of its STRING fields) against the host reader on one GPU.

    python tools/csv_typed_timing.py [--out profiles/csv_typed_timing.txt] [--log2-rows 16,20] [--reps 3]

One graph per size: a single node table of 2^k rows with an id, a nullable
INTEGER (1 in 8 NULL), a FLOAT (3 in 4 short decimals on the device's exact
path, 1 in 4 17-digit `repr` values for the host's slow path), a BOOLEAN, a
STRING drawn from 2^12 distinct values (some non-ASCII), a DATE and a
LOCALDATETIME, written by the seeded generator below into a temporary
directory in the FS graph layout.

Timed per size and route, under a host clock around `FSGraphSource.graph()`,
a materialize of the node table and a session synchronise:
 typed  the route of this commit (capf_csv_read_typed); `cold` is the first
        read of a fresh session (every string is new to the dictionary),
        `warm` the median of --reps further reads (every string is known);
        then one profiled read: per-kernel launches / ms / bytes, the number of
        FLOAT fields converted on the host, and the share of the kernel time
        spent interning (str_* and csv_typed_strings / _codes);
 host   the same file through the host reader `_parse_csv` and an upload (the
        route of the parent commit for this file), forced by a session proxy
        without the device entries; one cold and one warm read.
The typed result is compared with the host reader's on a sample of rows before
anything is reported.  Every GPU step is a child process of its own under a
time limit (--step-timeout); a step that fails or runs out of time ends the
run.  One JSON line per step goes to stdout and, with --out, is appended to
FILE.  No ratio is a target: nobody had measured either side."""
import argparse
import datetime
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = {"a_int": "INTEGER?", "b_flt": "FLOAT", "c_bool": "BOOLEAN", "d_str": "STRING", "e_date": "DATE",
         "f_dt": "LOCALDATETIME"}


def generate(root, log2_rows, seed=5):
    """The graph `t` under root: node table N of 2^log2_rows rows.  Returns the file's size."""
    rng = random.Random(seed)
    gdir = os.path.join(root, "t")
    os.makedirs(os.path.join(gdir, "nodes", "N"))
    with open(os.path.join(gdir, "capsGraphMetaData.json"), "w") as f:
        json.dump({"tableStorageFormat": "csv", "tags": [0]}, f)
    with open(os.path.join(gdir, "propertyGraphSchema.json"), "w") as f:
        json.dump({"version": "1.0", "labelPropertyMap": [{"labels": ["N"], "properties": PROPS}],
                   "relTypePropertyMap": []}, f)
    pool = [("name%d" % i) if i % 16 else ("näme-%d-名" % i) for i in range(1 << 12)]
    epoch = datetime.datetime(1970, 1, 1)
    path = os.path.join(gdir, "nodes", "N", "table.csv")
    with open(path, "w", encoding="utf-8", newline="") as f:
        for i in range(1 << log2_rows):
            r = rng.random()
            a = "" if i % 8 == 3 else str(rng.randrange(-10**9, 10**9))
            b = repr(r * 1000) if i % 4 == 1 else "%.3f" % (r * 1000)
            dt = epoch + datetime.timedelta(seconds=rng.randrange(-10**9, 2 * 10**9), microseconds=rng.randrange(10**6))
            f.write("%d,%s,%s,%s,%s,%s,%s\n" % (i, a, b, "true" if r < 0.5 else "false", pool[rng.randrange(len(pool))],
                                                 dt.date().isoformat(), dt.isoformat()))
    return os.path.getsize(path)


class HostOnly:
    """The session without its device CSV entries: FSGraphSource takes the host reader."""

    def __init__(self, s):
        self.table, self.empty = s.table, s.empty


def step(root, route, reps):
    sys.path.insert(0, ROOT)
    import capf_import
    capf_import.load()
    from capf_amd.fs_source import FSGraphSource
    from capf_amd.table import GpuSession
    sess = GpuSession(0)

    def read(s=sess):
        src = FSGraphSource(s if route == "typed" else HostOnly(s), root)
        sess.sync()
        t0 = time.perf_counter()
        t = src.graph("t").node_tables[0].table
        t.materialize()
        sess.sync()
        dt = time.perf_counter() - t0
        assert [r for _, r in src.routes] == [route], src.routes
        return t, dt

    t, cold = read()
    rec = {"route": route, "rows": t.size, "cold_ms": round(cold * 1e3, 2)}
    if route == "typed":  # the same values as the host reader's, on a sample of rows
        want, _ = FSGraphSource(HostOnly(sess), root).graph("t").node_tables[0].table, None
        for col in t.physicalColumns:
            g, w = t.column_values(col), want.column_values(col)
            stride = max(1, len(g) // 1000)
            assert [repr(x) for x in g[::stride]] == [repr(x) for x in w[::stride]], col
        del want
    warm = [read()[1] for _ in range(reps if route == "typed" else 1)]
    rec.update(warm_median_ms=round(statistics.median(warm) * 1e3, 2), warm_min_ms=round(min(warm) * 1e3, 2),
               reps=len(warm))
    if route == "typed":
        sess.set_profiling(True)
        sess.reset_profile()
        read()
        prof = {k: v for k, v in sess.profile().items()}
        sess.set_profiling(False)
        rec["slow_floats"] = sess.csv_slow_floats()
        rec["profile"] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4), "bytes": v["bytes"]}
                          for k, v in sorted(prof.items())}
        total = sum(v["total_ms"] for v in prof.values())
        interning = sum(v["total_ms"] for k, v in prof.items()
                        if k.startswith("str_") or k in ("csv_typed_strings", "csv_typed_codes"))
        rec["kernel_ms"] = round(total, 4)
        rec["interning_share_of_kernel_ms"] = round(interning / total, 4) if total else None
    sess.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log2-rows", default="16,20")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", nargs=2, metavar=("ROOT", "ROUTE"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        step(args.step[0], args.step[1], args.reps)
        return 0

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    emit("# python tools/csv_typed_timing.py " + " ".join(sys.argv[1:]))
    for k in args.log2_rows.split(","):
        root = tempfile.mkdtemp(prefix="csv_typed_")
        try:
            size = generate(root, int(k))
            for route in ("typed", "host"):
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", root, route,
                                        "--reps", str(args.reps)], capture_output=True, text=True,
                                       timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    emit(json.dumps({"log2_rows": int(k), "route": route, "error": "time limit"}))
                    return 1
                if r.returncode != 0:
                    emit(json.dumps({"log2_rows": int(k), "route": route, "error": r.stderr[-2000:]}))
                    return 1
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                emit(json.dumps({"log2_rows": int(k), "file_bytes": size, **rec}))
        finally:
            shutil.rmtree(root, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
